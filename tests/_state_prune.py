"""Store-prune test helpers: the stores the fixtures recorded from the reference give
(tests/golden/state_update.json, state_remove.json: base nodes, then every batch's emitted nodes),
the mirror's prune of a list of nodes (plenum_gpu.state_store.reachable_host), the host build of
csrc/pv_trie_prune.h (tools/hostcheck/stateprunecheck.cpp), hand-encoded stores for what the
fixtures cannot show and the case file of stateprunecheck_asan."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import _state_apply as sa
import _state_build as sb
import _state_proofs as sp
import _state_update as su
from plenum_gpu.state_proofs import rlp_encode
from plenum_gpu.state_store import reachable_host

HC_DIR = sb.HC_DIR
PR_OK, PR_NO_ROOTS, PR_ROOT_MISSING, PR_DIGEST_CAP, PR_NESTING = range(5)   # stateprune_host.h
MAX_INLINE = 7                                                              # pv_trie_prune.h: TP_MAX_INLINE
_lib = None
_cache = {}
sha3 = sb.sha3


# ------------------------------------------------------------------ the stores
def fixture_cases():
    """[(name, fixture module, case)]: 'up/..' of state_update.json, 'rm/..' of state_remove.json"""
    return [('up/' + c.name, su, c) for c in su.fixture()] + [('rm/' + c.name, sa, c) for c in sa.fixture()]


def shape_names():
    return [n for n, _, _ in fixture_cases()] + ['wave63', 'wave64', 'wave65', 'chain', 'mixed4096']


def filled(name):
    """one shape through the host twins of the build and the apply / update, cached -> (the store's
    nodes in the order they were added: the base's, then each batch's emitted ones, [base root,
    the root after each batch])"""
    if name not in _cache:
        if name[:3] in ('up/', 'rm/'):
            mod = su if name[:3] == 'up/' else sa
            _, base, batches = next(s for s in mod.fixture_shapes() if s[0] == 'fx/' + name[3:])
            b0, outs, _ = mod.host_run('fx/' + name[3:], base, batches)
        else:
            _, base, batches = next(s for s in sa.shapes() if s[0] == name)
            b0, outs, _ = sa.host_run(name, base, batches)
        nodes = list(b0.nodes())
        for b in outs:
            nodes += b.nodes()
        _cache[name] = (nodes, [b0.root] + [b.root for b in outs])
    return _cache[name]


class Want:
    """what a prune of a store holding `nodes` (ids in list order) to `roots` must give, by the
    mirror: the kept digests in new-id order, the counts, the compacted blob and offsets, the table
    size and the statuses"""

    def __init__(self, nodes, roots):
        nodes = [bytes(n) for n in nodes]
        digs = [sha3(n) for n in nodes]
        db = dict(zip(digs, nodes))
        kept, self.n_missing, self.root_status, self.deepest = reachable_host(db, roots)
        seen, self.digests, self.nodes = set(), [], []
        for d, n in zip(digs, nodes):               # ascending old id; the lowest id of equal digests
            if d in kept and d not in seen:
                seen.add(d)
                self.digests.append(d)
                self.nodes.append(n)
        assert seen == kept
        self.kept = kept
        self.n_kept = len(self.nodes)
        self.bytes_kept = sum(len(n) for n in self.nodes)
        self.blob = b''.join(self.nodes)
        self.off = np.zeros(self.n_kept + 1, np.uint64)
        if self.nodes:
            self.off[1:] = np.cumsum([len(n) for n in self.nodes])
        self.n_slots = 64
        while self.n_slots < 2 * self.n_kept:
            self.n_slots *= 2

    def info(self):
        return {'n_nodes': self.n_kept, 'n_unique': self.n_kept, 'n_bytes': self.bytes_kept, 'n_slots': self.n_slots}

    def counts(self):
        return {'n_kept': self.n_kept, 'bytes_kept': self.bytes_kept, 'n_missing': self.n_missing,
                'root_status': self.root_status}


# ------------------------------------------------------------------ hand-encoded stores
def ext_chain(n, tag):
    """n hashed nodes, each the only child of the next: a leaf under n - 1 one-nibble extensions ->
    (nodes leaf first, the top node's digest).  n kept nodes take n levels."""
    nodes = [rlp_encode([b'\x20', b'value of chain ' + tag + b'.' * 24])]
    for _ in range(n - 1):
        nodes.append(rlp_encode([b'\x11', sha3(nodes[-1])]))
    assert all(len(x) >= 32 for x in nodes)
    return nodes, sha3(nodes[-1])


def value_trap():
    """a branch and a hashed leaf whose VALUES are the 32-byte digests of two other stored nodes ->
    (nodes, root, the digests that must be dropped)"""
    x1 = rlp_encode([b'\x20\x01', b'a stored node only a leaf value names'])
    x2 = rlp_encode([b'\x20\x02', b'a stored node only a branch value names'])
    leaf = rlp_encode([b'\x31\x23', sha3(x1)])
    branch = rlp_encode([b''] * 3 + [sha3(leaf)] + [b''] * 12 + [sha3(x2)])
    assert len(leaf) >= 32
    return [x1, x2, leaf, branch], sha3(branch), {sha3(x1), sha3(x2)}


def _list(body):
    from plenum_gpu.state_proofs import _length_prefix
    return _length_prefix(len(body), 192) + body


def malformed_parent():
    """a branch whose slot 0 holds an inline child that does not parse at its own level (a list of
    three items, the first the digest of a stored node) and whose slot 1 refers to a stored leaf ->
    (nodes, root, the digest that must be dropped, the digest that must be kept)"""
    hidden = rlp_encode([b'\x20\x07', b'named from inside a malformed inline node'])
    leaf = rlp_encode([b'\x20\x08', b'a leaf beside the malformed inline child'])
    inline = _list(b'\xa0' + sha3(hidden) + b'\x01\x02')
    parent = _list(inline + b'\xa0' + sha3(leaf) + b'\x80' * 15)
    return [hidden, leaf, parent], sha3(parent), sha3(hidden), sha3(leaf)


def nested(levels):
    """one stored node with `levels` inline extensions nested under it, the innermost over the digest
    of a stored leaf -> (nodes, root, the leaf's digest)"""
    leaf = rlp_encode([b'\x20\x09', b'the leaf under the nested inline extensions'])
    node = [b'\x11', sha3(leaf)]
    for _ in range(levels):
        node = [b'\x11', node]
    top = rlp_encode(node)
    return [leaf, top], sha3(top), sha3(leaf)


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstateprunecheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstateprunecheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.pr_store_new.restype = vp
        so.pr_store_new.argtypes = [u64]
        so.pr_store_free.restype = None
        so.pr_store_free.argtypes = [vp]
        so.pr_store_add.restype = u64
        so.pr_store_add.argtypes = [vp, vp, vp, u64]
        so.pr_store_info.restype = None
        so.pr_store_info.argtypes = [vp, vp, vp, vp, vp]
        so.pr_store_dump.restype = None
        so.pr_store_dump.argtypes = [vp] * 6
        so.pr_store_tail_zero.restype = ctypes.c_int
        so.pr_store_tail_zero.argtypes = [vp]
        so.pr_prune.restype = ctypes.c_int
        so.pr_prune.argtypes = [vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, vp, u64, vp]
        _lib = so
    return _lib


class HostStore:
    """the store of statestore_host.h with the prune of stateprune_host.h on it"""

    def __init__(self, nodes=()):
        self._so = host_lib()
        self._h = self._so.pr_store_new(1)
        self.add_nodes(nodes)

    def close(self):
        if self._h:
            self._so.pr_store_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add_nodes(self, nodes):
        nodes = [bytes(n) for n in nodes]
        if not nodes:
            return 0
        blob, off = sb.pack(nodes)
        return self._so.pr_store_add(self._h, sp.ptr(blob), sp.ptr(off), len(nodes))

    def info(self):
        v = [ctypes.c_uint64(0) for _ in range(4)]
        self._so.pr_store_info(self._h, *[ctypes.byref(x) for x in v])
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes', 'n_slots'), (x.value for x in v)))

    def dump(self):
        """-> (blob bytes, off (n + 1): every node starts where the one before ends, [digests], dup flags)"""
        i = self.info()
        n = i['n_nodes']
        blob = np.zeros(max(i['n_bytes'], 1), np.uint8)
        beg, end = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        dig, dup = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        self._so.pr_store_dump(self._h, sp.ptr(blob), sp.ptr(beg), sp.ptr(end), sp.ptr(dig), sp.ptr(dup))
        return blob[:i['n_bytes']].tobytes(), beg[:n], end[:n], [dig[j].tobytes() for j in range(n)], dup[:n]

    def tail_zero(self):
        return bool(self._so.pr_store_tail_zero(self._h))

    def prune(self, roots, apply=True, want_digests=True, digest_cap=None):
        """-> {'rc', 'root_status', 'n_kept', 'bytes_kept', 'n_missing', 'digests', 'bad_root'}"""
        roots = [bytes(r) for r in roots]
        rts = np.frombuffer(b''.join(roots) + b'\0', np.uint8).copy()
        status = np.full(max(len(roots), 1), 0xee, np.uint8)
        kept, nbytes, missing, bad = (ctypes.c_uint64(0) for _ in range(4))
        cap = digest_cap
        if want_digests and cap is None:
            self._so.pr_prune(self._h, sp.ptr(rts), len(roots), 0, None, ctypes.byref(kept), None, None, None, 0, None)
            cap = kept.value
        dig = np.zeros((max(cap or 0, 1), 32), np.uint8) if want_digests else None
        rc = self._so.pr_prune(self._h, sp.ptr(rts), len(roots), 1 if apply else 0, sp.ptr(status), ctypes.byref(kept),
                               ctypes.byref(nbytes), ctypes.byref(missing), sp.ptr(dig) if want_digests else None,
                               cap or 0, ctypes.byref(bad))
        out = {'rc': rc, 'root_status': [int(x) for x in status[:len(roots)]], 'n_kept': kept.value,
               'bytes_kept': nbytes.value, 'n_missing': missing.value, 'bad_root': bad.value, 'digests': None}
        if want_digests and rc == PR_OK:
            out['digests'] = [dig[j].tobytes() for j in range(kept.value)]
        return out


def host_pruned(nodes, roots):
    """a fresh host store of `nodes` pruned to `roots` -> (the prune's dict, info(), dump(), tail_zero())"""
    with HostStore(nodes) as st:
        r = st.prune(roots)
        return r, st.info(), st.dump(), st.tail_zero()


def check_host_equals_want(nodes, roots):
    """the host twin's prune against the mirror's, byte for byte -> the Want"""
    want = Want(nodes, roots)
    with HostStore(nodes) as st:
        before = st.info()
        rep = st.prune(roots, apply=False)
        assert rep['rc'] == PR_OK and st.info() == before
        assert {k: rep[k] for k in want.counts()} == want.counts() and rep['digests'] == want.digests
        got = st.prune(roots)
        assert got == rep
        blob, beg, end, digs, dup = st.dump()
        assert st.info() == want.info() and st.tail_zero()
        assert blob == want.blob and digs == want.digests and not dup.any()
        assert (beg == want.off[:-1]).all() and (end == want.off[1:]).all()
        again = st.prune(roots)
        assert again == got and st.info() == want.info() and st.dump()[0] == want.blob
    return want


# ------------------------------------------------------------------ the case file
def write_cases(path, cases):
    """cases: [(store nodes, kept roots, Want or None for a nesting refusal)] in the layout of
    tools/hostcheck/stateprunecheck_main.cpp"""
    with open(path, 'wb') as fh:
        fh.write(b'SPC1' + struct.pack('<I', len(cases)))
        for nodes, roots, want in cases:
            fh.write(struct.pack('<Q', len(nodes)) + su._ragged([bytes(n) for n in nodes]))
            fh.write(struct.pack('<Q', len(roots)) + b''.join(bytes(r) for r in roots))
            if want is None:
                fh.write(struct.pack('<I', PR_NESTING) + bytes(len(roots)))
                continue
            fh.write(struct.pack('<I', PR_OK) + bytes(want.root_status))
            fh.write(struct.pack('<QQQ', want.n_kept, want.bytes_kept, want.n_missing) + b''.join(want.digests))
            fh.write(want.off.tobytes() + want.blob + struct.pack('<Q', want.n_slots))
