"""State-store test helpers: the fixture's tries as node sets, a bottom-up trie
builder, the host build of csrc/pv_trie_store.h (tools/hostcheck/statestorecheck.cpp),
the Python mirror run over the same queries, and the case file of
statestorecheck_asan."""
import ctypes
import hashlib
import os
import random
import struct
import subprocess

import numpy as np

import _state_proofs as sp
from conftest import REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
OK, VALUE_MISMATCH, NODE_MISSING, MALFORMED, PATH_TOO_LONG = range(5)   # PV_SP_* of plenum_verify.h
_lib = None
_tries = None


def sha3(b):
    return hashlib.sha3_256(b).digest()


# ------------------------------------------------------------------ fixture
def tries():
    """{trie name: (root hash, {hash: node RLP})} from the nodes of the fixture's `own` rows"""
    global _tries
    if _tries is None:
        out = {}
        for r in sp.fixture():
            if r.kind == 'own':
                root, db = out.setdefault(r.trie, (r.root, {}))
                assert root == r.root
                for n in r.nodes:
                    db[sha3(n)] = n
        _tries = out
    return _tries


def proof_rows():
    """the `own` and `absent/*` rows: one (root, key) -> (proof nodes, value or None) each"""
    return [r for r in sp.fixture() if not r.multi and (r.kind == 'own' or r.kind.startswith('absent/'))]


def extra_nodes():
    """nodes of the `extra_nodes` rows that belong to no trie's own proofs"""
    known = {h for _, db in tries().values() for h in db}
    out = {}
    for r in sp.fixture():
        if r.kind == 'extra_nodes':
            for n in r.nodes:
                if sha3(n) not in known:
                    out[sha3(n)] = n
    return list(out.values())


def flipped_roots():
    """[(trie, key, flipped node)] of the `flipped` rows whose flipped node is the path's root node"""
    out = []
    for r in sp.fixture():
        if r.kind == 'flipped' and not r.multi and not any(sha3(n) == r.root for n in r.nodes):
            db = tries()[r.trie][1]
            bad = [n for n in r.nodes if sha3(n) not in db]
            assert len(bad) == 1
            out.append((r.trie, r.kvs[0][0], bad[0]))
    return out


# ------------------------------------------------------------------ a trie builder
def build_trie(keys_values):
    """A trie over (key, encoded value) pairs built bottom-up -> (root hash, {hash: node RLP});
    restated from tools/bench_state_proofs.py::build_trie (that module imports torch)."""
    from plenum_gpu.state_proofs import rlp_encode
    db = {}

    def hp(nibbles, leaf):
        flags = (2 if leaf else 0) + (len(nibbles) & 1)
        nib = ([flags] if len(nibbles) & 1 else [flags, 0]) + list(nibbles)
        return bytes(16 * nib[i] + nib[i + 1] for i in range(0, len(nib), 2))

    def ref(node):
        enc = rlp_encode(node)
        if len(enc) < 32:
            return node
        h = sha3(enc)
        db[h] = enc
        return h

    def make(items, depth):
        if not items:
            return b''
        if len(items) == 1:
            k, v = items[0]
            return ref([hp(k[depth:], True), v])
        first = items[0][0]
        common = 0
        while all(len(k) > depth + common and k[depth + common] == first[depth + common] for k, _ in items):
            common += 1
        if common:
            return ref([hp(first[depth:depth + common], False), make(items, depth + common)])
        slots, value = [[] for _ in range(16)], b''
        for k, v in items:
            if len(k) == depth:
                value = v
            else:
                slots[k[depth]].append((k, v))
        return ref([make(s, depth + 1) for s in slots] + [value])

    items = sorted(([n for b in k for n in (b >> 4, b & 15)], v) for k, v in keys_values)
    top = make(items, 0)
    if not isinstance(top, bytes) or len(top) != 32:
        enc = rlp_encode(top)
        top = sha3(enc)
        db[top] = enc
    return top, db


def leaf_trie(node_len, key=b'k'):
    """a single-leaf trie whose root node RLP is exactly node_len bytes -> (root, db, value)"""
    from plenum_gpu.state_proofs import rlp_encode
    for vlen in range(max(node_len - 24, 1), node_len):
        value = rlp_encode([b'\x5a' * vlen])
        root, db = build_trie([(key, value)])
        if len(db[root]) == node_len:
            return root, db, value
        if len(db[root]) > node_len:
            break
    raise AssertionError('no value length gives a {}-byte leaf'.format(node_len))


# ------------------------------------------------------------------ results
class Result:
    """per query: status, node_count, node_ids (n x max_nodes), proof_off, val_rel, val_len, blob"""

    def __init__(self, n, max_nodes):
        self.max_nodes = max_nodes
        self.status, self.node_count = np.full(n, 0xee, np.uint8), np.zeros(n, np.uint32)
        self.node_ids = np.zeros((n, max_nodes), np.uint32)
        self.proof_off = np.zeros(n + 1, np.uint64)
        self.val_rel, self.val_len = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.blob = np.zeros(0, np.uint8)

    def proof(self, q):
        return self.blob[int(self.proof_off[q]):int(self.proof_off[q + 1])].tobytes()

    def value(self, q):
        o = int(self.proof_off[q] + self.val_rel[q])
        return self.blob[o:o + int(self.val_len[q])].tobytes()

    def ids(self, q):
        return self.node_ids[q, :min(int(self.node_count[q]), self.max_nodes)].tolist()

    def same(self, other, ids=True):
        """None, or what differs first"""
        for f in ('status', 'node_count', 'proof_off', 'val_rel', 'val_len', 'blob'):
            a, b = getattr(self, f), getattr(other, f)
            if a.shape != b.shape or not (a == b).all():
                return f
        if ids:
            for q in range(len(self.status)):
                if self.ids(q) != other.ids(q):
                    return 'node_ids[{}]'.format(q)
        return None


def default_max_nodes(keys):
    return 2 * max([len(k) for k in keys] + [0]) + 1


def mirror_prove(db, id_of, roots, root_idx, keys, max_nodes=None):
    """walk_host over every query, as a Result; id_of = {digest: node id} (lowest id of a digest)"""
    from plenum_gpu.state_store import walk_host
    max_nodes = max_nodes or default_max_nodes(keys)
    res = Result(len(keys), max_nodes)
    chunks, pos = [], 0
    for q, key in enumerate(keys):
        root = roots[root_idx[q] if root_idx is not None else q]
        st, nodes, value, proof, val_rel = walk_host(db, root, key, max_nodes)
        res.status[q], res.node_count[q] = st, len(nodes)
        for i, n in enumerate(nodes[:max_nodes]):
            res.node_ids[q, i] = id_of[sha3(n)]
        if proof is not None:
            chunks.append(proof)
            pos += len(proof)
            res.val_len[q], res.val_rel[q] = len(value), val_rel
            assert proof[val_rel:val_rel + len(value)] == value
        res.proof_off[q + 1] = pos
    res.blob = np.frombuffer(b''.join(chunks), np.uint8).copy()
    return res


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstatestorecheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstatestorecheck.so'))
        u64, u32, vp = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
        so.ss_create.restype, so.ss_create.argtypes = vp, [u64]
        so.ss_free.restype, so.ss_free.argtypes = None, [vp]
        so.ss_add.restype, so.ss_add.argtypes = u64, [vp, vp, vp, u64]
        so.ss_add_digests.restype, so.ss_add_digests.argtypes = u64, [vp, vp, u64]
        so.ss_info.restype, so.ss_info.argtypes = None, [vp] + [ctypes.POINTER(u64)] * 4
        so.ss_find.restype, so.ss_find.argtypes = ctypes.c_int64, [vp, vp]
        so.ss_slot_of.restype, so.ss_slot_of.argtypes = ctypes.c_int64, [vp, u32]
        so.ss_is_dup.restype, so.ss_is_dup.argtypes = ctypes.c_int, [vp, u32]
        so.ss_digest.restype, so.ss_digest.argtypes = None, [vp, u32, vp]
        so.ss_prove.restype = ctypes.c_int
        so.ss_prove.argtypes = [vp, vp, vp, u64, vp, vp, u64, u32] + [vp] * 7 + [u64]
        _lib = so
    return _lib


def pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b''.join(msgs) + b'\0' * 4, np.uint8).copy(), off


class HostStore:
    """the store of tools/hostcheck/statestore_host.h; also keeps {digest: lowest id} and
    {digest: node} of what was added, for the mirror"""

    def __init__(self, node_hint=1):
        self.so = host_lib()
        self.h = ctypes.c_void_p(self.so.ss_create(node_hint))
        self.id_of, self.db, self.count = {}, {}, 0

    def __del__(self):
        if self.h:
            self.so.ss_free(self.h)
            self.h = None

    def add(self, nodes):
        nodes = list(nodes)
        for n in nodes:
            self.id_of.setdefault(sha3(n), self.count)
            self.db[sha3(n)] = n
            self.count += 1
        blob, off = pack(nodes)
        return self.so.ss_add(self.h, sp.ptr(blob), sp.ptr(off), len(nodes))

    def add_digests(self, digests):
        for d in digests:
            self.id_of.setdefault(bytes(d), self.count)
            self.count += 1
        buf = np.frombuffer(b''.join(bytes(d) for d in digests) + b'\0', np.uint8).copy()
        return self.so.ss_add_digests(self.h, sp.ptr(buf), len(digests))

    def info(self):
        v = [ctypes.c_uint64(0) for _ in range(4)]
        self.so.ss_info(self.h, *[ctypes.byref(x) for x in v])
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes', 'n_slots'), (x.value for x in v)))

    def find(self, digest):
        return self.so.ss_find(self.h, sp.ptr(np.frombuffer(bytes(digest), np.uint8).copy()))

    def slot_of(self, node_id):
        return self.so.ss_slot_of(self.h, node_id)

    def is_dup(self, node_id):
        return bool(self.so.ss_is_dup(self.h, node_id))

    def prove(self, roots, root_idx, keys, max_nodes=None, proof_cap=None, sizing=False):
        """-> Result (with .rc, the return code)"""
        n = len(keys)
        max_nodes = max_nodes or default_max_nodes(keys)
        res = Result(n, max_nodes)
        rts = np.frombuffer(b''.join(roots) + b'\0', np.uint8).copy()
        ridx = None if root_idx is None else np.asarray(root_idx, np.uint32)
        kblob, koff = pack(keys)
        args = [self.h, sp.ptr(rts), sp.ptr(ridx), len(roots), sp.ptr(kblob), sp.ptr(koff), n, max_nodes,
                sp.ptr(res.status), sp.ptr(res.node_count), sp.ptr(res.node_ids), sp.ptr(res.proof_off),
                sp.ptr(res.val_rel), sp.ptr(res.val_len)]
        res.rc = self.so.ss_prove(*args, None, 0)
        if sizing:
            return res
        total = int(res.proof_off[n])
        blob = np.zeros(max(total, 1), np.uint8)
        res.rc = self.so.ss_prove(*args, sp.ptr(blob), total if proof_cap is None else proof_cap)
        res.blob = blob[:total] if res.rc == 0 else np.zeros(0, np.uint8)
        return res


# ------------------------------------------------------------------ the case file
def write_cases(path, cases):
    """cases: [(batches, roots, root_idx or None, keys, max_nodes, expected Result, n_nodes,
    n_unique)] in the layout of tools/hostcheck/statestorecheck_main.cpp; a batch is a list of
    node RLPs or ('digests', [32-byte digests])"""
    with open(path, 'wb') as fh:
        fh.write(b'SSC1' + struct.pack('<I', len(cases)))
        for batches, roots, root_idx, keys, max_nodes, want, n_nodes, n_unique in cases:
            fh.write(struct.pack('<Q', len(batches)))
            for nodes in batches:
                if isinstance(nodes, tuple):
                    fh.write(struct.pack('<BQ', 1, len(nodes[1])) + b''.join(nodes[1]))
                    continue
                off = np.zeros(len(nodes) + 1, np.uint64)
                off[1:] = np.cumsum([len(x) for x in nodes])
                fh.write(struct.pack('<BQ', 0, len(nodes)) + off.tobytes() + b''.join(nodes))
            fh.write(struct.pack('<Q', len(roots)) + b''.join(roots))
            fh.write(struct.pack('<QB', len(keys), root_idx is not None))
            if root_idx is not None:
                fh.write(np.asarray(root_idx, np.uint32).tobytes())
            koff = np.zeros(len(keys) + 1, np.uint64)
            koff[1:] = np.cumsum([len(k) for k in keys])
            fh.write(koff.tobytes() + b''.join(keys))
            fh.write(struct.pack('<IQQ', max_nodes, n_nodes, n_unique))
            fh.write(want.status.tobytes() + want.node_count.tobytes() + want.proof_off.tobytes() +
                     want.val_rel.tobytes() + want.val_len.tobytes() + want.blob.tobytes())


# ------------------------------------------------------------------ scenarios
def sc_fixture():
    """all five tries in one store, every `own` / `absent/*` row, mixed roots"""
    tr = tries()
    names = sorted(tr)
    rows = proof_rows()
    batches = [list(tr[n][1].values()) for n in names]
    return batches, [tr[n][0] for n in names], [names.index(r.trie) for r in rows], [r.kvs[0][0] for r in rows], None


def _kv(rng, n, tag=b''):
    from plenum_gpu.state_proofs import rlp_encode
    out = {}
    for i in range(n):
        key = sha3(tag + b'did:%d' % i) if i % 3 else tag + b'attr:%d' % i
        out[key] = rlp_encode([bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120)))])
    return out


def absent_keys(rng, keys, n):
    """keys that are not in the trie, of each kind: a random key (a blank slot or a leaf
    mismatch), a present key cut short, a present key made longer, a last-nibble change"""
    out, have = [], set(keys)
    while len(out) < n:
        k = keys[rng.randrange(len(keys))]
        kind = len(out) % 4
        c = (sha3(k + b'?'), k[:-1], k + b'\x01', k[:-1] + bytes([k[-1] ^ 1]))[kind]
        if c not in have:
            out.append(c)
    return out


def sc_built():
    rng = random.Random(14)
    kv = _kv(rng, 200)
    root, db = build_trie(kv.items())
    keys = list(kv) + absent_keys(rng, list(kv), 80) + [b'']
    return [list(db.values())], [root], [0] * len(keys), keys, None


def sc_boundaries():
    """single-leaf tries whose root node is 55, 56, 255, 256, 65,535 and 65,536 bytes"""
    batches, roots, keys = [], [], []
    for n in (55, 56, 255, 256, 65535, 65536):
        root, db, _ = leaf_trie(n)
        batches.append(list(db.values()))
        roots.append(root)
        keys.append(b'k')
    return batches, roots, None, keys, None


def history():
    """T0 of 300 keys, T1 = T0 with 40 keys changed, added or removed -> (kv0, kv1, (root, db) x 2)"""
    rng = random.Random(15)
    kv0 = _kv(rng, 300)
    kv1 = dict(kv0)
    ks = list(kv0)
    for i, k in enumerate(ks[:14]):
        kv1[k] = kv0[ks[299 - i]]          # changed: another key's value
    for k in ks[14:27]:
        del kv1[k]
    kv1.update(_kv(rng, 13, b'added'))
    return kv0, kv1, build_trie(kv0.items()), build_trie(kv1.items())


def sc_history():
    kv0, kv1, (r0, db0), (r1, db1) = history()
    keys = sorted(set(kv0) | set(kv1))
    return [list(db0.values()), list(db1.values())], [r0, r1], [0] * len(keys) + [1] * len(keys), keys + keys, None


def sc_hostile():
    """each `flipped` row whose flipped node is the root node: the walk starts in the flipped bytes"""
    tr = tries()
    batches, roots, keys = [], [], []
    for trie, key, bad in flipped_roots():
        batches.append(list(tr[trie][1].values()) + [bad])
        roots.append(sha3(bad))
        keys.append(key)
    # ... and every truncation of a branch and of a leaf, as their own roots
    name = max(tr, key=lambda n: len(tr[n][1]))
    nodes = sorted(tr[name][1].values(), key=len)
    for node in (nodes[0], nodes[-1]):
        for cut in range(1, len(node), 7):
            batches.append([node[:cut]])
            roots.append(sha3(node[:cut]))
            keys.append(proof_rows()[0].kvs[0][0])
    return batches, roots, None, keys, None


def deep_rows():
    return [r for r in proof_rows() if len(r.nodes) == 9]


def sc_too_long():
    tr = tries()
    rows = deep_rows()
    return [list(tr[rows[0].trie][1].values())], [rows[0].root], [0] * len(rows), [r.kvs[0][0] for r in rows], 2


def sc_missing():
    """a depth >= 6 key over stores lacking each path node in turn, an unknown root, the blank root"""
    from plenum_gpu.state_proofs import BLANK_ROOT
    from plenum_gpu.state_store import walk_host
    tr = tries()
    r = deep_rows()[0]
    root, db = tr[r.trie]
    path = walk_host(db, root, r.kvs[0][0])[1]
    out = []
    for i in range(len(path)):
        nodes = [n for n in db.values() if n != path[i]]
        out.append(([nodes], [root], None, [r.kvs[0][0]], None))
    out.append(([list(db.values())], [b'\x11' * 32, BLANK_ROOT], None, [r.kvs[0][0], b'any'], None))
    return out


SCENARIOS = {'fixture': sc_fixture, 'built': sc_built, 'boundaries': sc_boundaries, 'history': sc_history,
             'hostile': sc_hostile, 'too_long': sc_too_long}
