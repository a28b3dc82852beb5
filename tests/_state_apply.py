"""State-apply test helpers (sets and removals onto a committed root): the fixture recorded from
the reference (tests/golden/state_remove.json, tools/gen_state_remove_golden.py), the host build
of csrc/pv_trie_update.h in its removal mode (tools/hostcheck/stateapplycheck.cpp), the shared
case lists and the case file of stateapplycheck_asan.  A pair's encoded value of b'' removes
its key."""
import ctypes
import json
import os
import random
import struct
import subprocess

import numpy as np

import _state_build as sb
import _state_proofs as sp
import _state_update as su
from conftest import REPO

HC_DIR = sb.HC_DIR
OK, BAD_ORDER, BAD_VALUE, BAD_OFFSET, TOO_SMALL, BAD_WALK = range(6)   # stateupdate_host.h
_lib = None
_fixture = None
_cache = {}


class Batch:
    def __init__(self, d, reach):
        self.items = [(bytes.fromhex(k), None if v is None else bytes.fromhex(v)) for k, v in zip(d['keys'], d['values'])]
        self.root = bytes.fromhex(d['root'])
        self.reachable = reach          # the digests reachable from self.root in the reference
        self.added = set(bytes.fromhex(x) for x in d['added'])


class Case:
    def __init__(self, d):
        self.name = d['name']
        if 'base_from' in d:
            self.base = next(c for c in sb.fixture() if c.name == d['base_from']).items
        else:
            self.base = [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in zip(d['base_keys'], d['base_values'])]
        self.base_root = bytes.fromhex(d['base_root'])
        reach = set(bytes.fromhex(x) for x in d['base_digests'])
        self.base_reachable = reach
        self.batches = []
        for b in d['batches']:
            reach = (reach | set(bytes.fromhex(x) for x in b['added'])) - set(bytes.fromhex(x) for x in b['removed'])
            self.batches.append(Batch(b, reach))


def fixture():
    global _fixture
    if _fixture is None:
        with open(os.path.join(REPO, 'tests', 'golden', 'state_remove.json')) as fh:
            _fixture = [Case(c) for c in json.load(fh)['cases']]
    return _fixture


def case(name):
    return next(c for c in fixture() if c.name == name)


def ops(items):
    """(key, raw value or None) items -> sorted distinct (key, encoded value or b''): what the device form takes"""
    from plenum_gpu.state_store import _ops
    return _ops(items)


def fixture_shapes():
    """[(name, base pairs, [batch pairs])] of the fixture, as encoded pairs"""
    return [('fx/' + c.name, sb.pairs(c.base), [ops(b.items) for b in c.batches]) for c in fixture()]


def batch_onto(base, n, seed, removals=0.5):
    """n operations onto `base` pairs: the given share removals (four fifths of them of keys of the
    base, the rest of absent keys), the others sets, half overwriting a key of the base, half new"""
    rng = random.Random(seed)
    n_rm = int(n * removals)
    n_present = n_rm - n_rm // 5
    n_over = (n - n_rm) // 2
    picked = rng.sample(base, n_present + n_over)
    out = {k: b'' for k, _ in picked[:n_present]}
    for k, _ in picked[n_present:]:
        out[k] = sb._encode(bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120))))
    i = 0
    while len(out) < n_present + n_over + n_rm // 5:
        out[sb.sha3(b'gone:%d:%d' % (seed, i)) if i % 3 else b'attr:gone:%d:%d' % (seed, i)] = b''
        i += 1
    while len(out) < n:
        k = sb.sha3(b'new:%d:%d' % (seed, i)) if i % 3 else b'attr:new:%d:%d' % (seed, i)
        out[k] = sb._encode(bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120))))
        i += 1
    return sorted(out.items())


def shapes():
    """[(name, base pairs, [batch pairs])] beyond the fixture: the wave edge with half removals, the
    deepest chain fusing from the bottom and 4,096 mixed operations"""
    if 'shapes' not in _cache:
        out = []
        base = sb.mixed_pairs(300, 31)
        for n in (63, 64, 65):
            out.append(('wave%d' % n, base, [batch_onto(base, n, 200 + n)]))
        chain = sb.chain_pairs()
        # the all-sevens key (the deepest leaf) sorts last, before it the leaves that leave the chain
        # at nibble 62, 61, ...: the first batch removes the deepest leaf, the second the next eleven
        deepest_first = [k for k, _ in reversed(chain)]
        assert deepest_first[0] == bytes([0x77] * 32)
        out.append(('chain', chain, [[(deepest_first[0], b'')], [(k, b'') for k in sorted(deepest_first[1:12])]]))
        base = sb.mixed_pairs(4096, 13)
        out.append(('mixed4096', base, [batch_onto(base, 4096, 4096)]))
        _cache['shapes'] = out
    return _cache['shapes']


def all_shapes():
    return fixture_shapes() + shapes()


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstateapplycheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstateapplycheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.sa_store_new.restype = vp
        so.sa_store_new.argtypes = [u64]
        so.sa_store_free.restype = None
        so.sa_store_free.argtypes = [vp]
        so.sa_store_add.restype = u64
        so.sa_store_add.argtypes = [vp, vp, vp, u64]
        so.sa_store_info.restype = None
        so.sa_store_info.argtypes = [vp, vp, vp, vp]
        so.sa_apply.restype = ctypes.c_int
        so.sa_apply.argtypes = [vp, vp, vp, vp, vp, vp, u64, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, u64, vp, u64, vp,
                                vp, vp, vp]
        _lib = so
    return _lib


class HostStore:
    """the store of statestore_host.h with sa_apply on it"""

    def __init__(self, node_hint=1):
        self._so = host_lib()
        self._h = self._so.sa_store_new(node_hint)

    def close(self):
        if self._h:
            self._so.sa_store_free(self._h)
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
        return self._so.sa_store_add(self._h, sp.ptr(blob), sp.ptr(off), len(nodes))

    def info(self):
        v = [ctypes.c_uint64(0) for _ in range(3)]
        self._so.sa_store_info(self._h, *[ctypes.byref(x) for x in v])
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes'), (x.value for x in v)))

    def apply(self, root, prs, insert=True, blob_cap=None, node_cap=None, removals=True):
        """sa_apply of (key, encoded value or b'') pairs as given (no sorting) -> sb.Built with
        bad_index, status (the PV_SP_* status of a refused walk) and n_items (the merged list's
        length); removals=False: the update without the removal mode, on the same store"""
        so = self._so
        kb, ko = sb.pack([k for k, _ in prs])
        vb, vo = sb.pack([v for _, v in prs])
        old = np.frombuffer(bytes(root), np.uint8).copy()
        b = sb.Built()
        new = np.zeros(32, np.uint8)
        nn, nb, bad, items = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        status = ctypes.c_uint32(0)
        tail = [ctypes.byref(bad), ctypes.byref(status), ctypes.byref(items)]
        head = [self._h, sp.ptr(old), sp.ptr(kb), sp.ptr(ko), sp.ptr(vb), sp.ptr(vo), len(prs)]
        sizes = [sp.ptr(new), ctypes.byref(nn), ctypes.byref(nb)]
        rm = 1 if removals else 0
        b.rc = so.sa_apply(*head, 0, rm, *sizes, None, 0, None, 0, None, *tail)
        b.bad_index, b.status, b.n_items, b.max_level = bad.value, status.value, items.value, 0
        b.n_nodes, b.n_bytes = nn.value, nb.value
        b.blob, b.off, b.dig = np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros((0, 32), np.uint8)
        b.root = new.tobytes()
        if b.rc != OK:
            return b
        bc = b.n_bytes if blob_cap is None else blob_cap
        nc = b.n_nodes if node_cap is None else node_cap
        blob, off, dig = np.full(max(bc, 1), 0x5a, np.uint8), np.zeros(nc + 1, np.uint64), np.zeros((max(nc, 1), 32), np.uint8)
        b.rc = so.sa_apply(*head, 1 if insert else 0, rm, *sizes, sp.ptr(blob), bc, sp.ptr(off), nc, sp.ptr(dig), *tail)
        b.root = new.tobytes()
        if b.rc == OK:
            b.blob, b.off, b.dig = blob[:b.n_bytes], off, dig[:b.n_nodes]
        else:
            b.untouched = bool((blob == 0x5a).all() and not off.any() and not dig.any())
        return b


def host_run(name, base, batches):
    """the host twin over one shape, cached: the base built into a fresh host store, each batch
    applied with insert -> (base Built, [Built per batch], [the store's nodes before each batch])"""
    if name not in _cache:
        with HostStore() as st:
            b0 = sb.host_build(base)
            st.add_nodes(b0.nodes())
            root, outs, stores, nodes = b0.root, [], [], list(b0.nodes())
            for prs in batches:
                stores.append(list(nodes))
                b = st.apply(root, prs)
                assert b.rc == OK, (name, b.rc, b.bad_index, b.status)
                outs.append(b)
                nodes += b.nodes()
                root = b.root
            _cache[name] = (b0, outs, stores)
    return _cache[name]


def state_after(state, prs):
    """the {key: encoded value} state with the (key, encoded value or b'') pairs applied"""
    for k, v in prs:
        if v:
            state[k] = v
        else:
            state.pop(k, None)
    return state


def sibling_case():
    """a state, a key to remove, the nodes of that key's proof and the index of the key in the batch:
    the removed key's sibling under the last branch of its path is a hashed node outside the proof"""
    from plenum_gpu.state_store import apply_encoded_host as _apply_encoded_host, walk_host as _walk_host
    prs = sb.mixed_pairs(200, 43)
    b0 = sb.host_build(prs)
    db = b0.db()
    for j, (k, _) in enumerate(prs):
        proof = _walk_host(db, b0.root, k)[1]
        others = [h for h, n in db.items() if n not in proof]
        part = {sb.sha3(n): n for n in proof}
        try:
            _apply_encoded_host(part, b0.root, [(k, b'')])
        except KeyError:
            assert others
            return prs, b0, k, proof
    raise AssertionError('no key with a hashed sibling')


# ------------------------------------------------------------------ the case file
def write_cases(path, cases):
    """cases: [(store nodes, old root, pairs, expected Built)] in the layout of
    tools/hostcheck/stateapplycheck_main.cpp"""
    with open(path, 'wb') as fh:
        fh.write(b'SAC1' + struct.pack('<I', len(cases)))
        for nodes, root, prs, want in cases:
            fh.write(struct.pack('<Q', len(nodes)) + su._ragged(nodes) + bytes(root))
            fh.write(struct.pack('<Q', len(prs)) + su._ragged([k for k, _ in prs]) + su._ragged([v for _, v in prs]))
            fh.write(struct.pack('<IQI', want.rc, want.bad_index, want.status))
            if want.rc == OK:
                fh.write(want.root + struct.pack('<QQ', want.n_nodes, want.n_bytes) + want.off.tobytes() +
                         want.blob.tobytes() + want.dig.tobytes())
