"""State-update test helpers: the fixture recorded from the reference
(tests/golden/state_update.json, tools/gen_state_update_golden.py), the host build of
csrc/pv_trie_update.h (tools/hostcheck/stateupdatecheck.cpp), the shared case lists and the
case file of stateupdatecheck_asan."""
import ctypes
import json
import os
import random
import struct
import subprocess

import numpy as np

import _state_build as sb
import _state_proofs as sp
from conftest import REPO

HC_DIR = sb.HC_DIR
OK, BAD_ORDER, BAD_VALUE, BAD_OFFSET, TOO_SMALL, BAD_WALK = range(6)   # stateupdate_host.h
_lib = None
_fixture = None
_cache = {}


class Batch:
    def __init__(self, d, reach):
        self.items = [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in zip(d['keys'], d['values'])]
        self.root = bytes.fromhex(d['root'])
        self.reachable = reach          # the digests reachable from self.root in the reference


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
        with open(os.path.join(REPO, 'tests', 'golden', 'state_update.json')) as fh:
            _fixture = [Case(c) for c in json.load(fh)['cases']]
    return _fixture


def case(name):
    return next(c for c in fixture() if c.name == name)


def fixture_shapes():
    """[(name, base pairs, [batch pairs])] of the fixture, as encoded pairs"""
    return [('fx/' + c.name, sb.pairs(c.base), [sb.pairs(b.items) for b in c.batches]) for c in fixture()]


def _batch_onto(base, n, seed):
    """n sets onto `base` pairs: half overwrite a key of the base, half are new"""
    rng = random.Random(seed)
    out = {}
    for k, _ in rng.sample(base, n // 2):
        out[k] = sb._encode(bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120))))
    i = 0
    while len(out) < n:
        k = sb.sha3(b'new:%d:%d' % (seed, i)) if i % 3 else b'attr:new:%d:%d' % (seed, i)
        out[k] = sb._encode(bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120))))
        i += 1
    return sorted(out.items())


def chain_batch():
    """64 keys that leave the 63-branch chain of sb.chain_pairs() at every depth 0 .. 63, above it"""
    keys = []
    for i in range(64):
        nib = [7] * 64
        nib[i] = 9
        keys.append(bytes(16 * nib[2 * j] + nib[2 * j + 1] for j in range(32)))
    return sorted((k, sb._encode(b'leaves at %d' % i)) for i, k in enumerate(keys))


def shapes():
    """[(name, base pairs, [batch pairs])] beyond the fixture: the wave edge, the deepest chain,
    4,096 mixed sets and the list-header boundaries of a carried value"""
    if 'shapes' not in _cache:
        out = []
        base = sb.mixed_pairs(300, 31)
        for n in (63, 64, 65):
            out.append(('wave%d' % n, base, [_batch_onto(base, n, 100 + n)]))
        out.append(('chain', sb.chain_pairs(), [chain_batch()]))
        base = sb.mixed_pairs(4096, 13)
        out.append(('mixed4096', base, [_batch_onto(base, 4096, 4096)]))
        for n in (55, 56, 255, 256):
            out.append(('carried%d' % n, [(b'key', (bytes(range(1, 256)) * 2)[:n])],
                        [[(b'kez', b'\x01')], [(b'ke', b'\xc2\x81\x99')]]))
        _cache['shapes'] = out
    return _cache['shapes']


def all_shapes():
    return fixture_shapes() + shapes()


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstateupdatecheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstateupdatecheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.su_store_new.restype = vp
        so.su_store_new.argtypes = [u64]
        so.su_store_free.restype = None
        so.su_store_free.argtypes = [vp]
        so.su_store_add.restype = u64
        so.su_store_add.argtypes = [vp, vp, vp, u64]
        so.su_store_info.restype = None
        so.su_store_info.argtypes = [vp, vp, vp, vp]
        so.su_update.restype = ctypes.c_int
        so.su_update.argtypes = [vp, vp, vp, vp, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp]
        so.su_merge.restype = ctypes.c_int
        so.su_merge.argtypes = [vp, vp, vp, vp, vp, vp, u64] + [vp] * 9
        _lib = so
    return _lib


class HostStore:
    """the store of statestore_host.h with su_update on it"""

    def __init__(self, node_hint=1):
        self._so = host_lib()
        self._h = self._so.su_store_new(node_hint)

    def close(self):
        if self._h:
            self._so.su_store_free(self._h)
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
        return self._so.su_store_add(self._h, sp.ptr(blob), sp.ptr(off), len(nodes))

    def info(self):
        v = [ctypes.c_uint64(0) for _ in range(3)]
        self._so.su_store_info(self._h, *[ctypes.byref(x) for x in v])
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes'), (x.value for x in v)))

    def update(self, root, prs, insert=True, blob_cap=None, node_cap=None):
        """su_update of (key, encoded value) pairs as given (no sorting) -> sb.Built with bad_index,
        status (the PV_SP_* status of a refused walk) and n_items (the merged list's length)"""
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
        b.rc = so.su_update(*head, 0, *sizes, None, 0, None, 0, None, *tail)
        b.bad_index, b.status, b.n_items, b.max_level = bad.value, status.value, items.value, 0
        b.n_nodes, b.n_bytes = nn.value, nb.value
        b.blob, b.off, b.dig = np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros((0, 32), np.uint8)
        b.root = new.tobytes()
        if b.rc != OK:
            return b
        bc = b.n_bytes if blob_cap is None else blob_cap
        nc = b.n_nodes if node_cap is None else node_cap
        blob, off, dig = np.full(max(bc, 1), 0x5a, np.uint8), np.zeros(nc + 1, np.uint64), np.zeros((max(nc, 1), 32), np.uint8)
        b.rc = so.su_update(*head, 1 if insert else 0, *sizes, sp.ptr(blob), bc, sp.ptr(off), nc, sp.ptr(dig), *tail)
        b.root = new.tobytes()
        if b.rc == OK:
            b.blob, b.off, b.dig = blob[:b.n_bytes], off, dig[:b.n_nodes]
        else:
            b.untouched = bool((blob == 0x5a).all() and not off.any() and not dig.any())
        return b

    def merged(self, root, prs):
        """the merged list of a batch -> [(nibbles, kind, payload)]"""
        so = self._so
        kb, ko = sb.pack([k for k, _ in prs])
        vb, vo = sb.pack([v for _, v in prs])
        old = np.frombuffer(bytes(root), np.uint8).copy()
        n, pbytes, vbytes = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        head = [self._h, sp.ptr(old), sp.ptr(kb), sp.ptr(ko), sp.ptr(vb), sp.ptr(vo), len(prs), ctypes.byref(n),
                ctypes.byref(pbytes), ctypes.byref(vbytes)]
        assert so.su_merge(*head, None, None, None, None, None, None) == OK
        ikey, ival = np.zeros(max(pbytes.value, 1), np.uint8), np.zeros(max(vbytes.value, 1), np.uint8)
        ikoff, ivoff = np.zeros(n.value + 1, np.uint64), np.zeros(n.value + 1, np.uint64)
        inib, ikind = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint8)
        assert so.su_merge(*head, sp.ptr(ikey), sp.ptr(ikoff), sp.ptr(inib), sp.ptr(ikind), sp.ptr(ival), sp.ptr(ivoff)) == OK
        out = []
        for i in range(n.value):
            path = ikey[int(ikoff[i]):int(ikoff[i + 1])].tobytes()
            nib = [x for b in path for x in (b >> 4, b & 15)]
            assert len(nib) - int(inib[i]) in (0, 1) and (len(nib) == int(inib[i]) or nib[-1] == 0)
            out.append((nib[:int(inib[i])], int(ikind[i]), ival[int(ivoff[i]):int(ivoff[i + 1])].tobytes()))
        return out


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
                b = st.update(root, prs)
                assert b.rc == OK, (name, b.rc, b.bad_index, b.status)
                outs.append(b)
                nodes += b.nodes()
                root = b.root
            _cache[name] = (b0, outs, stores)
    return _cache[name]


# ------------------------------------------------------------------ the case file
def _ragged(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs])
    return off.tobytes() + b''.join(msgs)


def write_cases(path, cases):
    """cases: [(store nodes, old root, pairs, expected Built)] in the layout of
    tools/hostcheck/stateupdatecheck_main.cpp"""
    with open(path, 'wb') as fh:
        fh.write(b'SUC1' + struct.pack('<I', len(cases)))
        for nodes, root, prs, want in cases:
            fh.write(struct.pack('<Q', len(nodes)) + _ragged(nodes) + bytes(root))
            fh.write(struct.pack('<Q', len(prs)) + _ragged([k for k, _ in prs]) + _ragged([v for _, v in prs]))
            fh.write(struct.pack('<IQI', want.rc, want.bad_index, want.status))
            if want.rc == OK:
                fh.write(want.root + struct.pack('<QQ', want.n_nodes, want.n_bytes) + want.off.tobytes() +
                         want.blob.tobytes() + want.dig.tobytes())
