"""State-build test helpers: the fixture recorded from the reference
(tests/golden/state_build.json, tools/gen_state_build_golden.py), the host build of
csrc/pv_trie_build.h (tools/hostcheck/statebuildcheck.cpp), the shared case lists and the
case file of statebuildcheck_asan."""
import ctypes
import hashlib
import json
import os
import random
import struct
import subprocess

import numpy as np

import _state_proofs as sp
import _state_store as ss
from conftest import REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
OK, BAD_ORDER, BAD_VALUE, BAD_OFFSET, TOO_SMALL = range(5)   # statebuild_host.h
_lib = None
_fixture = None
_cache = {}


def sha3(b):
    return hashlib.sha3_256(b).digest()


class Case:
    def __init__(self, d):
        self.name = d['name']
        self.items = [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in zip(d['keys'], d['values'])]
        self.root = bytes.fromhex(d['root'])
        self.digests = [bytes.fromhex(x) for x in d['digests']]


def fixture():
    """the cases of tests/golden/state_build.json; the reference accepted the empty key"""
    global _fixture
    if _fixture is None:
        with open(os.path.join(REPO, 'tests', 'golden', 'state_build.json')) as fh:
            data = json.load(fh)
        assert all(c.get('empty_key', 'accepted') == 'accepted' for c in data['cases'])
        _fixture = [Case(c) for c in data['cases']]
    return _fixture


def pairs(items):
    """(key, raw value) items -> sorted distinct (key, encoded value): what the device form takes"""
    from plenum_gpu.state_store import _pairs
    return _pairs(items)


def proof_fixture_tries():
    """per trie of tests/golden/state_proofs.json: (name, sorted (key, encoded value) pairs,
    root, {hash: node RLP}) -- the `own` rows' keys with their encoded values"""
    out = []
    for name, (root, db) in sorted(ss.tries().items()):
        kv = {}
        for r in sp.fixture():
            if r.kind == 'own' and r.trie == name:
                for k, v in r.kvs:
                    kv[k] = _encode(v)
        out.append((name, sorted(kv.items()), root, db))
    return out


def _encode(v):
    from plenum_gpu.state_proofs import rlp_encode
    return rlp_encode([v])


def boundary_pairs():
    """[(name, pairs)]: single leaves of 55 / 56 / 255 / 256 / 65,535 / 65,536 bytes (the list
    header's boundaries) and one trie holding all six values"""
    if 'boundary' not in _cache:
        out, vals = [], []
        for n in (55, 56, 255, 256, 65535, 65536):
            _, _, value = ss.leaf_trie(n)
            out.append(('leaf%d' % n, [(b'k', value)]))
            vals.append(value)
        out.append(('all', sorted((b'key%d' % i, v) for i, v in enumerate(vals))))
        _cache['boundary'] = out
    return _cache['boundary']


def random_pairs(n, seed, klen=32):
    rng = random.Random(seed)
    kv = {}
    while len(kv) < n:
        kv[bytes(rng.getrandbits(8) for _ in range(klen))] = _encode(bytes(rng.getrandbits(8)
                                                                           for _ in range(rng.randint(2, 60))))
    return sorted(kv.items())


def mixed_pairs(n, seed):
    """two thirds 32-byte keys, values of 2 - 250 bytes, as the fixture's mixed state"""
    rng = random.Random(seed)
    kv = {}
    for i in range(n):
        key = sha3(b'did:%d' % i) if i % 3 else b'attr:%d' % i
        kv[key] = _encode(bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 250))))
    return sorted(kv.items())


def chain_pairs():
    """64 keys of 32 bytes: key i shares exactly i nibbles with every later key, so the trie is
    a chain of 63 branches, the deepest the key length allows"""
    base = [7] * 64
    keys = []
    for i in range(64):
        nib = list(base)
        if i < 63:
            nib[i] = 3                      # leaves the chain at nibble i, below the others
        keys.append(bytes(16 * nib[2 * j] + nib[2 * j + 1] for j in range(32)))
    return sorted((k, _encode(b'value %d' % i)) for i, k in enumerate(keys))


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstatebuildcheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstatebuildcheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.sb_build.restype = ctypes.c_int
        so.sb_build.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp]
        _lib = so
    return _lib


class Built:
    """rc, root, n_nodes, n_bytes, blob, off, dig (n x 32), bad_index, max_level"""

    def nodes(self):
        return [self.blob[int(self.off[i]):int(self.off[i + 1])].tobytes() for i in range(self.n_nodes)]

    def db(self):
        out = {}
        for i, n in enumerate(self.nodes()):
            assert sha3(n) == self.dig[i].tobytes()
            out[sha3(n)] = n
        return out

    def same(self, other):
        """None, or what differs first"""
        for f in ('rc', 'root', 'n_nodes', 'n_bytes'):
            if getattr(self, f) != getattr(other, f):
                return f
        for f in ('off', 'blob', 'dig'):
            a, b = getattr(self, f), getattr(other, f)
            if a.shape != b.shape or not (a == b).all():
                return f
        return None


def pack(msgs):
    """blob (4-byte aligned by numpy, 16 spare bytes) and offsets"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b''.join(msgs) + b'\0' * 16, np.uint8).copy(), off


def host_build(prs, blob_cap=None, node_cap=None):
    """sb_build over (key, encoded value) pairs as given (no sorting) -> Built"""
    so = host_lib()
    kb, ko = pack([k for k, _ in prs])
    vb, vo = pack([v for _, v in prs])
    b = Built()
    root = np.zeros(32, np.uint8)
    nn, nb, bad, ml = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    args = [sp.ptr(kb), sp.ptr(ko), sp.ptr(vb), sp.ptr(vo), len(prs), sp.ptr(root), ctypes.byref(nn), ctypes.byref(nb)]
    b.rc = so.sb_build(*args, None, 0, None, 0, None, ctypes.byref(bad), ctypes.byref(ml))
    b.bad_index, b.max_level = bad.value, ml.value
    b.n_nodes, b.n_bytes = nn.value, nb.value
    b.blob, b.off, b.dig = np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros((0, 32), np.uint8)
    b.root = root.tobytes()
    if b.rc != OK:
        return b
    bc = b.n_bytes if blob_cap is None else blob_cap
    nc = b.n_nodes if node_cap is None else node_cap
    blob, off, dig = np.full(max(bc, 1), 0x5a, np.uint8), np.zeros(nc + 1, np.uint64), np.zeros((max(nc, 1), 32), np.uint8)
    b.rc = so.sb_build(*args, sp.ptr(blob), bc, sp.ptr(off), nc, sp.ptr(dig), None, None)
    b.root = root.tobytes()
    if b.rc == OK:
        b.blob, b.off, b.dig = blob[:b.n_bytes], off, dig[:b.n_nodes]
    else:
        b.untouched = bool((blob == 0x5a).all() and not off.any() and not dig.any())
    return b


def host_build_cached(name, prs):
    if name not in _cache:
        _cache[name] = host_build(prs)
    return _cache[name]


# ------------------------------------------------------------------ the case file
def write_cases(path, cases):
    """cases: [(pairs, expected Built)] in the layout of tools/hostcheck/statebuildcheck_main.cpp"""
    with open(path, 'wb') as fh:
        fh.write(b'SBC1' + struct.pack('<I', len(cases)))
        for prs, want in cases:
            fh.write(struct.pack('<Q', len(prs)))
            for msgs in ([k for k, _ in prs], [v for _, v in prs]):
                off = np.zeros(len(msgs) + 1, np.uint64)
                if msgs:
                    off[1:] = np.cumsum([len(m) for m in msgs])
                fh.write(off.tobytes() + b''.join(msgs))
            fh.write(struct.pack('<IQ', want.rc, want.bad_index))
            if want.rc == OK:
                fh.write(want.root + struct.pack('<QQ', want.n_nodes, want.n_bytes) + want.off.tobytes() +
                         want.blob.tobytes() + want.dig.tobytes())
