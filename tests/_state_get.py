"""State-read test helpers: the host build of csrc/pv_trie_get.h
(tools/hostcheck/stategetcheck.cpp), the Python mirror run over the same queries, the case file of
stategetcheck_asan, and the scenarios -- the smallest tries at which the read walk, the decode and
the copy can go wrong -- shared by the CPU and the GPU tests.

A scenario is (add batches, roots, root_idx or None, keys); every scenario is read in both decode
modes."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import _state_proofs as sp
import _state_store as ss
from conftest import REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
OK, VALUE_MISMATCH, NODE_MISSING, MALFORMED = range(4)   # PV_SP_* of plenum_verify.h
sha3 = ss.sha3
_lib = None


class Result:
    """per query: status, found, val_off (n + 1), the compact value bytes"""

    def __init__(self, n):
        self.status, self.found = np.full(n, 0xee, np.uint8), np.full(n, 0xee, np.uint8)
        self.val_off = np.zeros(n + 1, np.uint64)
        self.blob = np.zeros(0, np.uint8)
        self.rc = 0

    def value(self, q):
        """None unless found; b'' is a present key with an empty payload"""
        if not self.found[q]:
            return None
        return self.blob[int(self.val_off[q]):int(self.val_off[q + 1])].tobytes()

    def values(self):
        return [self.value(q) for q in range(len(self.status))]

    def same(self, other):
        """None, or what differs first"""
        for f in ('status', 'found', 'val_off', 'blob'):
            a, b = getattr(self, f), getattr(other, f)
            if a.shape != b.shape or not (a == b).all():
                return f
        return None


def mirror_get(db, roots, root_idx, keys, decode):
    """get_host over every query, as a Result"""
    from plenum_gpu.state_store import get_host
    res = Result(len(keys))
    chunks, pos = [], 0
    for q, key in enumerate(keys):
        st, found, value = get_host(db, roots[root_idx[q] if root_idx is not None else q], key, decode)
        res.status[q], res.found[q] = st, found
        chunks.append(value)
        pos += len(value)
        res.val_off[q + 1] = pos
    res.blob = np.frombuffer(b''.join(chunks), np.uint8).copy()
    return res


# ------------------------------------------------------------------ the host build
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstategetcheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstategetcheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.sgc_create.restype, so.sgc_create.argtypes = vp, [u64]
        so.sgc_free.restype, so.sgc_free.argtypes = None, [vp]
        so.sgc_add.restype, so.sgc_add.argtypes = u64, [vp, vp, vp, u64]
        so.sgc_get.restype = ctypes.c_int
        so.sgc_get.argtypes = [vp, vp, vp, u64, vp, vp, u64, ctypes.c_int32, vp, vp, vp, vp, u64]
        so.sgc_decode.restype = ctypes.c_int
        so.sgc_decode.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        _lib = so
    return _lib


def host_decode(value):
    """tg_decode on the host build -> the payload, or None"""
    buf = np.frombuffer(bytes(value) + b'\0', np.uint8).copy()
    pb, pe = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if not host_lib().sgc_decode(sp.ptr(buf), len(value), ctypes.byref(pb), ctypes.byref(pe)):
        return None
    return bytes(value[pb.value:pe.value])


class HostStore:
    """the store of tools/hostcheck/statestore_host.h read by stateget_host.h; keeps {digest: node}"""

    def __init__(self, batches=()):
        self.so = host_lib()
        self.h = ctypes.c_void_p(self.so.sgc_create(1))
        self.db = {}
        for b in batches:
            self.add(b)

    def __del__(self):
        if self.h:
            self.so.sgc_free(self.h)
            self.h = None

    def add(self, nodes):
        nodes = list(nodes)
        for n in nodes:
            self.db[sha3(n)] = n
        blob, off = ss.pack(nodes)
        return self.so.sgc_add(self.h, sp.ptr(blob), sp.ptr(off), len(nodes))

    def get(self, roots, root_idx, keys, decode, val_cap=None, sizing=False):
        """-> Result (with .rc, the return code)"""
        n = len(keys)
        res = Result(n)
        rts = np.frombuffer(b''.join(roots) + b'\0', np.uint8).copy()
        ridx = None if root_idx is None else np.asarray(root_idx, np.uint32)
        kblob, koff = ss.pack(keys)
        args = [self.h, sp.ptr(rts), sp.ptr(ridx), len(roots), sp.ptr(kblob), sp.ptr(koff), n, int(decode),
                sp.ptr(res.status), sp.ptr(res.found), sp.ptr(res.val_off)]
        res.rc = self.so.sgc_get(*args, None, 0)
        if sizing or res.rc:
            return res
        total = int(res.val_off[n])
        blob = np.zeros(max(total, 1), np.uint8)
        res.rc = self.so.sgc_get(*args, sp.ptr(blob), total if val_cap is None else val_cap)
        res.blob = blob[:total] if res.rc == 0 else np.zeros(0, np.uint8)
        return res


def run_host(sc, decode):
    """-> (host Result, mirror Result) of one scenario; the two must agree"""
    batches, roots, ridx, keys = sc
    st = HostStore(batches)
    got = st.get(roots, ridx, keys, decode)
    want = mirror_get(st.db, roots, ridx, keys, decode)
    assert got.rc == 0
    assert got.same(want) is None, got.same(want)
    return got, want


# ------------------------------------------------------------------ the case file
def write_cases(path, cases, values):
    """cases: [(batches, roots, root_idx or None, keys, decode, expected Result)], values: [(stored
    value, payload or None)], in the layout of tools/hostcheck/stategetcheck_main.cpp"""
    with open(path, 'wb') as fh:
        fh.write(b'SGC1' + struct.pack('<I', len(cases)))
        for batches, roots, root_idx, keys, decode, want in cases:
            fh.write(struct.pack('<Q', len(batches)))
            for nodes in batches:
                off = np.zeros(len(nodes) + 1, np.uint64)
                off[1:] = np.cumsum([len(x) for x in nodes])
                fh.write(struct.pack('<Q', len(nodes)) + off.tobytes() + b''.join(nodes))
            fh.write(struct.pack('<Q', len(roots)) + b''.join(roots))
            fh.write(struct.pack('<QB', len(keys), root_idx is not None))
            if root_idx is not None:
                fh.write(np.asarray(root_idx, np.uint32).tobytes())
            koff = np.zeros(len(keys) + 1, np.uint64)
            koff[1:] = np.cumsum([len(k) for k in keys])
            fh.write(koff.tobytes() + b''.join(keys))
            fh.write(struct.pack('<i', int(decode)))
            fh.write(want.status.tobytes() + want.found.tobytes() + want.val_off.tobytes() + want.blob.tobytes())
        fh.write(struct.pack('<I', len(values)))
        for value, payload in values:
            fh.write(struct.pack('<Q', len(value)) + value)
            if payload is None:
                fh.write(struct.pack('<BQQ', 0, 0, 0))
            else:
                pb = _payload_begin(value)
                fh.write(struct.pack('<BQQ', 1, pb, pb + len(payload)))


def _payload_begin(value):
    """where the first item's payload starts in an accepted stored value"""
    from plenum_gpu.state_proofs import _rlp_item
    head = _rlp_item(value, 0, len(value))
    return _rlp_item(value, head[1], head[2])[1]


# ------------------------------------------------------------------ tries
def enc(payload):
    from plenum_gpu.state_proofs import rlp_encode
    return rlp_encode([payload])


def trie(pairs):
    """(key, stored value) pairs, the stored value taken as it is -> (root, {hash: node RLP})"""
    from plenum_gpu.state_store import build_encoded_host
    return build_encoded_host(sorted(dict(pairs).items()))


def _v(n, tag):
    """n distinct bytes, none of them RLP-special by accident of position"""
    return bytes((37 * i + tag) % 251 + 1 for i in range(n))


# a key that is a proper prefix of another (the branch's value slot), an extension over a branch,
# hashed leaves, an inline (< 32-byte) leaf inside a branch and an inline branch
SHAPE_PAIRS = [(b'k', enc(_v(40, 1))), (b'k1', enc(_v(40, 2))), (b'k12', enc(_v(35, 3))),
               (b'\xab\xcd\x10\x01', enc(_v(40, 4))), (b'\xab\xcd\x20\x02', enc(_v(40, 5))),
               (b'\x11\x22\x33', enc(_v(40, 6))),
               (b'\x31\x01', enc(b'a')), (b'\x31\x02', enc(b'\x90')),          # two inline leaves: an inline branch
               (b'\x41\x07', enc(b'in')), (b'\x45\x07', enc(_v(40, 7)))]        # an inline leaf beside a hashed one
SHAPE_ABSENT = [b'\x11\x23\x33',            # diverges inside the leaf path of 11 22 33
                b'\xab\xc1\x10\x01',        # diverges inside the extension over [b, c, d]
                b'\xab\xcd\x30\x01',        # an empty branch slot
                b'\x11\x22', b'\xab',       # shorter than the stored path
                b'\x11\x22\x33\x44', b'k123',   # longer than the stored path
                b'\xab\xcd',                # ends at a branch without a value
                b'', b'\x31\x03', b'\x41']


def sc_shapes():
    from plenum_gpu.state_proofs import BLANK_ROOT
    root, db = trie(SHAPE_PAIRS)
    from plenum_gpu.state_store import walk_host
    # the root alone hashed: the extension, the branch and the leaf under it inline; root and branch
    # hashed, the leaf inline
    assert [len(walk_host(db, root, k)[1]) for k in (b'\x31\x01', b'\x41\x07')] == [1, 2]
    leaf_root, leaf_db = trie([(b'only', enc(_v(40, 8)))])
    keys = [k for k, _ in SHAPE_PAIRS] + SHAPE_ABSENT
    one = [b'only', b'onlx', b'onl', b'only1', b'']
    return ([list(db.values()), list(leaf_db.values())], [root, leaf_root, BLANK_ROOT],
            [0] * len(keys) + [1] * len(one) + [2, 2], keys + one + [b'k', b''])


PAYLOAD_LENGTHS = (0, 1, 1, 54, 55, 56, 255, 256, 1100)


def payloads():
    """the string- and list-header boundaries: payload q has PAYLOAD_LENGTHS[q] bytes, the second
    one-byte payload is >= 0x80 (it takes a string header, the first is its own item)"""
    out = []
    for q, n in enumerate(PAYLOAD_LENGTHS):
        p = _v(n, 10 + q)
        if n == 1:
            p = b'\x05' if q == 1 else b'\x85'
        out.append((b'pay:%d' % q, p))
    return out


def sc_payloads():
    """a length-0 payload is a stored rlp([b'']) = c1 80, which only a raw node can bring"""
    pls = payloads()
    root, db = trie([(k, enc(p)) for k, p in pls])
    return [list(db.values())], [root], [0] * (len(pls) + 1), [k for k, _ in pls] + [b'pay:x']


# stored values that the decode refuses, and (second table) lenient forms it accepts
HOSTILE_VALUES = [
    b'\x83abc',                 # a bare string
    b'\x05',                    # a bare byte
    b'\xc0',                    # an empty list
    b'\xc2\xc1\x01',            # the first item is a list
    b'\xc5\x83ab',              # the list's length overruns the value
    b'\xc2\x83ab',              # the list ends before the value does
    b'\xc3\x85ab',              # the first item's length overruns the list
    b'\xc3\xb8\x05a',           # a long string whose length overruns
    b'\xc2\xb9\x01',            # a long string whose length bytes overrun
    b'\xf8',                    # a long list header alone
    b'\xf9\x00',                # ... with one of its two length bytes
    b'\xf8\x03\x81',            # a long list over less than it says
    b'\xbf' + b'\xff' * 8,      # eight length bytes of 0xff
    b'\xc9\xbf' + b'\xff' * 8,  # ... inside a list
]
LENIENT_VALUES = [
    (b'\xf8\x02\x81\x99', b'\x99'),                       # a long list header over a short length
    (b'\xc3\xb8\x01\x07', b'\x07'),                       # a long string header over one byte
    (b'\xc4\x82hi\x01', b'hi'),                           # items after the first are not looked at
    (b'\xc3\x81\x05\xc0', b'\x05'),                       # a byte below 0x80 under a string header
    (b'\xf9\x00\x02\x81\x99', b'\x99'),                   # a leading zero in the length
]


def sc_hostile():
    """one trie that holds every hostile and every lenient stored value between well-formed
    neighbours; without decode each reads back as it is stored"""
    pairs = []
    for i, v in enumerate(HOSTILE_VALUES):
        pairs += [(b'h%02d-' % i, enc(_v(20 + i, 40 + i))), (b'h%02d' % i, v)]
    for i, (v, _) in enumerate(LENIENT_VALUES):
        pairs.append((b'l%02d' % i, v))
    root, db = trie(pairs)
    return [list(db.values())], [root], [0] * len(pairs), [k for k, _ in pairs]


def sc_roots():
    """two roots in one call (an overwritten key reads old at the old root and new at the new one),
    a root the store does not hold, and a store missing one child"""
    from plenum_gpu.state_store import apply_encoded_host
    base = [(b'\x10' + bytes([i]) * 3, enc(_v(40, 60 + i))) for i in range(6)]
    r0, db0 = trie(base)
    r1, db1 = apply_encoded_host(db0, r0, [(base[2][0], enc(b'new value'))])
    keys = [k for k, _ in base]
    part = [(bytes([16 * s + 1, 7]), enc(_v(40, 80 + s))) for s in range(4)]
    r2, db2 = trie(part)
    gone = next(h for h, n in db2.items() if h != r2 and part[1][1] in n)      # the leaf of part[1]
    held = [n for h, n in db2.items() if h != gone]
    pk = [k for k, _ in part]
    return ([list(db0.values()), list(db1.values()), held], [r0, r1, b'\x11' * 32, r2],
            [0] * len(keys) + [1] * len(keys) + [2] + [3] * len(pk), keys + keys + [keys[0]] + pk)


COUNTS = (1, 63, 64, 65, 257)
# value lengths around the lane group (16), the wave (64) and one block's worth of groups
COUNT_LENGTHS = (1, 15, 16, 17, 0, 31, 32, 33, 63, 64, 65, 127, 129, 3, 255, 257, 100)


def count_trie():
    pairs = [(sha3(b'count:%d' % i), enc(_v(n, 100 + i))) for i, n in enumerate(COUNT_LENGTHS)]
    root, db = trie(pairs)
    return pairs, root, db


def sc_count(n):
    """n queries that cycle through the keys of count_trie and, every seventh, an absent key"""
    pairs, root, db = count_trie()
    keys = [sha3(b'none:%d' % q) if q % 7 == 6 else pairs[q % len(pairs)][0] for q in range(n)]
    return [list(db.values())], [root], [0] * n, keys


def scenarios():
    out = {'shapes': sc_shapes(), 'payloads': sc_payloads(), 'hostile': sc_hostile(), 'roots': sc_roots()}
    for n in COUNTS:
        out['count%d' % n] = sc_count(n)
    return out
