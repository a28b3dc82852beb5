"""Cases for the BLS COMMIT check's three check kernels (csrc/pv_bls.hip) at the
places the grouping pipeline and the lane-sharing kernels can go wrong: ragged
key segments, key sets on both sides of GROUP_LOCAL_KEYS, and H(m) at the edges
of try-and-increment and of SHA-256 padding.  Shared by tests/test_bls_cases.py
(the conditions on the reference alone, CPU) and tests/test_gpu_bls_shapes.py
(the kernels).

Every expected value comes from oracle/bn254_oracle.c (libbls_oracle.so) or
tests/_bn254_py.py: keys from bls_oracle_pubkey, signatures from
bls_oracle_sign, verdicts from bls_oracle_verify_batch.  The one exception is
the rule of include/plenum_verify.h for PV_BLS_KEY_NOT_IN_G2: a check against a
key on the twist that bls_oracle_g2_in_subgroup rejects has verdict 0.
Everything is deterministic (fixed seeds); nothing comes from the GPU."""
import ctypes
import functools
import hashlib
import json
import os
import random

import numpy as np

import _bn254_py as bn
from conftest import REPO, golden

ORACLE = os.path.join(REPO, 'oracle', 'libbls_oracle.so')
O_BYTES = bytes(128)                       # decodes to O as a key (off the twist) and as sigma (prefix 0)
G1_INF = b'\x04' + bytes(63) + b'\x01' + bytes(63)   # ECP::tobytes of O: AMCL's (0, 1)

# _native.set_tuning values that select each check kernel for a call of any size
KERNELS = {'pair': {'bls_quad_max': 0, 'bls_oct_max': 0}, 'quad': {'bls_oct_max': 0}, 'oct': {}}


@functools.lru_cache(None)
def oracle():
    return ctypes.CDLL(ORACLE)


@functools.lru_cache(None)
def generator():
    with open(golden('bls.json')) as fh:
        return bytes.fromhex(json.load(fh)['generator_hex'])


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------ oracle wrappers
def secret(i):
    """the i-th fixed secret scalar, 32 bytes big-endian (0..8 are the valid keys)"""
    return (int.from_bytes(hashlib.sha256(b'bls shapes key %d' % i).digest(), 'big') % bn.R).to_bytes(32, 'big')


@functools.lru_cache(None)
def pubkey(sk):
    out = ctypes.create_string_buffer(128)
    oracle().bls_oracle_pubkey(sk, generator(), out)
    return out.raw


@functools.lru_cache(None)
def sign(sk, msg):
    out = ctypes.create_string_buffer(128)
    oracle().bls_oracle_sign(sk, msg, ctypes.c_uint64(len(msg)), out)
    return out.raw


def hash_to_g1(msg):
    out = ctypes.create_string_buffer(128)
    oracle().bls_oracle_hash_to_g1(msg, ctypes.c_uint64(len(msg)), out)
    return out.raw


def aggregate_sigs(sigs):
    out = ctypes.create_string_buffer(128)
    oracle().bls_oracle_aggregate_sigs(b''.join(sigs), ctypes.c_uint64(len(sigs)), out)
    return out.raw


def verify_multi(sig, msg, keys):
    return oracle().bls_oracle_verify_multi(sig, ctypes.c_uint64(len(sig)), msg, ctypes.c_uint64(len(msg)),
                                            b''.join(keys), ctypes.c_uint64(len(keys)), generator())


def pack(msgs):
    """messages back to back -> (blob u8, off u64[n + 1])"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b''.join(msgs), np.uint8).copy(), off


def key_outside_g2(pk):
    """on the twist (not O) and rejected by the oracle's subgroup check"""
    return bn.g2_from_bytes(pk) is not None and oracle().bls_oracle_g2_in_subgroup(pk) == 0


def expected(keys, sig, blob, off, midx, kidx):
    """bls_oracle_verify_batch over the key array, then the header's rule: verdict
    0 for every check against a key of status PV_BLS_KEY_NOT_IN_G2"""
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 128)
    sig = np.ascontiguousarray(sig, np.uint8).reshape(-1, 128)
    midx, kidx = np.ascontiguousarray(midx, np.uint32), np.ascontiguousarray(kidx, np.uint32)
    assert len(midx) == len(kidx) == len(sig) and int(kidx.max()) < len(keys) and int(midx.max()) < len(off) - 1
    blob16 = np.concatenate([blob, np.zeros(16, np.uint8)])
    want = np.full(len(sig), 9, np.uint8)
    oracle().bls_oracle_verify_batch(_p(sig), None, _p(blob16), _p(off), _p(midx), _p(kidx), _p(keys), generator(),
                                     ctypes.c_uint64(len(sig)), _p(want), 8)
    assert set(want.tolist()) <= {0, 1}
    for k in sorted(set(kidx.tolist())):
        if key_outside_g2(keys[k].tobytes()):
            want[kidx == k] = 0
    return want


# ------------------------------------------------------------------ the message pool (part 3)
# b'hash-edge %d' % i needs INCREMENTS[j] steps of try-and-increment for i = HASH_EDGE_I[j]
HASH_EDGE_I = (0, 1, 6, 19, 15, 211, 4, 488, 287, 1696, 1656, 6263, 19679, 17250)
INCREMENTS = tuple(range(13)) + (14,)
PAD_EDGE_LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128)   # around SHA-256's 55/56 and 64-byte edges


def increments(msg):
    """how often hash_to_g1's loop (tests/_bn254_py.py) increments the digest before x^3 + 2 is a square"""
    x0 = int.from_bytes(hashlib.sha256(msg).digest(), 'big')
    n = 0
    while not bn.is_qr(((x0 + n) % bn.P) ** 3 + bn.B):
        n += 1
    return n


@functools.lru_cache(None)
def pool():
    """25 messages, packed back to back: start offsets at every residue mod 4, a
    count that is no multiple of 8 (k_bls_prep's last block is partly filled)"""
    rnd = random.Random(31)
    msgs = [b'hash-edge %d' % i for i in HASH_EDGE_I] + [rnd.randbytes(n) for n in PAD_EDGE_LENGTHS]
    return tuple(msgs)


# ------------------------------------------------------------------ signature classes (part 1)
def _xy(s):
    assert s[0] == 4
    return int.from_bytes(s[1:33], 'big'), int.from_bytes(s[33:65], 'big')


def _enc(x, y):
    return b'\x04' + x.to_bytes(32, 'big') + y.to_bytes(32, 'big') + bytes(63)


def _compressed(s, parity_flip):
    x, y = _xy(s)
    return bytes([2 | ((y & 1) ^ parity_flip)]) + x.to_bytes(32, 'big') + bytes(95)


def _bitflip_y(s):
    b = bytearray(s)
    b[64] ^= 0x10
    return bytes(b)


# name -> (sigma from (own secret, another secret, message, another message), verdict for a valid key)
CLASSES = (
    ('valid', lambda sk, sk2, m, m2: sign(sk, m), 1),
    ('other-message', lambda sk, sk2, m, m2: sign(sk, m2), 0),
    ('other-key', lambda sk, sk2, m, m2: sign(sk2, m), 0),
    ('negated', lambda sk, sk2, m, m2: (lambda x, y: _enc(x, bn.P - y))(*_xy(sign(sk, m))), 0),
    ('sigma-O', lambda sk, sk2, m, m2: O_BYTES, 0),
    ('compressed', lambda sk, sk2, m, m2: _compressed(sign(sk, m), 0), 1),
    ('compressed-wrong-parity', lambda sk, sk2, m, m2: _compressed(sign(sk, m), 1), 0),
    ('x-plus-p', lambda sk, sk2, m, m2: (lambda x, y: _enc(x + bn.P, y))(*_xy(sign(sk, m))), 0),
    ('y-bitflip', lambda sk, sk2, m, m2: _bitflip_y(sign(sk, m)), 0),
)
CLASS_VERDICT = {name: v for name, _, v in CLASSES}
_CLASS_FN = {name: f for name, f, _ in CLASSES}

N_VALID = 8
RAGGED_COUNTS = (1, 7, 8, 9, 15, 16, 17, 33, 3, 3, 0, 31)    # checks per key entry: both sides of 8 / 16 / 32
RAGGED_STATUS = [0] * 8 + [1, 2, 0, 0]
# entries 8 (O) and 9 (outside G2) get these classes; the signer is secret 0
SPECIAL_CLASSES = {8: ('valid', 'sigma-O', 'compressed'), 9: ('valid', 'sigma-O', 'compressed')}
SPECIAL_VERDICT = {8: (0, 1, 0), 9: (0, 0, 0)}


@functools.lru_cache(None)
def valid_keys():
    return tuple(pubkey(secret(i)) for i in range(N_VALID + 1))


def _assemble(keys, rows, seed):
    """rows of (key entry, message, sigma bytes, label), shuffled -> arrays + expected verdicts"""
    rows = list(rows)
    random.Random(seed).shuffle(rows)
    blob, off = pack(pool())
    sig = np.frombuffer(b''.join(r[2] for r in rows), np.uint8).reshape(-1, 128).copy()
    kidx = np.array([r[0] for r in rows], np.uint32)
    midx = np.array([r[1] for r in rows], np.uint32)
    karr = np.frombuffer(b''.join(keys), np.uint8).reshape(-1, 128).copy()
    want = expected(karr, sig, blob, off, midx, kidx)
    return dict(keys=karr, sig=sig, blob=blob, off=off, midx=midx, kidx=kidx, want=want,
                labels=[r[3] for r in rows])


@functools.lru_cache(None)
def ragged():
    """part 1: 12 key entries, 143 checks scattered through the call"""
    vk = valid_keys()
    keys = list(vk[:N_VALID]) + [O_BYTES, bn.g2_to_bytes(bn.twist_point_outside_g2()), vk[N_VALID], vk[0]]
    owner = list(range(N_VALID)) + [0, 0, N_VALID, 0]        # the secret behind (or, for 8 and 9, used with) an entry
    msgs = pool()
    rows, table = [], []
    for e, cnt in enumerate(RAGGED_COUNTS):
        for c in range(cnt):
            name = SPECIAL_CLASSES[e][c] if e in SPECIAL_CLASSES else CLASSES[c % len(CLASSES)][0]
            m = (7 * e + 3 * c) % len(msgs)
            sk, sk2 = secret(owner[e]), secret((owner[e] + 1) % N_VALID)
            sigma = _CLASS_FN[name](sk, sk2, msgs[m], msgs[(m + 1) % len(msgs)])
            label = 'key{}#{}:{}:msg{}'.format(e, c, name, m)
            rows.append((e, m, sigma, label))
            table.append(SPECIAL_VERDICT[e][c] if e in SPECIAL_VERDICT else CLASS_VERDICT[name])
    c = _assemble(keys, rows, 143)
    # the class table's verdict per check, in the shuffled order (the CPU test holds it against the oracle)
    by_label = {r[3]: t for r, t in zip(rows, table)}
    c['table'] = np.array([by_label[x] for x in c['labels']], np.uint8)
    return c


# ------------------------------------------------------------------ key sets around GROUP_LOCAL_KEYS (part 2)
GROUP_LOCAL_KEYS = 2048
KEYSET_COUNTS = {2048: {0: 17, 1: 1, 255: 2, 256: 9, 2046: 2, 2047: 9},
                 2049: {0: 17, 1: 1, 255: 2, 256: 1, 2046: 2, 2047: 9, 2048: 9}}


@functools.lru_cache(None)
def keyset(nkeys):
    """part 2: nkeys entries (entry e = valid key e mod 8), ~40 checks on the first
    and last entries and around index 256, classes valid / other-message / other-key"""
    vk = valid_keys()
    keys = [vk[e % N_VALID] for e in range(nkeys)]
    msgs = pool()
    rows = []
    for e, cnt in sorted(KEYSET_COUNTS[nkeys].items()):
        for c in range(cnt):
            name = CLASSES[c % 3][0]
            m = (5 * e + 3 * c) % len(msgs)
            sk, sk2 = secret(e % N_VALID), secret((e + 1) % N_VALID)
            sigma = _CLASS_FN[name](sk, sk2, msgs[m], msgs[(m + 1) % len(msgs)])
            rows.append((e, m, sigma, 'key{}#{}:{}:msg{}'.format(e, c, name, m)))
    return _assemble(keys, rows, nkeys)


# ------------------------------------------------------------------ H(m) under the check kernels (part 3b)
@functools.lru_cache(None)
def hash_checks():
    """one valid key, two checks per message of the pool: the oracle's sigma over
    it (1) and the oracle's sigma over the pool's next message (0)"""
    msgs = pool()
    sk = secret(3)
    rows = []
    for m in range(len(msgs)):
        rows.append((0, m, sign(sk, msgs[m]), 'msg{}:valid'.format(m)))
        rows.append((0, m, sign(sk, msgs[(m + 1) % len(msgs)]), 'msg{}:next-message'.format(m)))
    return _assemble([pubkey(sk)], rows, 50)


# ------------------------------------------------------------------ small pieces (part 4)
EDGE_SCALARS = (1, 2, bn.R - 1, bn.R + 1, 1 << 255, (1 << 256) - 1)


def g1_neg_bytes(s):
    x, y = _xy(s)
    return _enc(x, (bn.P - y) % bn.P)


@functools.lru_cache(None)
def aggregate_sets():
    """signature sets whose running sum passes through O and goes on"""
    m = pool()[2]
    s, t = sign(secret(0), m), sign(secret(1), m)
    ns = g1_neg_bytes(s)
    return ((s, ns, t), (s, ns, s, s), (O_BYTES, s), (s, O_BYTES, ns, t, t))


@functools.lru_cache(None)
def multi_checks():
    """(sigma, message, key list) with key sums that pass through O or double: [k, -k, k2] and [k, k, -k]"""
    m = pool()[5]
    k, k2 = valid_keys()[0], valid_keys()[1]
    nk = bn.g2_to_bytes(bn.g2_neg(bn.g2_from_bytes(k)))
    s, s2 = sign(secret(0), m), sign(secret(1), m)
    return ((s2, m, (k, nk, k2)), (s, m, (k, nk, k2)), (s, m, (k, k, nk)), (s2, m, (k, k, nk)))
