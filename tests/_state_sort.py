"""State-sort test helpers: the host sort of csrc/pv_trie_sort.h
(tools/hostcheck/statesortcheck.cpp), the case lists shared by tests/test_state_sort_host.py and
tests/test_gpu_state_sort.py, and the case file of statesortcheck_asan.  Every shuffle has a
fixed seed; the expected permutation is always plenum_gpu.state_store.sort_keys_host."""
import ctypes
import itertools
import os
import random
import struct
import subprocess

import numpy as np

import _state_build as sb
from conftest import REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
OK, BAD_OFFSET, BAD_LENGTH = 0, 1, 2   # statesort_host.h
TILE = 2048                            # plenum_gpu.state_store.SORT_TILE, checked against the header
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 65537)
PREFIX_LENGTHS = (5, 6, 7, 8, 13, 14, 15, 16)
_lib = None
_cache = {}


def shuffled(keys, seed):
    keys = list(keys)
    random.Random(seed).shuffle(keys)
    return keys


def random_keys(n, seed, klen=32):
    """n distinct random keys of klen bytes, in the order they were drawn"""
    rng = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        k = rng.getrandbits(8 * klen).to_bytes(klen, 'big')
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def size_keys(n):
    if ('size', n) not in _cache:
        _cache['size', n] = random_keys(n, 1000 + n)
    return _cache['size', n]


def short_strings():
    """every string of length 0 - 3 over {00, 01, 7f, 80, ff}: 156 keys, the empty key included"""
    alphabet = (0x00, 0x01, 0x7f, 0x80, 0xff)
    return [bytes(t) for n in range(4) for t in itertools.product(alphabet, repeat=n)]


def edge_keys():
    """the short strings bare and behind fixed prefixes of 5 .. 16 bytes, so that keys end at, one
    before and one after a word boundary; shuffled"""
    keys = list(short_strings())
    for plen in PREFIX_LENGTHS:
        prefix = bytes(range(0x41, 0x41 + plen))
        keys += [prefix + s for s in short_strings()]
    return shuffled(keys, 31)


def shared_keys(n, shared, tail, seed, copies=0):
    """n distinct keys of `shared` equal bytes and a tail of `tail` random bytes, `copies` of them
    present twice; shuffled"""
    prefix = bytes(random.Random(seed).getrandbits(8) for _ in range(shared))
    keys = [prefix + t for t in random_keys(n, seed + 1, tail)]
    return shuffled(keys + keys[:copies], seed + 2)


def long_keys():
    """300 keys of exactly 1,024 bytes that differ in the last byte only (so 44 byte values occur twice)"""
    body = bytes(random.Random(41).getrandbits(8) for _ in range(1023))
    return shuffled([body + bytes([i % 256]) for i in range(300)], 42)


def too_long_keys():
    """valid keys and, at index 17, one key of 1,025 bytes"""
    keys = random_keys(40, 43)
    keys[17] = b'\x55' * 1025
    return keys


def multiplicity_keys():
    """each of 2,000 keys present 1 - 5 times"""
    rng = random.Random(44)
    keys = []
    for k in random_keys(2000, 45):
        keys += [k] * rng.randint(1, 5)
    return shuffled(keys, 46)


def tile_run_keys():
    """2 TILE + 9 keys: positions TILE - 20 .. TILE + 19 hold one key, the rest are distinct"""
    keys = random_keys(2 * TILE + 9, 47)
    for i in range(TILE - 20, TILE + 20):
        keys[i] = keys[TILE - 20]
    return keys


def equal_by_length():
    """equal keys of length 7, 8 and 9 (three of each) among their neighbours in order"""
    keys = []
    for n in (7, 8, 9):
        keys += [b'abcdefghi'[:n]] * 3
    return shuffled(keys + [b'abcdefg\x00', b'abcdefgh\x00', b'abcdef', b'abcdefghj'], 48)


def mixed_keys():
    """the keys of _state_build.mixed_pairs(4096, 13): attr:%d keys next to SHA3 keys; shuffled"""
    if 'mixed' not in _cache:
        _cache['mixed'] = shuffled([k for k, _ in sb.mixed_pairs(4096, 13)], 49)
    return _cache['mixed']


def chain_keys(copies=0):
    """the 64 keys of _state_build.chain_pairs(), the first `copies` present twice; shuffled"""
    keys = [k for k, _ in sb.chain_pairs()]
    return shuffled(keys + keys[:copies], 50)


def accepted_cases():
    """[(name, keys)] of every case list that sorts"""
    out = [('size%d' % n, shuffled(size_keys(n), 2000 + n)) for n in SIZES]
    out += [('edges', edge_keys()),
            ('shared200', shared_keys(3000, 200, 8, 51, copies=10)),
            ('long1024', long_keys()),
            ('multiplicity', multiplicity_keys()),
            ('equal1000', [b'\x11' * 32] * 1000),
            ('tile_run', tile_run_keys()),
            ('equal789', equal_by_length()),
            ('mixed4096', mixed_keys()),
            ('chain', chain_keys()),
            ('chain_dup', chain_keys(copies=9)),
            ('empty_keys', [b'', b'', b'\x00', b'']),
            ('none', [])]
    return out


def mirror(keys):
    from plenum_gpu.state_store import sort_keys_host
    return sort_keys_host(keys)


def pack(keys, lead=0):
    """blob (`lead` unused bytes, the keys back to back, 16 spare bytes) and offsets"""
    off = np.full(len(keys) + 1, lead, np.uint64)
    if keys:
        off[1:] += np.cumsum([len(k) for k in keys]).astype(np.uint64)
    return np.frombuffer(b'\xee' * lead + b''.join(keys) + b'\0' * 16, np.uint8).copy(), off


# ------------------------------------------------------------------ the host sort
def host_lib():
    global _lib
    if _lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstatesortcheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstatesortcheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.ss_sort.restype = ctypes.c_int
        so.ss_sort.argtypes = [vp, vp, u64, ctypes.c_int, vp, vp, vp, vp]
        so.ss_tile.restype = ctypes.c_uint32
        so.ss_max_key_bytes.restype = ctypes.c_uint64
        _lib = so
    return _lib


def host_sort(keys, lsd=False, off=None, blob=None):
    """ss_sort -> (rc, perm, rounds, bad_index); perm is None when refused"""
    so = host_lib()
    if blob is None:
        blob, off = pack(keys)
    n = len(off) - 1
    perm = np.full(max(n, 1), 0xffffffff, np.uint32)
    m, bad, rounds = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = so.ss_sort(blob.ctypes.data, off.ctypes.data, n, int(lsd), perm.ctypes.data, ctypes.byref(m),
                    ctypes.byref(rounds), ctypes.byref(bad))
    if rc != OK:
        assert (perm == 0xffffffff).all()
        return rc, None, rounds.value, bad.value
    return rc, perm[:m.value].copy(), rounds.value, bad.value


# ------------------------------------------------------------------ the case file
def write_cases(path, cases):
    """cases: [(keys, off or None, rc, bad_index, perm, rounds)] in the layout of
    tools/hostcheck/statesortcheck_main.cpp; the blob is written without spare bytes"""
    with open(path, 'wb') as fh:
        fh.write(b'SSC1' + struct.pack('<I', len(cases)))
        for keys, off, rc, bad, perm, rounds in cases:
            blob = b''.join(keys)
            if off is None:
                off = pack(keys)[1]
            fh.write(struct.pack('<Q', len(off) - 1) + np.asarray(off, np.uint64).tobytes())
            fh.write(struct.pack('<Q', len(blob)) + blob)
            fh.write(struct.pack('<IQ', rc, bad))
            if rc == OK:
                fh.write(struct.pack('<Q', len(perm)) + np.asarray(perm, np.uint32).tobytes() +
                         struct.pack('<I', rounds))
