"""Pairs of DISTINCT synthetic batches for the two-batches-in-flight tests, and
the checker of their outputs.  Importing this needs no GPU.

The async verify slots (pv_*_device_async, workspace 0 / 1) exist so that two
batches can be in flight at once.  A test that puts the same batch in both
slots cannot see one slot computing from the other's state: the bytes come out
right either way.  Here every pair (A, B) differs in size, message-length law,
keys and tamper positions, and meets the

    CONDITION ON THE PAIRS: the expected bitmaps of A and B differ in EVERY
    64-signature word they both have (every word of the shorter bitmap, its
    partial last word included),

so a swapped, mixed or stale word of the other batch can never look right.
Every n is no multiple of 64 (the last bitmap word is partial; its unused high
bits are zero in every kernel's output), except WIDE_A's 25 * 8000, the size
of C3's pipelined pass.

Everything expected comes from the synth spec (plenum_gpu.synth) alone:
expected_tamper() is pure Python, the verdict of signature i is `not tampered`,
and the bitmap is that packed little-endian into int64 words.
"""
import functools
from collections import namedtuple

import numpy as np

from plenum_gpu import synth

# first / n count signatures (COMMIT: first = first 3PC batch * n_nodes);
# mlen..mlen_max is the message-length range (unused by COMMIT); key_mod > 0 or
# wide makes the batch run the prepared-key path
Params = namedtuple('Params', 'mode cfg first n mlen mlen_max key_mod n_nodes wide')
Expected = namedtuple('Expected', 'verdict bitmap')

SENTINEL_VERDICT = 7     # what the tests fill the outputs with before a schedule
SENTINEL_WORD = -1


def _plain(mode, cfg, first, n, mlen, mlen_max=None, key_mod=0):
    return Params(mode, cfg, first, n, mlen, mlen if mlen_max is None else mlen_max, key_mod, 25, False)


def _commit(n_nodes, first_batch, n_batches):
    return Params(synth.COMMIT, 3, first_batch * n_nodes, n_batches * n_nodes, 0, 0, 0, n_nodes, True)


GENERIC_A = _plain(synth.RANGE, 4, 0, 200_037, 128, 1024)
GENERIC_B = _plain(synth.FIXED, 2, 777, 70_001, 256)
KEYED_A = _plain(synth.RANGE, 4, 0, 200_037, 128, 1024, key_mod=4096)
# first 3,000,000 leaves words 54 and 592 equal to A's; 3,000,128 leaves none
KEYED_B = _plain(synth.RANGE, 4, 3_000_128, 70_001, 128, 512, key_mod=1021)
WIDE_A = _commit(25, 31, 8000)
WIDE_B = _commit(16, 9000, 3001)
SMALL_B = _plain(synth.FIXED, 2, 5_000_000, 1000, 256)   # <= LAT_MAX_DEFAULT: the one-launch latency kernel

PAIRS = {
    'generic': (GENERIC_A, GENERIC_B),
    'keyed': (KEYED_A, KEYED_B),
    'wide': (WIDE_A, WIDE_B),
    'mixed': (GENERIC_A, KEYED_B),              # generic path beside keyed path
    'small_beside_large': (GENERIC_A, SMALL_B),
}
BATCH_NAMES = {GENERIC_A: 'generic_A', GENERIC_B: 'generic_B', KEYED_A: 'keyed_A', KEYED_B: 'keyed_B',
               WIDE_A: 'wide_A', WIDE_B: 'wide_B', SMALL_B: 'small_B'}
BATCHES = tuple(BATCH_NAMES)
assert set(BATCHES) == {p for pair in PAIRS.values() for p in pair}


def is_keyed(p):
    return bool(p.key_mod) or p.wide


def commit_batches(p):
    """(first 3PC batch, number of 3PC batches) of a COMMIT parameter set."""
    assert p.mode == synth.COMMIT and p.first % p.n_nodes == 0 and p.n % p.n_nodes == 0
    return p.first // p.n_nodes, p.n // p.n_nodes


@functools.lru_cache(maxsize=None)
def expected_tamper(p):
    """tamper flags (n,) bool of the parameter set, from the synth spec alone (read-only)."""
    if p.mode == synth.COMMIT:
        b0, nb = commit_batches(p)
        t = np.concatenate([synth.c3_slots(b0 + j, p.n_nodes)[1] for j in range(nb)]).astype(bool)
    else:
        t = np.fromiter((synth.tampered(p.cfg, p.first + j) for j in range(p.n)), dtype=bool, count=p.n)
    assert t.shape == (p.n,)
    t.setflags(write=False)
    return t


def pack_bitmap(verdict):
    """(n,) 0/1 -> ceil(n/64) int64 words, bit i % 64 of word i // 64; unused high bits zero."""
    n = len(verdict)
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = verdict
    return np.packbits(bits, bitorder='little').view(np.int64)


@functools.lru_cache(maxsize=None)
def expected_outputs(p):
    """Expected(verdict (n,) uint8, bitmap int64 words) of the parameter set (read-only)."""
    v = (~expected_tamper(p)).astype(np.uint8)
    bm = pack_bitmap(v)
    v.setflags(write=False)
    bm.setflags(write=False)
    return Expected(v, bm)


def check_outputs(verdict, bitmap, expected):
    """None when verdict / bitmap (numpy arrays read back from the device) are
    exactly `expected`; else the first difference as (what, index, got, want):
    the first wrong verdict byte, else the first wrong bitmap word (a wrong
    length is reported as index 'len')."""
    verdict = np.asarray(verdict)
    bitmap = np.asarray(bitmap).view(np.int64)
    for what, got, want in (('verdict', verdict, expected.verdict), ('bitmap', bitmap, expected.bitmap)):
        if got.shape != want.shape:
            return what, 'len', got.shape, want.shape
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            return what, i, int(got[i]), int(want[i])
    return None


def common_words(a, b):
    """number of bitmap words both parameter sets have"""
    return (min(a.n, b.n) + 63) // 64


def equal_words(a, b):
    """indices of the common bitmap words in which the expected bitmaps of a and b agree"""
    k = common_words(a, b)
    return np.flatnonzero(expected_outputs(a).bitmap[:k] == expected_outputs(b).bitmap[:k])


def make_batch(p, device=0):
    """The signed SyntheticBatch of a parameter set (signs on the GPU), with its
    key cache set up when the set is keyed and output sets for both slots."""
    from plenum_gpu.device import SyntheticBatch
    b = SyntheticBatch(device, p.n, p.mlen, cfg=p.cfg, first=p.first, key_mod=p.key_mod, mode=p.mode,
                       mlen_max=p.mlen_max, n_nodes=p.n_nodes)
    if is_keyed(p):
        assert b.use_key_cache(True, wide=p.wide)
    b.make_slots()
    return b
