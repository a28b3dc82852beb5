"""The length / alignment grid of the Ed25519 hash routes (pure Python + numpy).

Every device-side form of SHA-512(R || A || M) and the signer's two hashes are
built on msg_fetch / msg_assemble / hram_assemble_ra or on sha512_prefixed /
msg_bytes8 (csrc/pv_verify_core.h).  What those depend on is the message
length (block count, where the 0x80 pad and the length words fall) and the
start address of the message modulo 4 (`mis`).  build() returns one signed
batch that holds every length of LENGTHS at every start alignment 0..3, signed
by the oracle, with a known set of rows made to fail.

Row kinds:
  'grid'      one per (length, alignment) pair
  'filler'    a 1-3 byte message in front of a grid row that needs it to start
              at its alignment; an ordinary signed row, checked like the rest
  'precheck'  PRECHECK_RUN rows at the head of the batch (indices 0..63: the
              first 64 indices one k_hash wave takes) whose S fails the
              canonical-scalar pre-check, so that wave has nothing to hash;
              their lengths are multiples of 4, so they shift no alignment

Rejections (everything else must verify):
  * every third non-empty grid row: last message byte flipped after signing
  * every seventh non-empty grid row left untouched by that: first byte flipped
  * the 'precheck' rows and ISOLATED_PRECHECK filler rows: sig[i, 63] |= 0xf0
"""
import collections

import numpy as np

import _oracle as orc

N_SEEDS = 61          # a prime: the seed pool is cycled, so the keyed routes see every key many times
PRECHECK_RUN = 64     # one full wavefront of k_hash / k_chunk_half
ISOLATED_PRECHECK = 5


def hram_blocks(mlen):
    """SHA-512 compressions of R || A || M (64 + mlen bytes, the 0x80 pad, a 16-byte length)"""
    return (64 + mlen + 17 + 127) // 128


def edge_lengths():
    """e-2 .. e+2 around, for k = 1..7: 128k - 81 (last length with k blocks of
    R || A || M), 128k - 64 (R || A || M ends on a block), and the same two edges
    of the signer's 32-byte-prefix hash, 128k - 49 and 128k - 32"""
    out = set()
    for k in range(1, 8):
        for e in (128 * k - 81, 128 * k - 64, 128 * k - 49, 128 * k - 32):
            out.update(range(e - 2, e + 3))
    return out


SPECIAL = (1000, 1023, 1024, 1025, 4096)
LENGTHS = tuple(sorted(set(range(200)) | edge_lengths() | set(SPECIAL)))
FULL_PAIRS = tuple((ln, a) for ln in LENGTHS for a in range(4))
# the thinned grid of the slow host-build entries: every edge length and the
# special ones at all four alignments, 0..199 at alignment 0 only
_EDGE = edge_lengths() | set(SPECIAL)
THIN_PAIRS = tuple((ln, a) for ln in LENGTHS for a in range(4) if ln in _EDGE or a == 0)

Cases = collections.namedtuple('Cases', 'seeds pk sig blob off want clean_blob clean_sig length align kind tamper')
# seeds (n,32), pk (n,32), sig (n,64): the final arrays; blob u8, off u64 (n+1)
# want (n,) bool: the oracle's verdicts on the final arrays
# clean_blob / clean_sig: before any tampering (every row verifies; the signer's input and output)
# length, align (n,) int; kind (n,) str; tamper (n,) str: '', 'last', 'first' or 'precheck'


def build(pairs=FULL_PAIRS, seed=20261020):
    rng = np.random.default_rng(seed)
    lens, kinds, aligns = [], [], []
    cur = 0

    def add(ln, kind):
        nonlocal cur
        lens.append(ln)
        kinds.append(kind)
        aligns.append(cur % 4)
        cur += ln

    for j in range(PRECHECK_RUN):
        add(4 * (j % 8), 'precheck')
    for ln, a in pairs:
        if cur % 4 != a:
            add((a - cur) % 4, 'filler')
        add(ln, 'grid')
    n = len(lens)
    length = np.array(lens, np.int64)
    align = np.array(aligns, np.int64)
    kind = np.array(kinds)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(length)
    clean_blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    pool = rng.integers(0, 256, (N_SEEDS, 32), dtype=np.uint8)
    seeds = np.ascontiguousarray(pool[np.arange(n) % N_SEEDS])
    pk, clean_sig = orc.sign_batch(seeds, clean_blob, off)

    blob, sig = clean_blob.copy(), clean_sig.copy()
    tamper = np.array([''] * n, dtype='U8')
    nonempty = untouched = 0
    for i in np.nonzero(kind == 'grid')[0]:
        if length[i] == 0:
            continue
        nonempty += 1
        if nonempty % 3 == 0:
            blob[int(off[i + 1]) - 1] ^= 0x01
            tamper[i] = 'last'
            continue
        untouched += 1
        if untouched % 7 == 0:
            blob[int(off[i])] ^= 0x80
            tamper[i] = 'first'
    fillers = np.nonzero(kind == 'filler')[0]
    isolated = fillers[np.linspace(0, len(fillers) - 1, ISOLATED_PRECHECK + 2).astype(int)[1:-1]]
    for i in list(np.nonzero(kind == 'precheck')[0]) + list(isolated):
        sig[i, 63] |= 0xf0
        tamper[i] = 'precheck'
    want = orc.verify_batch(pk, sig, blob, off)
    return Cases(seeds, pk, sig, blob, off, want, clean_blob, clean_sig, length, align, kind, tamper)


def describe(c, rows, limit=8):
    """for assertion messages: the distinct lengths and alignments of `rows` and
    (row, length, alignment, kind, tamper) of the first `limit` of them"""
    rows = [int(i) for i in rows]
    lens, runs = sorted({int(c.length[i]) for i in rows}), []
    for ln in lens:          # lengths as runs a-b
        if runs and ln == runs[-1][1] + 1:
            runs[-1][1] = ln
        else:
            runs.append([ln, ln])
    return {'lengths': ','.join(str(a) if a == b else '{}-{}'.format(a, b) for a, b in runs),
            'alignments': sorted({int(c.align[i]) for i in rows}),
            'first': [(i, int(c.length[i]), int(c.align[i]), str(c.kind[i]), str(c.tamper[i])) for i in rows[:limit]]}


def aligned_slices(c, max_rows=256):
    """[start, end) row ranges of at most max_rows rows that each begin at a
    blob offset = 0 (mod 4): a call on such a slice rebases the offsets to the
    slice and keeps every row's start alignment"""
    n = len(c.length)
    cut = (c.off[:n] % 4 == 0)
    out, s = [], 0
    while s < n:
        e = min(n, s + max_rows)
        while e < n and not cut[e]:
            e -= 1
        assert e > s, 'no aligned cut within {} rows of row {}'.format(max_rows, s)
        out.append((s, e))
        s = e
    return out


def take(c, s, e):
    """pk, sig, blob, off of rows [s, e), offsets rebased to the slice"""
    o = c.off[s:e + 1]
    return c.pk[s:e], c.sig[s:e], c.blob[int(o[0]):int(o[-1])], o - o[0]
