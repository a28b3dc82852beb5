"""The hash-route grid (_hram_cases.py) on the CPU: the grid is what it claims
to be, the oracle agrees with hashlib on every row of it, and the host build
of the kernel source (tools/hostcheck) gives the oracle's verdicts and
signatures on it.  The GPU routes run the same grid in test_gpu_hram_edges.py."""
import ctypes
import hashlib

import numpy as np
import pytest

import _hram_cases as hcs
import _oracle as orc
from test_hostcheck import _load, _p, hc_verify

L = 2 ** 252 + 27742317777372353535851937790883648493


@pytest.fixture(scope='module')
def grid():
    return hcs.build()


@pytest.fixture(scope='module')
def thin():
    """the grid thinned for the slow host-build entries: every edge length at
    all four alignments, lengths 0..199 at alignment 0 (a batch of its own, so
    every row starts at the alignment it is listed with)"""
    return hcs.build(hcs.THIN_PAIRS)


@pytest.fixture(scope='module')
def hc():
    return _load()


def _msg(c, i, blob=None):
    b = c.blob if blob is None else blob
    return b[int(c.off[i]):int(c.off[i + 1])].tobytes()


def test_lengths_and_alignments_present_once(grid, thin):
    c = grid
    assert len(hcs.LENGTHS) == 315
    g = c.kind == 'grid'
    pairs = list(zip(c.length[g].tolist(), c.align[g].tolist()))
    assert len(pairs) == len(set(pairs)) == 4 * len(hcs.LENGTHS)
    assert set(pairs) == set(hcs.FULL_PAIRS)
    # the recorded alignment is the row's start offset in the blob
    assert (c.align == (c.off[:-1] % 4).astype(np.int64)).all()
    assert (c.length == (c.off[1:] - c.off[:-1]).astype(np.int64)).all()
    for a in range(4):
        assert int((c.align[g] == a).sum()) == len(hcs.LENGTHS)
    f = c.kind == 'filler'
    assert ((c.length[f] >= 1) & (c.length[f] <= 3)).all()
    assert int((c.kind == 'precheck').sum()) == hcs.PRECHECK_RUN and (c.kind[:hcs.PRECHECK_RUN] == 'precheck').all()
    # keys repeat: the whole seed pool, each seed many times
    assert len(np.unique(c.pk, axis=0)) == hcs.N_SEEDS
    # the thinned grid keeps every edge length at all four alignments
    tg = thin.kind == 'grid'
    tp = set(zip(thin.length[tg].tolist(), thin.align[tg].tolist()))
    assert tp == set(hcs.THIN_PAIRS)
    assert {(ln, a) for ln in hcs.edge_lengths() | set(hcs.SPECIAL) for a in range(4)} <= tp
    assert {(ln, 0) for ln in range(200)} <= tp
    assert (thin.align == (thin.off[:-1] % 4).astype(np.int64)).all()


def test_block_count_steps_present(grid):
    """for each block count 1..7 of R || A || M (and of the signer's 32-byte-prefix
    hash) the last length with that count and the first with the next are there
    at all four alignments"""
    have = set(zip(grid.length[grid.kind == 'grid'].tolist(), grid.align[grid.kind == 'grid'].tolist()))
    for k in range(1, 8):
        last = 128 * k - 81
        assert hcs.hram_blocks(last) == k and hcs.hram_blocks(last + 1) == k + 1
        last32 = 128 * k - 49
        assert (32 + last32 + 17 + 127) // 128 == k and (32 + last32 + 1 + 17 + 127) // 128 == k + 1
        for ln in (last, last + 1, last32, last32 + 1, 128 * k - 64, 128 * k - 32):
            for a in range(4):
                assert (ln, a) in have, (k, ln, a)


def test_oracle_accepts_untampered_and_rejects_exactly_tampered(grid):
    c = grid
    assert orc.verify_batch(c.pk, c.clean_sig, c.clean_blob, c.off).all()
    assert ((c.tamper != '') == ~c.want).all(), hcs.describe(c, np.nonzero((c.tamper != '') == c.want)[0])
    assert c.want.any() and (~c.want).any()
    for t in ('last', 'first', 'precheck'):
        assert (c.tamper == t).any()
    # the rule: every third non-empty grid row 'last', every seventh of the rest 'first'
    ne = np.nonzero((c.kind == 'grid') & (c.length > 0))[0]
    assert (c.tamper[ne[2::3]] == 'last').all() and int((c.tamper == 'last').sum()) == len(ne) // 3
    rest = ne[c.tamper[ne] != 'last']
    assert (c.tamper[rest[6::7]] == 'first').all() and int((c.tamper == 'first').sum()) == len(rest) // 7
    assert int((c.tamper == 'precheck').sum()) == hcs.PRECHECK_RUN + hcs.ISOLATED_PRECHECK
    assert (c.sig[c.tamper == 'precheck', 63] >= 0xf0).all()
    # nothing but the listed bytes differs from the signed batch
    assert int((c.blob != c.clean_blob).sum()) == int(((c.tamper == 'last') | (c.tamper == 'first')).sum())
    assert int((c.sig != c.clean_sig).any(axis=1).sum()) == int((c.tamper == 'precheck').sum())


def test_oracle_hram_vs_hashlib_every_row(grid):
    """ties the checker to an independent SHA-512 at exactly these lengths"""
    c = grid
    bad = []
    for i in range(len(c.length)):
        sig, pk, m = c.sig[i].tobytes(), c.pk[i].tobytes(), _msg(c, i)
        want = int.from_bytes(hashlib.sha512(sig[:32] + pk + m).digest(), 'little') % L
        if int.from_bytes(orc.hram(sig, pk, m), 'little') != want:
            bad.append(i)
    assert not bad, hcs.describe(c, bad)


def test_host_build_verify_batch(hc, grid):
    """hc_verify_batch (hash_one + the curve stage as the kernels run them) on every row"""
    c = grid
    got = hc_verify(hc, c.pk, c.sig, c.blob, c.off)
    wrong = np.nonzero(got != c.want)[0]
    assert len(wrong) == 0, ('hc_verify_batch', len(wrong), hcs.describe(c, wrong))


def _keyed_quad(hc, c, small):
    upk, kidx = np.unique(c.pk, axis=0, return_inverse=True)
    kidx = np.ascontiguousarray(kidx.reshape(-1), np.uint32)
    upk = np.ascontiguousarray(upk, np.uint8)
    n = len(c.pk)
    v = np.zeros(n, np.uint8)
    b = orc.padded(c.blob)
    assert b.ctypes.data % 4 == 0       # the listed alignments are the addresses the code sees
    fn = hc.hc_verify_keyed_quad_small if small else hc.hc_verify_keyed_quad
    fn(_p(upk), ctypes.c_uint64(len(upk)), _p(kidx), _p(np.ascontiguousarray(c.sig)), _p(b),
       _p(np.ascontiguousarray(c.off)), ctypes.c_uint64(n), _p(v))
    return v.astype(bool)


@pytest.mark.parametrize('small', [False, True], ids=['4sides', '8sides'])
def test_host_build_keyed_quad(hc, thin, small):
    """hc_verify_keyed_quad / _small (keyed_sched_block + keyed_hash: schedules
    of the first KQ_SCHED_BLOCKS blocks ahead, hram_block beyond) on the thinned grid"""
    c = thin
    got = _keyed_quad(hc, c, small)
    wrong = np.nonzero(got != c.want)[0]
    assert len(wrong) == 0, ('keyed_quad', small, len(wrong), hcs.describe(c, wrong))


def test_host_build_sign_batch(hc, thin):
    """hc_sign_batch (sha512_prefixed / msg_bytes8: both hashes of the signer)
    equals the oracle's keys and signatures byte for byte on the thinned grid"""
    c = thin
    n = len(c.pk)
    b = orc.padded(c.clean_blob)
    assert b.ctypes.data % 4 == 0
    pk = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    hc.hc_sign_batch(_p(c.seeds), _p(b), _p(np.ascontiguousarray(c.off)), ctypes.c_uint64(n), _p(pk), _p(sig))
    wrong = np.nonzero((pk != c.pk).any(axis=1) | (sig != c.clean_sig).any(axis=1))[0]
    assert len(wrong) == 0, ('hc_sign_batch', len(wrong), hcs.describe(c, wrong))
