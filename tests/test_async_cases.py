"""The pairs of tests/_async_cases.py meet their condition, and its checker
has teeth (CPU only: the expectations come from the synth spec alone)."""
import numpy as np
import pytest

import _async_cases as ac

PAIR_NAMES = sorted(ac.PAIRS)


@pytest.mark.parametrize('name', PAIR_NAMES)
def test_pairs_differ_in_every_word(name):
    """The condition on the pairs: no common 64-signature word of the two
    expected bitmaps is equal, so no word of the other batch can pass for the
    batch's own.  The two batches also differ in size and in their keys."""
    a, b = ac.PAIRS[name]
    k = ac.common_words(a, b)
    assert k == (b.n + 63) // 64 and b.n < a.n
    assert b.n % 64 != 0                       # B's last word is partial
    eq = ac.equal_words(a, b)
    assert eq.size == 0, 'words {} of {} agree: change a `first`'.format(eq.tolist(), k)
    assert (a.cfg, a.first, a.key_mod, a.n_nodes) != (b.cfg, b.first, b.key_mod, b.n_nodes)
    for p in (a, b):                           # ~5 % tampered (COMMIT: k_b of n_nodes votes): both verdicts occur
        t = ac.expected_tamper(p)
        assert 0.03 < t.mean() < 0.5


def test_generic_pair_recorded_counts():
    """The figures the pair was chosen by: 6,787 verdict positions of the
    common prefix differ, the first at index 6."""
    a, b = ac.PAIRS['generic']
    d = np.flatnonzero(ac.expected_outputs(a).verdict[:b.n] != ac.expected_outputs(b).verdict)
    assert (d.size, int(d[0])) == (6787, 6)


def test_expected_tamper_is_the_spec():
    """expected_tamper against synth.host_batch_ex (the restatement the device
    generator is tested against) on the head of every parameter set."""
    from plenum_gpu import synth
    for p in ac.BATCHES:
        m = 3 * p.n_nodes
        _, msgs, tamper, _ = synth.host_batch_ex(p.mode, p.cfg, p.first, m, p.mlen, p.mlen_max, p.key_mod, p.n_nodes)
        assert (ac.expected_tamper(p)[:m] == tamper).all()
        if p.mode != synth.COMMIT:
            assert all(p.mlen <= len(x) <= p.mlen_max for x in msgs)
    assert ac.SMALL_B.n <= 32768                # plenum_gpu._native.LAT_MAX_DEFAULT


@pytest.mark.parametrize('p', ac.BATCHES, ids=ac.BATCH_NAMES.get)
def test_checker_accepts_own_outputs(p):
    e = ac.expected_outputs(p)
    assert e.verdict.shape == (p.n,) and e.bitmap.shape == ((p.n + 63) // 64,)
    assert ac.check_outputs(e.verdict.copy(), e.bitmap.copy(), e) is None
    assert ac.check_outputs(e.verdict.copy(), e.bitmap.view(np.uint64).copy(), e) is None
    # the unused high bits of a partial last word are expected zero
    if p.n % 64:
        assert (int(e.bitmap[-1]) & 0xffffffffffffffff) >> (p.n % 64) == 0
    bits = np.unpackbits(e.bitmap.view(np.uint8), bitorder='little')[:p.n]
    assert (bits == e.verdict).all() and (e.verdict == ~ac.expected_tamper(p)).all()


@pytest.mark.parametrize('name', PAIR_NAMES)
def test_checker_reports_the_other_batch(name):
    """A's outputs replaced by B's expected ones (as a slot that computed from
    the other slot's state would leave them), whole and word by word."""
    a, b = ac.PAIRS[name]
    ea, eb = ac.expected_outputs(a), ac.expected_outputs(b)
    k = ac.common_words(a, b)
    # everything of B, cut or padded to A's shape
    v = ea.verdict.copy()
    v[:b.n] = eb.verdict
    bm = ea.bitmap.copy()
    bm[:k] = eb.bitmap
    d = ac.check_outputs(v, bm, ea)
    first = int(np.flatnonzero(ea.verdict[:b.n] != eb.verdict)[0])
    assert d == ('verdict', first, int(eb.verdict[first]), int(ea.verdict[first]))
    assert ac.check_outputs(v, ea.bitmap, ea)[:2] == ('verdict', first)
    assert ac.check_outputs(ea.verdict, bm, ea)[:2] == ('bitmap', 0)
    # B's outputs in B's own shape
    assert ac.check_outputs(eb.verdict, eb.bitmap, ea) == ('verdict', 'len', eb.verdict.shape, ea.verdict.shape)
    # any single word of A replaced by B's word at the same position
    for w in range(k):
        bm = ea.bitmap.copy()
        bm[w] = eb.bitmap[w]
        assert ac.check_outputs(ea.verdict, bm, ea) == ('bitmap', w, int(eb.bitmap[w]), int(ea.bitmap[w])), w
    # ... and any 64 verdicts of A by B's
    for w in range(k):
        v = ea.verdict.copy()
        hi = min(64 * w + 64, b.n)
        v[64 * w:hi] = eb.verdict[64 * w:hi]
        d = ac.check_outputs(v, ea.bitmap, ea)
        assert d is not None and d[0] == 'verdict' and 64 * w <= d[1] < hi, w


@pytest.mark.parametrize('p', ac.BATCHES, ids=ac.BATCH_NAMES.get)
def test_checker_reports_the_sentinel(p):
    """Outputs a schedule never wrote: the fill is still there."""
    e = ac.expected_outputs(p)
    v7 = np.full(p.n, ac.SENTINEL_VERDICT, np.uint8)
    bm1 = np.full((p.n + 63) // 64, ac.SENTINEL_WORD, np.int64)
    assert ac.check_outputs(v7, bm1, e) == ('verdict', 0, 7, int(e.verdict[0]))
    assert ac.check_outputs(v7, e.bitmap, e) == ('verdict', 0, 7, int(e.verdict[0]))
    # no expected word is all ones up to the unused bits' zeros ... unless no
    # signature of the word is tampered: then the first word that has one
    d = ac.check_outputs(e.verdict, bm1, e)
    first = int(np.flatnonzero(e.bitmap != -1)[0])
    assert d == ('bitmap', first, -1, int(e.bitmap[first]))
    # one verdict byte, one bitmap word left unwritten anywhere
    rng = np.random.default_rng(5)
    for i in rng.choice(p.n, 50, replace=False):
        v = e.verdict.copy()
        v[i] = ac.SENTINEL_VERDICT
        assert ac.check_outputs(v, e.bitmap, e) == ('verdict', int(i), 7, int(e.verdict[i]))
    # the last (partial) word left unwritten is seen even when every
    # signature of it is accepted: its unused bits are expected zero
    if p.n % 64:
        bm = e.bitmap.copy()
        bm[-1] = ac.SENTINEL_WORD
        assert ac.check_outputs(e.verdict, bm, e)[:3] == ('bitmap', len(bm) - 1, -1)
