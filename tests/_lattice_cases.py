"""Case families of the Lehmer-round lattice reduction (csrc/pv_lattice.h
hs_euclid_lehmer), shared by tests/test_lattice_lehmer.py (host build) and
tests/test_gpu_lattice_lehmer.py (device kernels).

A family is a list of h < L built, as _devcheck_cases.lattice_h() builds its
planted cases, from a chosen continued fraction of 8L / h.  Where a family is
named after a place in a round, the place is read from the host build's own
round record (hc_lattice_rounds) of the UNPLANTED h, and the planted quotient
replaces the one at that step.  Quotients stop at 2^32 - 7, below the window
[2^32 - 6, 2^32 + 1] in which host and device may defer differently
(tests/test_gpu_devcheck.py)."""
import ctypes
import functools
import random

import _devcheck_cases as D

PLANT_E = (2 ** 16, 2 ** 31, 2 ** 32 - 7)
PLACES = ('first', 'middle', 'last')


def hc():
    return D.host_libs()[0]


def rounds(h):
    """(status, stats5, ks): hc_lattice_rounds of h; ks = proven steps per round in order, 0 = a fallback step"""
    s = (ctypes.c_uint32 * 5)()
    ks = (ctypes.c_uint8 * 193)()
    st = hc().hc_lattice_rounds(h.to_bytes(32, 'little'), s, ks)
    return st, list(s), list(ks[:s[0]])


def h_of(qs):
    """h with 8L / h = [qs[0]; qs[1], ...] up to rounding: its first quotients are qs"""
    h = int(D.L8 / D.cf_value(qs))
    assert 0 < h < D.L, qs[:4]
    return h


def _base(seed, n=75):
    r = random.Random(7100 + seed)
    return [8 + seed] + [r.randrange(1, 10) for _ in range(n)]


def round_spans(ks):
    """[(first step, steps)] of the rounds that proved at least three steps"""
    out, at = [], 0
    for k in ks:
        if k >= 3:
            out.append((at, k))
        at += max(k, 1)
    return out


@functools.lru_cache(None)
def planted_in_round():
    """[(e, place, h)]: e at the first / middle / last step of the second and the third round of four base h"""
    out = []
    for seed in range(4):
        qs = _base(seed)
        spans = round_spans(rounds(h_of(qs))[2])
        assert len(spans) >= 4, spans
        for start, k in (spans[1], spans[2]):
            for place, pos in zip(PLACES, (start, start + k // 2, start + k - 1)):
                for e in PLANT_E:
                    p = qs[:pos] + [e] + qs[pos + 1:]
                    h = h_of(p)
                    assert D.euclid_quotients(h)[pos] == e, (seed, pos, e)
                    out.append((e, place, h))
    return tuple(out)


@functools.lru_cache(None)
def ones():
    """60 consecutive quotients of 1, from the second step, the tenth and the thirtieth"""
    out = []
    for seed, lead in enumerate((1, 9, 29)):
        qs = _base(seed)[:lead] + [1] * 60 + _base(seed + 10)
        h = h_of(qs)
        assert D.euclid_quotients(h)[lead:lead + 60] == [1] * 60
        out.append(h)
    return tuple(out)


@functools.lru_cache(None)
def close_leading_words():
    """at the first step of a round the two remainders agree in their leading 60 bits and more: quotients 1 and
    then about 2^61, so nothing of that round can be proven (and the big quotient defers, on both forms)"""
    out = []
    for seed in range(4):
        qs = _base(seed)
        spans = round_spans(rounds(h_of(qs))[2])
        for start, _ in spans[1:3]:
            p = qs[:start] + [1, 2 ** 61 + 12345] + qs[start + 2:]
            h = h_of(p)
            q = D.euclid_quotients(h)
            assert q[start] == 1 and q[start + 1] >> 60 >= 2, (seed, start)
            out.append(h)
    return tuple(out)


@functools.lru_cache(None)
def exits():
    """(full, cut, twice): by construction every exit is a fallback step.  full: random h whose exit step
    follows a round of 15 steps or more (one that ran to its cofactor cap: the exit is the step right after a
    round boundary); cut: h whose last round proved one or two steps (the exit margin ended it: the exit
    would have been inside that round); twice: a quotient of 2^31 + 5 planted so that the step before the
    exit is a fallback step too"""
    rnd = random.Random(7300)
    full, cut, twice = [], [], []
    for _ in range(20000):
        if len(full) == 4 and len(cut) == 4:
            break
        h = rnd.randrange(D.L)
        st, s, ks = rounds(h)
        if len(ks) >= 3 and ks[-1] == 0 and s[4] == 1:
            if ks[-2] >= 15 and len(full) < 4:
                full.append(h)
            if 1 <= ks[-2] <= 2 and len(cut) < 4:
                cut.append(h)
    assert len(full) == 4 and len(cut) == 4
    for seed in range(8):
        qs = _base(seed)
        n = len(D.euclid_quotients(h_of(qs)))
        for pos in range(n - 1, n - 30, -1):
            h = h_of(qs[:pos] + [2 ** 31 + 5] + qs[pos + 1:])
            q = D.euclid_quotients(h)
            st, s, ks = rounds(h)
            if len(q) == pos + 2 and ks[-2:] == [0, 0] and s[4] == 1:
                twice.append(h)
                break
    assert len(twice) >= 2, len(twice)
    return tuple(full), tuple(cut), tuple(twice)


@functools.lru_cache(None)
def small():
    """h < 2^128 (no step at all), the edge included"""
    rnd = random.Random(7400)
    return (0, 1, 2, 2 ** 64, 2 ** 127, 2 ** 128 - 1) + tuple(rnd.randrange(2 ** 128) for _ in range(10))


@functools.lru_cache(None)
def longest():
    """an h of exactly 98 steps, the most a wave's slowest lane was seen to take among random h
    (tools/lattice_sim.py): a run of quotients 1, as long as it takes, in front of a random tail"""
    for n in range(80):
        h = h_of([8] + [1] * n + _base(3))
        if len(D.euclid_quotients(h)) == 98:
            return h
    raise AssertionError('no 98-step h')


@functools.lru_cache(None)
def families():
    """{name: tuple of h}; not disjoint"""
    full, cut, twice = exits()
    f = {
        'planted first': tuple(h for _, p, h in planted_in_round() if p == 'first'),
        'planted middle': tuple(h for _, p, h in planted_in_round() if p == 'middle'),
        'planted last': tuple(h for _, p, h in planted_in_round() if p == 'last'),
        'ones': ones(),
        'close leading words': close_leading_words(),
        'exit after a full round': full,
        'exit after a cut round': cut,
        'exit after a fallback step': twice,
        'small': small(),
        'L - 1': (D.L - 1,),
    }
    for name, hs in f.items():
        assert hs and all(0 <= h < D.L for h in hs), name
        assert not any(D.near_2_32(h) for h in hs), name
    return f


@functools.lru_cache(None)
def planted_all():
    out = []
    for hs in families().values():
        out += hs
    return tuple(out)


@functools.lru_cache(None)
def random_h(n, seed=7600):
    rnd = random.Random(seed)
    return tuple(rnd.randrange(D.L) for _ in range(n))


# ------------------------------------------------ Python-integer restatement
def _f64(x):
    """pv_lattice.h words_to_f64: Horner over the eight words, one rounding per word"""
    v = float((x >> 224) & 0xffffffff)
    for k in range(6, -1, -1):
        v = v * 4294967296.0 + float((x >> (32 * k)) & 0xffffffff)
    return v


def _fits(v):
    return v + D.PAT33 < 2 ** 132


def py_half_scalars(h):
    """(status, |c|, d, c_neg) by Euclid over Python integers and half_scalars' selection rule; None where a
    quotient inside or above the near-2^32 window makes the deferral the float estimate's business"""
    import math
    a, b, ta, tb, odd, steps = D.L8, h, 0, 1, 1, 0
    while b >= 2 ** 128:
        if steps >= 192:
            return D.HS_DEFER, 0, 0, 0
        q = a // b
        if q > D.NEAR_HI:
            return D.HS_DEFER, 0, 0, 0
        if q >= D.NEAR_LO:
            return None
        a, b, ta, tb = b, a - q * b, tb, ta + q * tb
        odd ^= 1
        steps += 1
    if tb & 1:
        return D.HS_HALF, b, tb, int(odd == 0)
    if not _fits(a):
        if b == 0:
            return D.HS_DEFER, 0, 0, 0
        kd = math.ceil((_f64(a) - 2.5e39) / _f64(b))
        if not kd < 4294967294.0:
            return D.HS_DEFER, 0, 0, 0
        k = int(kd) if kd > 0 else 0
        a -= k * b
        if a < 0:
            return D.HS_DEFER, 0, 0, 0
        ta += k * tb
        if not _fits(a):
            a -= b
            ta += tb
        if not _fits(a):
            return D.HS_DEFER, 0, 0, 0
    if not _fits(ta):
        return D.HS_DEFER, 0, 0, 0
    return D.HS_HALF, a, ta, int(odd == 1)
