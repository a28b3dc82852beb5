"""Case generators and Python-integer references of the device check
(tools/devcheck): every op of dc_ops_pv.h / dc_ops_bn.h gets a seeded,
deterministic list of operands INSIDE the contract its header documents (the
generators assert that) and a reference over Python integers.  Shared by
tests/test_devcheck_cases.py (host twins, CPU) and tests/test_gpu_devcheck.py
(device kernels).

cases()[op] is a uint32 array (n, IW): one packed case per row, the layout the
op bodies read.  check(op, inp, out) asserts the reference on the rows of out.
Everything is exact integer arithmetic; there is no tolerance."""
import ctypes
import functools
import os
import random
import subprocess
from fractions import Fraction

import numpy as np

from _bn_madchain_ref import G as BNG, NL, REPO, ref_mul

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
L8 = 8 * L
PAT33 = int('8' * 33, 16)
HS_MAX = 2 ** 132 - PAT33            # |c|, d < HS_MAX (pv_lattice.h fits132)
HS_NONE, HS_HALF, HS_DEFER = 0, 1, 2
SHIFT = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
WIDTH = [26, 25] * 5

# (words in, words out) per op, as in dc_ops_pv.h / dc_ops_bn.h
LANE_OPS = {
    'fe_mul': (20, 10), 'fe_sq': (10, 10), 'fe_sq2x': (10, 10), 'fe_mul2': (40, 20), 'fe_mul3': (60, 30),
    'fe_sq2': (20, 20), 'fe_mul_l': (20, 10), 'fe_sq_l': (10, 10), 'fe_sq2x_l': (10, 10), 'fe_sqn': (11, 10),
    'fe_invert': (10, 10), 'fe_pow22523': (10, 10), 'fe_carry': (10, 10), 'fe_carry_even': (10, 10),
    'fe_sub': (20, 10), 'fe_sub4': (20, 10), 'fe_neg': (10, 10), 'fe_frombytes_w': (8, 10),
    'fe_tobytes_w': (10, 8), 'fe_iszero': (10, 1), 'fe_isnegative': (10, 1), 'sc_reduce64': (16, 8),
    'sc_muladd': (24, 8), 'sc_mul_small': (13, 8), 'half_scalars': (8, 12), 'lattice_one': (33, 21),
}
BN_OPS = {
    'bn_mul': (20, 10), 'bn_sqr': (10, 10), 'bn_norm': (10, 10), 'bn_reduce': (10, 10), 'bn_canon': (10, 10),
    'bn_add_mul': (30, 10), 'bn_sub_mul': (30, 10), 'bn_f2mul': (40, 20), 'bn_f2sqr': (20, 20),
}
QUAD_OPS = {'q_dbl': (40, 40), 'q_to_cached': (40, 40), 'q_add': (81, 40), 'q_sum_is_identity': (80, 4)}
ALL_OPS = dict(LANE_OPS, **BN_OPS, **QUAD_OPS)
# batch sizes every op is also cut to (quads: whole quads)
LANE_CUTS = (1, 63, 64, 65, 257)
QUAD_CUTS = (1, 15, 16, 17)


# ---------------------------------------------------------------- field
def fe_value(limbs):
    return sum(int(v) << s for v, s in zip(limbs, SHIFT))


def fe_limbs(x):
    """reduced limbs of 0 <= x < 2^255"""
    assert 0 <= x < 2 ** 255
    return [(x >> s) & ((1 << w) - 1) for s, w in zip(SHIFT, WIDTH)]


def _fl(x10):
    """floor(2^(x10 / 10)), exactly: the largest n with n^10 <= 2^x10"""
    n = int(2 ** (x10 / 10))
    while (n + 1) ** 10 <= 2 ** x10:
        n += 1
    while n ** 10 > 2 ** x10:
        n -= 1
    return n


TIGHT_E, TIGHT_O = 2 ** 26 + 2 ** 10, 2 ** 25 + 2 ** 18
LOOSE_E, LOOSE_O = _fl(277), _fl(267)
WIDE_E = _fl(283)                      # fe_mul's f against a LOOSE g (pv_field.h header)
P_LIMBS = fe_limbs(P)
P4_LIMBS = [4 * v for v in P_LIMBS]     # fe_sub4's largest subtrahend that cannot underflow: 4p limb for limb
M31 = 2 ** 31 - 1


def is_tight(v):
    return all(x <= (TIGHT_O if i & 1 else TIGHT_E) for i, x in enumerate(v))


def is_loose(v):
    return all(x <= (LOOSE_O if i & 1 else LOOSE_E) for i, x in enumerate(v))


def tight_out(v):
    """TIGHT, the bound pv_field.h states for the outputs of mul / sq / carry"""
    return is_tight(v)


# the exactness conditions of tools/hostcheck/hostcheck.cpp, restated
def check_mul(f, g):
    ok = all(2 * f[i] < 2 ** 32 for i in range(1, 10, 2)) and all(19 * g[j] < 2 ** 32 for j in range(1, 10))
    for k in range(10):
        s = 1 << 39
        for i in range(10):
            j = (k - i + 10) % 10
            t = f[i] * g[j]
            if (i & 1) and (j & 1):
                t *= 2
            if i + j >= 10:
                t *= 19
            s += t
        ok = ok and s < 2 ** 64
    return ok


def check_sq(f):
    return (all(2 * f[i] < 2 ** 32 for i in range(8)) and all(19 * f[j] < 2 ** 32 for j in (6, 8))
            and all(38 * f[j] < 2 ** 32 for j in (5, 7, 9)) and check_mul(f, f))


def check_sq2x(f):
    ok = (all(2 * f[i] < 2 ** 32 for i in range(8)) and all(4 * f[i] < 2 ** 32 for i in (0, 1, 3))
          and all(38 * f[j] < 2 ** 32 for j in (6, 8)) and all(76 * f[j] < 2 ** 32 for j in (5, 7, 9)))
    for k in range(10):
        s = 1 << 39
        for i in range(10):
            j = (k - i + 10) % 10
            t = 2 * f[i] * f[j]
            if (i & 1) and (j & 1):
                t *= 2
            if i + j >= 10:
                t *= 19
            s += t
        ok = ok and s < 2 ** 64
    return ok


def _maxvec(e, o):
    return [o if i & 1 else e for i in range(10)]


@functools.lru_cache(None)
def field_pool():
    """(specials, random TIGHT, random LOOSE): limb vectors, values sum(limb_i << ceil(25.5 i))"""
    rnd = random.Random(2551)
    sp = []
    for k in (1, 2, 3, 4, 6):
        kp = [k * v for v in P_LIMBS]
        sp += [kp, [kp[0] + 1] + kp[1:], [kp[0] - 1] + kp[1:]]
    sp += [fe_limbs(2 ** 255 - 1), [P_LIMBS[0] + 18] + P_LIMBS[1:], [0] * 10, [1] + [0] * 9]
    for e, o in ((TIGHT_E, TIGHT_O), (LOOSE_E, LOOSE_O)):
        m = _maxvec(e, o)
        sp.append(m)
        sp += [[m[i] if i == j else 0 for i in range(10)] for j in range(10)]
        sp += [[m[i] if (i & 1) == ph else 0 for i in range(10)] for ph in (0, 1)]
    rt = [[rnd.randrange((TIGHT_O if i & 1 else TIGHT_E) + 1) for i in range(10)] for _ in range(300)]
    rl = [[rnd.randrange((LOOSE_O if i & 1 else LOOSE_E) + 1) for i in range(10)] for _ in range(300)]
    return sp, rt, rl


def _rows(rows, width):
    a = np.array(rows, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == width and (a < 2 ** 32).all()
    return np.ascontiguousarray(a.astype(np.uint32))


def _field_cases():
    sp, rt, rl = field_pool()
    pool = sp + rt + rl
    loose = [v for v in pool if is_loose(v)]
    tight = [v for v in pool if is_tight(v)]
    sp_loose = [v for v in sp if is_loose(v)]
    rnd = random.Random(77)
    # multiplies: special x special, every vector against a stride partner, and the
    # wide-f pairs (even limbs at floor(2^28.3), against the LOOSE maximum and LOOSE randoms)
    pairs = [(a, b) for a in sp_loose for b in sp_loose]
    pairs += [(loose[i], loose[(7 * i + 3) % len(loose)]) for i in range(len(loose))]
    gmax = _maxvec(LOOSE_E, LOOSE_O)
    wide = [[WIDE_E if not i & 1 else LOOSE_O for i in range(10)],
            [WIDE_E if not i & 1 else TIGHT_O for i in range(10)],
            [WIDE_E if not i & 1 else 0 for i in range(10)]]
    wide += [[rnd.randrange(WIDE_E + 1) if not i & 1 else rnd.randrange(LOOSE_O + 1) for i in range(10)]
             for _ in range(40)]
    pairs += [(f, gmax) for f in wide] + [(f, rl[i]) for i, f in enumerate(wide)]
    assert all(check_mul(f, g) for f, g in pairs)
    assert all(check_sq(f) for f in loose) and all(check_sq2x(f) for f in tight)
    n = len(pairs)
    c = {}
    c['fe_mul'] = c['fe_mul_l'] = _rows([f + g for f, g in pairs], 20)
    c['fe_mul2'] = _rows([sum(pairs[i], []) + sum(pairs[(5 * i + 1) % n], []) for i in range(n)], 40)
    c['fe_mul3'] = _rows([sum(pairs[i], []) + sum(pairs[(5 * i + 1) % n], []) + sum(pairs[(11 * i + 2) % n], [])
                          for i in range(n)], 60)
    c['fe_sq'] = c['fe_sq_l'] = c['fe_invert'] = c['fe_pow22523'] = _rows(loose, 10)
    c['fe_sq2'] = _rows([loose[i] + loose[(3 * i + 1) % len(loose)] for i in range(len(loose))], 20)
    c['fe_sq2x'] = c['fe_sq2x_l'] = _rows(tight, 10)
    c['fe_sqn'] = _rows([f + [k] for k in (1, 2, 5, 50) for f in loose], 11)
    # carries and encodings: additionally limbs up to 2^31 - 1
    big = [[M31] * 10, [0] * 9 + [M31]] + [[rnd.randrange(M31 + 1) for _ in range(10)] for _ in range(300)]
    c['fe_carry'] = c['fe_tobytes_w'] = c['fe_iszero'] = c['fe_isnegative'] = _rows(pool + big, 10)
    # fe_carry_even: even limbs <= 2^28.6, odd <= 2^27.6 (its header comment)
    ce, co = _fl(286), _fl(276)
    ev = [_maxvec(ce, co)] + [[rnd.randrange((co if i & 1 else ce) + 1) for i in range(10)] for _ in range(300)]
    assert all(x <= (co if i & 1 else ce) for v in pool for i, x in enumerate(v))
    c['fe_carry_even'] = _rows(pool + ev, 10)
    # subtractions: f LOOSE; g TIGHT (fe_sub, fe_neg) or up to the limbs of 4p (fe_sub4: 2^28 / 2^27)
    c['fe_sub'] = _rows([loose[i] + tight[(5 * i + 2) % len(tight)] for i in range(len(loose))]
                        + [a + b for a in sp_loose for b in sp if is_tight(b)], 20)
    c['fe_neg'] = _rows(tight, 10)
    g4 = [v for v in pool if all(x <= m for x, m in zip(v, P4_LIMBS))]
    g4 += [P4_LIMBS] + [[rnd.randrange(m + 1) for m in P4_LIMBS] for _ in range(300)]
    c['fe_sub4'] = _rows([loose[i % len(loose)] + g for i, g in enumerate(g4)]
                         + [a + P4_LIMBS for a in sp_loose], 20)
    vals = [P - 1, P, P + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1, 0, 1, 2 ** 255 + 19, 2 ** 255 + P]
    vals += [rnd.randrange(2 ** 256) for _ in range(300)]
    c['fe_frombytes_w'] = _rows([words(v, 8) for v in vals], 8)
    return c


def words(x, n):
    assert 0 <= x < 2 ** (32 * n)
    return [(x >> (32 * k)) & 0xffffffff for k in range(n)]


def unwords(w):
    return sum(int(v) << (32 * k) for k, v in enumerate(w))


def _fes(row, n):
    return [[int(x) for x in row[10 * j:10 * j + 10]] for j in range(n)]


def _check_field(op, inp, out):
    for r, (i, o) in enumerate(zip(inp, out)):
        what = '{} case {}'.format(op, r)
        if op in ('fe_mul', 'fe_mul_l', 'fe_mul2', 'fe_mul3'):
            n = len(o) // 10
            f, h = _fes(i, 2 * n), _fes(o, n)
            for k in range(n):
                assert fe_value(h[k]) % P == fe_value(f[2 * k]) * fe_value(f[2 * k + 1]) % P, what
                assert tight_out(h[k]), what
        elif op in ('fe_sq', 'fe_sq_l', 'fe_sq2', 'fe_sq2x', 'fe_sq2x_l'):
            n = len(o) // 10
            f, h = _fes(i, n), _fes(o, n)
            m = 2 if 'sq2x' in op else 1
            for k in range(n):
                assert fe_value(h[k]) % P == m * fe_value(f[k]) ** 2 % P, what
                assert tight_out(h[k]), what
        elif op in ('fe_sqn', 'fe_invert', 'fe_pow22523'):
            f, h = fe_value(_fes(i, 1)[0]), _fes(o, 1)[0]
            e = 2 ** int(i[10]) if op == 'fe_sqn' else (P - 2 if op == 'fe_invert' else (P - 5) // 8)
            assert fe_value(h) % P == pow(f, e, P), what
            assert tight_out(h), what
        elif op == 'fe_carry':
            f, h = _fes(i, 1)[0], _fes(o, 1)[0]
            assert fe_value(h) % P == fe_value(f) % P, what
            assert tight_out(h), (what, h)
        elif op == 'fe_carry_even':
            f, h = _fes(i, 1)[0], _fes(o, 1)[0]
            assert fe_value(h) == fe_value(f), what          # no wrap: the same integer
            assert all(h[k] < 2 ** 26 for k in range(0, 10, 2)), what
            assert all(h[k] == f[k] + (f[k - 1] >> 26) for k in range(1, 10, 2)), what
        elif op in ('fe_sub', 'fe_sub4'):
            f, g = _fes(i, 2)
            h = _fes(o, 1)[0]
            assert fe_value(h) % P == (fe_value(f) - fe_value(g)) % P, what
            k = 2 if op == 'fe_sub' else 4
            assert all(h[t] == f[t] + k * P_LIMBS[t] - g[t] for t in range(10)), what
        elif op == 'fe_neg':
            f, h = _fes(i, 1)[0], _fes(o, 1)[0]
            assert fe_value(h) % P == -fe_value(f) % P, what
            assert is_loose(h), what
        elif op == 'fe_frombytes_w':
            h = _fes(o, 1)[0]
            assert h == fe_limbs(unwords(i) % 2 ** 255), what     # bit 255 dropped, reduced limbs
        elif op == 'fe_tobytes_w':
            assert unwords(o) == fe_value(_fes(i, 1)[0]) % P, what   # canonical
        elif op == 'fe_iszero':
            assert int(o[0]) == (1 if fe_value(_fes(i, 1)[0]) % P == 0 else 0), what
        elif op == 'fe_isnegative':
            assert int(o[0]) == (fe_value(_fes(i, 1)[0]) % P) & 1, what
        else:
            raise KeyError(op)


# ------------------------------------------------------- scalars, lattice
def cf_value(qs):
    """[qs[0]; qs[1], ...] as a Fraction"""
    x = Fraction(qs[-1])
    for q in reversed(qs[:-1]):
        x = q + 1 / x
    return x


def euclid_quotients(h):
    """the partial quotients half_scalars' Euclid on (8L, h) takes: one per step
    while the divisor is >= 2^128"""
    a, b, qs = L8, h, []
    while b >= 2 ** 128:
        q, r = divmod(a, b)
        qs.append(q)
        a, b = b, r
    return qs


PLANT_E = (1, 2, 3, 2 ** 16, 2 ** 31, 2 ** 32 - 5, 2 ** 32 - 4, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32,
           2 ** 32 + 1, 2 ** 40)
PLANT_POS = (1, 2, 3, 5, 20)
NEAR_LO, NEAR_HI = 2 ** 32 - 6, 2 ** 32 + 1     # the documented host/device exception's window
H_FIXED = (0, 1, 2, 3, 5, 8, 2 ** 127, 2 ** 128 - 1, 2 ** 128, 2 ** 128 + 1, 2 ** 131, HS_MAX - 1, L // 3, L // 2,
           L - 2, L - 1)


@functools.lru_cache(None)
def lattice_h():
    """[(kind, h, e)]: kind 'fixed' / 'random' / 'planted' (e = the planted quotient)"""
    assert HS_MAX == int('7' * 32 + '8', 16)
    out = [('fixed', h, None) for h in H_FIXED]
    rnd = random.Random(4000)
    out += [('random', rnd.randrange(L), None) for _ in range(4000)]
    first = (8, 9, 13, 100)
    for pos in PLANT_POS:
        for seed in range(4):
            for e in PLANT_E:
                r = random.Random(1000 * pos + 10 * seed + 1)
                qs = [first[seed]] + [r.randrange(1, 7) for _ in range(pos - 1)] + [e]
                qs += [r.randrange(1, 10) for _ in range(70)]
                h = int(L8 / cf_value(qs))
                assert 0 < h < L and euclid_quotients(h)[pos] == e, (pos, seed, e)
                out.append(('planted', h, e))
    # the same quotients first (pos = 0); h < L needs a first quotient >= 8, so e in {1, 2, 3} has no such h
    for seed in range(4):
        for e in PLANT_E:
            if e < 8:
                continue
            r = random.Random(9000 + seed)
            qs = [e] + [r.randrange(1, 10) for _ in range(70)]
            h = int(L8 / cf_value(qs))
            assert 0 < h < L and euclid_quotients(h)[0] == e, (seed, e)
            out.append(('planted', h, e))
    return tuple(out)


def near_2_32(h):
    """the exception's scope: a partial quotient in [2^32 - 6, 2^32 + 1] on the way"""
    return any(NEAR_LO <= q <= NEAR_HI for q in euclid_quotients(h))


def _scalar_cases():
    rnd = random.Random(99)
    c = {}
    xs = [0, 1, L - 1, L, L + 1, 2 * L, 2 ** 512 - 1, 2 ** 256, (2 ** 252) * L, 2 ** 512 - L, (2 ** 259) * L - 1]
    xs += [rnd.randrange(2 ** 512) for _ in range(300)] + [rnd.randrange(2 ** 253) for _ in range(50)]
    c['sc_reduce64'] = _rows([words(x, 16) for x in xs], 16)
    edge = [0, 1, L - 1, L, 2 ** 256 - 1, 2 ** 255]
    tr = [(a, b, cc) for a in edge for b in edge for cc in (0, L - 1, 2 ** 256 - 1)]
    tr += [tuple(rnd.randrange(2 ** 256) for _ in range(3)) for _ in range(300)]
    c['sc_muladd'] = _rows([words(a, 8) + words(b, 8) + words(cc, 8) for a, b, cc in tr], 24)
    ds = [0, 1, HS_MAX - 1, 2 ** 128 - 1, 2 ** 128, 2 ** 131]
    ss = [0, 1, L - 1]
    ms = [(d, s) for d in ds for s in ss] + [(rnd.randrange(HS_MAX), rnd.randrange(L)) for _ in range(300)]
    c['sc_mul_small'] = _rows([words(d, 5) + words(s, 8) for d, s in ms], 13)
    hs = lattice_h()
    c['half_scalars'] = _rows([words(h, 8) for _, h, _ in hs], 8)
    # lattice_one: fixed, planted and 500 of the random h; digest h + k L, S, force_full
    sel = [t for t in hs if t[0] != 'random'] + [t for t in hs if t[0] == 'random'][:500]
    rows = []
    for n, (_, h, _) in enumerate(sel):
        kmax = (2 ** 512 - 1 - h) // L
        for ff in (0, 1):
            i = 2 * n + ff
            k = (0, 1, rnd.randrange(kmax + 1), kmax)[i % 4]
            s = (0, 1, L - 1, rnd.randrange(L))[(i // 4) % 4]
            x = h + k * L
            assert x < 2 ** 512 and x % L == h
            rows.append(words(x, 16) + words(rnd.randrange(2 ** 256), 8) + words(s, 8) + [ff])
    c['lattice_one'] = _rows(rows, 33)
    return c


def check_half(h, st, c, d, neg, what):
    """the integer properties of an HS_HALF result (pv_lattice.h half_scalars)"""
    assert st in (HS_HALF, HS_DEFER), what
    if st == HS_DEFER:
        assert c == 0 and d == 0 and neg == 0, what
        return
    assert d % 2 == 1 and d > 0, what
    assert ((-c if neg else c) - d * h) % L8 == 0, what
    assert c < HS_MAX and d < HS_MAX, what
    assert neg in (0, 1), what


S_PAT = sum(0x80008000 << (32 * k) for k in range(8))
H_PAT = sum(0x88888888 << (32 * k) for k in range(8))


def _check_scalar(op, inp, out):
    for r, (i, o) in enumerate(zip(inp, out)):
        what = '{} case {}'.format(op, r)
        if op == 'sc_reduce64':
            assert unwords(o) == unwords(i) % L, what
        elif op == 'sc_muladd':
            assert unwords(o) == (unwords(i[0:8]) * unwords(i[8:16]) + unwords(i[16:24])) % L, what
        elif op == 'sc_mul_small':
            assert unwords(o) == unwords(i[0:5]) * unwords(i[5:13]) % L, what
        elif op == 'half_scalars':
            check_half(unwords(i), int(o[0]), unwords(o[1:6]), unwords(o[6:11]), int(o[11]), what)
        elif op == 'lattice_one':
            h, s, ff = unwords(i[0:16]) % L, unwords(i[24:32]), int(i[32])
            st, flags = int(o[20]), int(o[18])
            assert flags & 0xff == st and flags >> 9 == 0 and int(o[19]) == 0, what
            assert st in (HS_HALF, HS_DEFER) and (st == HS_DEFER or not ff), what
            if st == HS_HALF:
                c, d = unwords(o[0:5]) - PAT33, unwords(o[5:10]) - PAT33
                assert c >= 0 and d >= 0, what
                check_half(h, st, c, d, (flags >> 8) & 1, what)
                assert unwords(o[10:18]) == d * s % L + S_PAT, what      # s' = d S mod L, offset form
            else:
                assert flags >> 8 == 0, what
                assert unwords(o[0:8]) == h + H_PAT and int(o[8]) == 0 and int(o[9]) == 0, what
                assert unwords(o[10:18]) == s + S_PAT, what
        else:
            raise KeyError(op)


# ---------------------------------------------------------------- BN254
BNP = BNG.P
BN_R = 2 ** 280
BN_RINV = pow(BN_R, -1, BNP)
LAZY = 2 ** 29 - 1


def bn_value(limbs):
    return sum(int(v) << (28 * k) for k, v in enumerate(limbs))


def bn_norm_limbs(x):
    """normalised limbs of an integer: limbs 0..8 in [0, 2^28), limb 9 signed"""
    out = [(x >> (28 * k)) & (2 ** 28 - 1) for k in range(9)]
    return out + [x >> 252]


def _u32(v):
    return [x & 0xffffffff for x in v]


def _s32rows(row, n):
    a = np.asarray(row, dtype=np.uint32).astype(np.int32)
    return [[int(x) for x in a[10 * j:10 * j + 10]] for j in range(n)]


@functools.lru_cache(None)
def bn_pool():
    """(lazy vectors, normalised vectors)"""
    rnd = random.Random(254)
    # eight sign patterns of every limb at +-(2^29 - 1): all +, all - (crossed below they give the pairs
    # of tests/test_bn_madchains.py), alternating, split halves, and two seeded ones
    signs = [[1] * NL, [-1] * NL, [1, -1] * 5, [-1, 1] * 5, [1] * 5 + [-1] * 5, [-1] * 5 + [1] * 5]
    signs += [[rnd.choice((1, -1)) for _ in range(NL)] for _ in range(2)]
    lazy = [[sg * LAZY for sg in pat] for pat in signs]
    for j in range(NL):
        for s in (LAZY, -LAZY):
            lazy.append([s if i == j else 0 for i in range(NL)])
    normal = [bn_norm_limbs(x * BN_R % BNP) for x in (0, 1, BNP - 1)] + [bn_norm_limbs(BN_R % BNP)]
    assert normal[1] == normal[3]
    lazy += normal
    lazy += [[rnd.randrange(-LAZY, LAZY + 1) for _ in range(NL)] for _ in range(400)]
    # normalised: mul outputs lie in (-p/2, 3p/2); any limb 9 below 2^28 in magnitude keeps a sum of two lazy
    normal += [bn_norm_limbs(rnd.randrange(-BNP // 2, 3 * BNP // 2)) for _ in range(200)]
    normal += [[rnd.randrange(2 ** 28) for _ in range(NL - 1)] + [rnd.randrange(-2 ** 28 + 1, 2 ** 28)]
               for _ in range(200)]
    return lazy, normal


def _bn_cases():
    lazy, normal = bn_pool()
    rnd = random.Random(255)
    n, m = len(lazy), len(normal)
    c = {}
    pairs = [(lazy[i], lazy[j]) for i in range(8) for j in range(8)]      # every extreme against every extreme
    pairs += [(lazy[i], lazy[(13 * i + 5) % n]) for i in range(n)]
    c['bn_mul'] = _rows([_u32(a + b) for a, b in pairs], 20)
    c['bn_sqr'] = c['bn_norm'] = _rows([_u32(a) for a in lazy], 10)
    # canon folds a product: its operand also keeps the magnitude bound of pv_bn254.h (< 2^266), so the
    # top limb stays below 2^13
    c['bn_canon'] = _rows([_u32(a[:9] + [max(-2 ** 13 + 1, min(2 ** 13 - 1, a[9]))]) for a in lazy], 10)
    # reduce: a normalised value of any magnitude < 2^282
    red = normal + [[rnd.randrange(2 ** 28) for _ in range(NL - 1)] + [t] for t in
                    (2 ** 30 - 1, -2 ** 30 + 1, 2 ** 29, -2 ** 29, 0, -1, 1)]
    red += [[rnd.randrange(2 ** 28) for _ in range(NL - 1)] + [rnd.randrange(-2 ** 30 + 1, 2 ** 30)]
            for _ in range(400)]
    c['bn_reduce'] = _rows([_u32(a) for a in red], 10)
    tr = [(normal[i % m], normal[(7 * i + 1) % m], lazy[i]) for i in range(n)]
    c['bn_add_mul'] = c['bn_sub_mul'] = _rows([_u32(a + b + d) for a, b, d in tr], 30)
    # f2mul: x lazy (x.a + x.b below 2^30 per limb), y normalised; f2sqr: x normalised
    c['bn_f2mul'] = _rows([_u32(lazy[i] + lazy[(3 * i + 7) % n] + normal[i % m] + normal[(5 * i + 2) % m])
                           for i in range(n)], 40)
    c['bn_f2sqr'] = _rows([_u32(normal[i] + normal[(5 * i + 2) % m]) for i in range(m)], 20)
    return c


def _is_normal(v):
    return all(0 <= x < 2 ** 28 for x in v[:9])


def _check_bn(op, inp, out):
    one_m = bn_norm_limbs(BN_R % BNP)
    for r, (i, o) in enumerate(zip(inp, out)):
        what = '{} case {}'.format(op, r)
        a = _s32rows(i, len(i) // 10)
        h = _s32rows(o, len(o) // 10)
        if op in ('bn_mul', 'bn_sqr', 'bn_add_mul', 'bn_sub_mul'):
            if op == 'bn_mul':
                x, y = a
            elif op == 'bn_sqr':
                x, y = a[0], None
            else:
                sg = 1 if op == 'bn_add_mul' else -1
                x, y = [p + sg * q for p, q in zip(a[0], a[1])], a[2]
            want = ref_mul(x, y, sqr=y is None)
            assert h[0] == want, what                                   # the exact limbs
            yv = bn_value(x if y is None else y)
            assert bn_value(h[0]) % BNP == bn_value(x) * yv * BN_RINV % BNP, what
            assert _is_normal(h[0]), what
        elif op == 'bn_norm':
            assert bn_value(h[0]) == bn_value(a[0]) and _is_normal(h[0]), what
            assert h[0] == bn_norm_limbs(bn_value(a[0])), what
        elif op == 'bn_reduce':
            v = bn_value(h[0])
            assert v % BNP == bn_value(a[0]) % BNP and _is_normal(h[0]) and abs(v) < 3 * BNP, what
        elif op == 'bn_canon':
            assert h[0] == bn_norm_limbs(bn_value(a[0]) % BNP), what     # fold(mul(a, ONE_M)): a mod p in [0, p)
            assert h[0] == _fold(ref_mul(a[0], one_m)), what
        elif op == 'bn_f2mul':
            xa, xb, ya, yb = (bn_value(v) for v in a)
            assert bn_value(h[0]) % BNP == (xa * ya - xb * yb) * BN_RINV % BNP, what
            assert bn_value(h[1]) % BNP == (xa * yb + xb * ya) * BN_RINV % BNP, what
            assert _is_normal(h[0]) and _is_normal(h[1]), what
        elif op == 'bn_f2sqr':
            xa, xb = (bn_value(v) for v in a)
            assert bn_value(h[0]) % BNP == (xa * xa - xb * xb) * BN_RINV % BNP, what
            assert bn_value(h[1]) % BNP == 2 * xa * xb * BN_RINV % BNP, what
            assert _is_normal(h[0]) and _is_normal(h[1]), what
        else:
            raise KeyError(op)


def _fold(t):
    v = bn_value(t)
    assert -BNP < v < 2 * BNP
    return bn_norm_limbs(v % BNP)


# ----------------------------------------------------------- lane quads
ED_D = -121665 * pow(121666, -1, P) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def ed_add(a, b):
    (x1, y1), (x2, y2) = a, b
    t = ED_D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, -1, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, -1, P) % P)


def ed_neg(a):
    return (-a[0] % P, a[1])


def ed_mul(k, a):
    r = (0, 1)
    while k:
        if k & 1:
            r = ed_add(r, a)
        a = ed_add(a, a)
        k >>= 1
    return r


def ed_x(y, sign):
    u, v = (y * y - 1) % P, (ED_D * y * y + 1) % P
    x = pow(u * pow(v, -1, P) % P, (P + 3) // 8, P)
    if (x * x * v - u) % P:
        x = x * SQRT_M1 % P
    if (x * x * v - u) % P:
        return None
    return P - x if (x & 1) != sign and x else x


ED_B = (ed_x(4 * pow(5, -1, P) % P, 0), 4 * pow(5, -1, P) % P)
ED_O = (0, 1)


@functools.lru_cache(None)
def quad_points():
    rnd = random.Random(8)
    pts = [ed_mul(k, ED_B) for k in (1, 2, 3, 2 ** 128, L - 1)] + [ED_O]
    t2, t4 = (0, P - 1), (SQRT_M1, 0)
    t8 = None
    y = 2
    while t8 is None:       # L Q has order dividing 8 for every curve point Q
        x = ed_x(y, 0)
        if x is not None:
            q = ed_mul(L, (x, y))
            if ed_mul(4, q) != ED_O:
                t8 = q
        y += 1
    assert ed_mul(2, t2) == ED_O and ed_mul(2, t4) == t2 and ed_mul(2, t8) in (t4, ed_neg(t4))
    pts += [t2, t4, t8]
    pts += [ed_mul(rnd.randrange(1, L), ED_B) for _ in range(50)]
    return tuple(pts)


def _p3(pt, rnd):
    z = rnd.randrange(1, P)
    x, y = pt
    return [fe_limbs(x * z % P), fe_limbs(y * z % P), fe_limbs(z), fe_limbs(x * y * z % P)]


def _cached(pt, rnd, neg):
    """add order (Y - X, Y + X, 2 d T, 2 Z); a negative digit swaps the first two"""
    z = rnd.randrange(1, P)
    x, y = pt[0] * z % P, pt[1] * z % P
    e = [fe_limbs((y - x) % P), fe_limbs((y + x) % P), fe_limbs(2 * ED_D * pt[0] * pt[1] * z % P), fe_limbs(2 * z % P)]
    return [e[1], e[0], e[2], e[3]] if neg else e


@functools.lru_cache(None)
def _quad_cases():
    pts = quad_points()
    rnd = random.Random(81)
    c = {}
    c['q_dbl'] = c['q_to_cached'] = _rows([sum(_p3(p, rnd), []) for p in pts], 40)
    pairs = [(p, p) for p in pts] + [(p, ed_neg(p)) for p in pts] + [(p, ED_O) for p in pts] + [(ED_O, p) for p in pts]
    pairs += [(pts[i], pts[(7 * i + 3) % len(pts)]) for i in range(len(pts))]
    rows, want = [], []
    for p, e in pairs:
        for neg in (0, 1):
            rows.append(sum(_p3(p, rnd), []) + sum(_cached(e, rnd, neg), []) + [neg])
            want.append(ed_add(p, ed_neg(e) if neg else e))
    c['q_add'] = _rows(rows, 81)
    c['q_sum_is_identity'] = _rows([sum(_p3(p, rnd), []) + sum(_cached(e, rnd, 0), []) for p, e in pairs], 80)
    return c, {'q_add': want, 'q_sum_is_identity': [ed_add(p, e) == ED_O for p, e in pairs]}


def _proj(o):
    return [fe_value(v) % P for v in _fes(o, 4)]


def _check_quad(op, inp, out):
    want = _quad_cases()[1]
    for r, (i, o) in enumerate(zip(inp, out)):
        what = '{} case {}'.format(op, r)
        px, py, pz, pt = _proj(i[:40])
        zi = pow(pz, -1, P)
        p = (px * zi % P, py * zi % P)
        if op in ('q_dbl', 'q_add'):
            x, y, z, t = _proj(o)
            wx, wy = ed_add(p, p) if op == 'q_dbl' else want[op][r]
            assert z != 0 and x == wx * z % P and y == wy * z % P, what       # projectively equal
            assert t * z % P == x * y % P, what
            assert all(tight_out(v) for v in _fes(o, 4)), what
        elif op == 'q_to_cached':
            got = _proj(o)
            assert got == [(py - px) % P, (py + px) % P, 2 * ED_D * pt % P, 2 * pz % P], what
            assert all(tight_out(v) for v in _fes(o, 4)), what
        elif op == 'q_sum_is_identity':
            assert [int(v) for v in o] == [1 if want[op][r] else 0] * 4, what
        else:
            raise KeyError(op)


# ------------------------------------------------------------------ API
@functools.lru_cache(None)
def cases():
    c = {}
    c.update(_field_cases())
    c.update(_scalar_cases())
    c.update(_bn_cases())
    c.update(_quad_cases()[0])
    assert set(c) == set(ALL_OPS)
    for op, a in c.items():
        assert a.dtype == np.uint32 and a.shape[1] == ALL_OPS[op][0], op
        a.setflags(write=False)
    return c


def check(op, inp, out):
    """assert the integer reference of `op` on every row of out (rows of inp -> rows of out)"""
    assert len(inp) == len(out) and out.shape[1] == ALL_OPS[op][1]
    if op in QUAD_OPS:
        _check_quad(op, inp, out)
    elif op in BN_OPS:
        _check_bn(op, inp, out)
    elif op.startswith('fe_'):
        _check_field(op, inp, out)
    else:
        _check_scalar(op, inp, out)


# -------------------------------------------------------------- runners
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


@functools.lru_cache(None)
def host_libs():
    """(libhostcheck, libbn254check): the host twins hcw_<op> / bncw_<op>"""
    subprocess.run(['make', '-s', '-C', HC_DIR, 'libhostcheck.so', 'libbn254check.so'], check=True)
    return ctypes.CDLL(os.path.join(HC_DIR, 'libhostcheck.so')), ctypes.CDLL(os.path.join(HC_DIR, 'libbn254check.so'))


def host_run(op, inp):
    """the host twin of `op` on the rows of inp; asserts that no bound hook fired"""
    hc, bnc = host_libs()
    inp = np.ascontiguousarray(inp, np.uint32)
    out = np.full((len(inp), ALL_OPS[op][1]), 0xa5a5a5a5, np.uint32)
    if op in BN_OPS:
        bnc.bnc_reset()
        getattr(bnc, 'bncw_' + op)(_p(inp), ctypes.c_uint64(len(inp)), _p(out))
        assert bnc.bnc_bad() == 0 and bnc.bnc_disc_bad() == 0, op + ': an operand outside the bn::mul contract'
    else:
        hc.hc_reset_counts()
        getattr(hc, 'hcw_' + op)(_p(inp), ctypes.c_uint64(len(inp)), _p(out))
        assert hc.hc_get_counts(_p(np.zeros(8, np.uint64))) == 0, op + ': an operand outside the field contract'
    return out


@functools.lru_cache(None)
def host_outputs(op):
    out = host_run(op, cases()[op])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def dev_lib():
    return ctypes.CDLL(os.path.join(REPO, 'tools', 'devcheck', 'libdevcheck.so'))


def dev_run(op, inp):
    """(status, out) of the device kernel of `op` on the rows of inp"""
    inp = np.ascontiguousarray(inp, np.uint32)
    out = np.zeros((len(inp), ALL_OPS[op][1]), np.uint32)
    fn = getattr(dev_lib(), 'dc_' + op)
    fn.restype = ctypes.c_int
    return fn(_p(inp), ctypes.c_uint64(len(inp)), _p(out)), out
