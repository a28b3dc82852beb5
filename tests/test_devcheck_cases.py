"""The device check's case lists and host twins, on the CPU (tools/devcheck,
tests/_devcheck_cases.py): every generated operand is inside its header's
contract, every host twin (the plain C++ branches, g++) equals the
Python-integer reference on every case with no bound hook firing, the planted
partial quotients are where they were planted, and libdevcheck.so builds for
gfx950 and exports every dc_* entry point.  The device side of the same cases is
tests/test_gpu_devcheck.py."""
import ctypes
import hashlib
import sys

import numpy as np
import pytest

import _devcheck_cases as D
from conftest import PKG


def _digest(c):
    h = hashlib.sha256()
    for op in sorted(c):
        h.update(op.encode() + c[op].tobytes())
    return h.hexdigest()


def test_generators_are_deterministic_and_in_contract():
    """cases() asserts the restated hc_check_mul / hc_check_sq / hc_check_sq2x on
    every field operand it emits; built twice it gives the same bytes"""
    first = _digest(D.cases())
    for f in (D.cases, D.field_pool, D.lattice_h, D.bn_pool, D.quad_points, D._quad_cases):
        f.cache_clear()
    assert _digest(D.cases()) == first
    for op, a in D.cases().items():
        assert len(a) >= max(D.QUAD_CUTS if op in D.QUAD_OPS else D.LANE_CUTS), op
    sp, rt, rl = D.field_pool()
    assert len(rt) == 300 and all(D.is_tight(v) for v in rt)
    assert len(rl) == 300 and all(D.is_loose(v) for v in rl) and not all(D.is_tight(v) for v in rl)
    # the header's TIGHT-only rule for 2 f^2: the LOOSE maximum is outside fe_sq2x's contract
    assert not D.check_sq2x(D._maxvec(D.LOOSE_E, D.LOOSE_O)) and D.check_sq(D._maxvec(D.LOOSE_E, D.LOOSE_O))


def test_planted_quotients_sit_where_planted():
    hs = D.lattice_h()
    planted = [(h, e) for k, h, e in hs if k == 'planted']
    assert len(planted) == 260 + 4 * sum(1 for e in D.PLANT_E if e >= 8)
    assert all(e in D.euclid_quotients(h) for h, e in planted)
    assert sum(1 for k, h, e in hs if k == 'random') == 4000
    assert all(0 <= h < D.L for _, h, _ in hs)


@pytest.mark.parametrize('op', sorted(D.ALL_OPS))
def test_host_twin_equals_integer_reference(op):
    inp = D.cases()[op]
    out = D.host_outputs(op)            # asserts hc_get_counts / bnc_bad: no bound violation
    assert not (out == 0xa5a5a5a5).all(axis=1).any(), 'a case the twin did not write'
    D.check(op, inp, out)


def test_hc_lattice_one_and_half_scalars_entry_points():
    """hc_lattice_one is the lattice_one twin; the byte-level hc_half_scalars agrees with the word-level twin"""
    hc, _ = D.host_libs()
    inp = D.cases()['lattice_one']
    out = np.zeros((len(inp), 21), np.uint32)
    hc.hc_lattice_one(D._p(inp), ctypes.c_uint64(len(inp)), D._p(out))
    assert (out == D.host_outputs('lattice_one')).all()
    hin, hout = D.cases()['half_scalars'], D.host_outputs('half_scalars')
    for i in range(0, len(hin), 37):
        c, d, neg = ctypes.create_string_buffer(20), ctypes.create_string_buffer(20), ctypes.c_uint32()
        st = hc.hc_half_scalars(hin[i].tobytes(), c, d, ctypes.byref(neg))
        assert st == hout[i][0]
        if st == D.HS_HALF:
            assert (c.raw, d.raw, neg.value) == (hout[i][1:6].tobytes(), hout[i][6:11].tobytes(), hout[i][11])


def test_deferral_caps_on_the_host():
    """the planted quotient decides the path: every e >= 2^32 - 2 defers; below the
    near-2^32 window at most 2 % of the planted cases defer (their random tails
    keep the generic ~0.2 %), and at most 1 % of the 4,000 random h"""
    hs, out = D.lattice_h(), D.host_outputs('half_scalars')
    st = {k: [] for k in ('low', 'high', 'random')}
    for (kind, h, e), o in zip(hs, out):
        if kind == 'random':
            st['random'].append(int(o[0]))
        elif kind == 'planted' and e <= 2 ** 32 - 5:
            st['low'].append(int(o[0]))
        elif kind == 'planted' and e >= 2 ** 32 - 2:
            st['high'].append(int(o[0]))
    assert len(st['random']) == 4000 and st['low'] and st['high']
    assert all(s == D.HS_DEFER for s in st['high'])
    assert st['low'].count(D.HS_DEFER) <= 0.02 * len(st['low'])
    assert st['random'].count(D.HS_DEFER) <= 0.01 * len(st['random'])
    # the edge values: no Euclid trip below 2^128 (c = h, d = 1)
    for (kind, h, _), o in zip(hs, out):
        if kind == 'fixed' and h < 2 ** 128:
            assert (int(o[0]), D.unwords(o[1:6]), D.unwords(o[6:11]), int(o[11])) == (D.HS_HALF, h, 1, 0)


def test_libdevcheck_builds_and_exports_every_op():
    """cross-compiles for gfx950 (no GPU needed) and resolves every dc_<op>; nothing is called"""
    sys.path.insert(0, PKG)
    import build as pkg_build
    lib = ctypes.CDLL(pkg_build.build_devcheck())
    for op in D.ALL_OPS:
        assert getattr(lib, 'dc_' + op) is not None, op
