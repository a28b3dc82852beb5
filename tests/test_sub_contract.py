"""fe_sub / fe_sub4's subtrahend contract (pv_field.h: every limb of g at most
the limb of 2p / 4p, under which the device's |K - g| + f equals f + K - g) is
asserted by the host instrumentation build: PV_CHECK_SUB is live on the fixture
runs, and flags a subtrahend one past the bound in any limb."""
import ctypes

import numpy as np
import pytest

import _devcheck_cases as D
from conftest import split_sm
from test_hostcheck import _load, counts, hc_verify


@pytest.fixture(scope='module')
def hc():
    lib = _load()
    lib.hc_get_sub_checks.restype = ctypes.c_uint64
    return lib


def test_sub_checks_run_on_raw_vectors(hc, raw_vectors):
    r = raw_vectors
    sel = np.arange(0, len(r['verdict']), 5)
    msgs = [r['blob'][int(r['off'][i]):int(r['off'][i + 1])].tobytes() for i in sel]
    off = np.zeros(len(sel) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    hc.hc_reset_counts()
    got = hc_verify(hc, r['pk'][sel], r['sig'][sel], np.frombuffer(b''.join(msgs), np.uint8), off)
    c, bad = counts(hc)
    n = hc.hc_get_sub_checks()
    print('raw vectors: {} subtrahend checks for {} verifies'.format(n, len(sel)))
    assert 0 < n <= int(c[6])   # c[6] also counts fe_neg, which has no subtrahend bound
    assert bad == 0
    assert (got == r['verdict'][sel].astype(bool)).all()


def test_sub_checks_run_on_adversarial(hc, adversarial):
    rows = [row for row in split_sm(adversarial) if len(row[2]) >= 64]
    pk = np.stack([np.frombuffer(r[1], np.uint8) for r in rows])
    sig = np.stack([np.frombuffer(r[2][:64], np.uint8) for r in rows])
    msgs = [r[2][64:] for r in rows]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    hc.hc_reset_counts()
    hc_verify(hc, pk, sig, np.frombuffer(b''.join(msgs), np.uint8), off)
    _, bad = counts(hc)
    n = hc.hc_get_sub_checks()
    print('adversarial: {} subtrahend checks for {} verifies'.format(n, len(rows)))
    assert n > 0
    assert bad == 0


def _direct(hc, op, g):
    """fe_sub / fe_sub4 called once with f = 0 and subtrahend g -> (checks, bad)"""
    inp = np.array([[0] * 10 + list(g)], np.uint32)
    out = np.zeros((1, 10), np.uint32)
    hc.hc_reset_counts()
    getattr(hc, 'hcw_' + op)(ctypes.c_void_p(inp.ctypes.data), ctypes.c_uint64(1), ctypes.c_void_p(out.ctypes.data))
    _, bad = counts(hc)
    return hc.hc_get_sub_checks(), bad


@pytest.mark.parametrize('k', [2, 4])
@pytest.mark.parametrize('limb', range(10))
def test_subtrahend_one_past_the_bound_is_flagged(hc, capfd, k, limb):
    op = 'fe_sub' if k == 2 else 'fe_sub4'
    K = [k * v for v in D.P_LIMBS]
    assert _direct(hc, op, K) == (1, 0), 'g = K in every limb is inside the contract'
    g = [0] * 10
    g[limb] = K[limb]
    assert _direct(hc, op, g) == (1, 0)
    g[limb] = K[limb] + 1
    assert _direct(hc, op, g) == (1, 1)
    capfd.readouterr()   # the violation's message on stderr
    hc.hc_reset_counts()
