"""The device-only arithmetic variants on the GPU (tools/devcheck): every op of
dc_ops_pv.h / dc_ops_bn.h runs on the chosen operands of
tests/_devcheck_cases.py, one case per lane (one point per lane quad), through
the code the device compiles -- the v_mad_u64_u32 asm chains, the interleaved
generated chains, the __builtin_addc / subc carry forms, v_rcp_f64 + Newton, the
BN254 asm columns, the DPP quad_perm moves -- and its raw result words must equal

  * the host twin's words bit for bit (g++, the plain C++ branches), and
  * the Python-integer reference in value.

One documented exception: a lattice case whose exact Euclid has a partial
quotient in [2^32 - 6, 2^32 + 1] may come back HS_HALF on one side and HS_DEFER
on the other (the decision compares a float64 quotient estimate, computed
differently on the device, with 4294967294.0); every HS_HALF result must still
satisfy the integer properties, the cases that took the exception are counted
and printed, and the count cannot exceed the number of planted cases in that
window.  Everything else is exact; there is no tolerance."""
import time

import numpy as np
import pytest

import _devcheck_cases as D

pytestmark = pytest.mark.gpu

_state = {'failed': None, 'full': {}}


def _dev(op, inp):
    """one dc_<op> call; after a non-zero status nothing more is launched in this module"""
    assert _state['failed'] is None, 'not launched: dc_{} returned HIP status {} earlier'.format(*_state['failed'])
    t0 = time.perf_counter()
    st, out = D.dev_run(op, inp)
    dt = time.perf_counter() - t0
    if st != 0:
        _state['failed'] = (op, st)
    assert st == 0, 'dc_{} returned HIP status {}'.format(op, st)
    print('dc_{}: {} cases in {:.1f} ms'.format(op, len(inp), 1e3 * dt))
    return out


def _full(op):
    if op not in _state['full']:
        _state['full'][op] = _dev(op, D.cases()[op])
    return _state['full'][op]


def _lattice_h(op, row):
    return D.unwords(row[0:8]) if op == 'half_scalars' else D.unwords(row[0:16]) % D.L


def _status(op, row):
    return int(row[0]) if op == 'half_scalars' else int(row[20])


def _planted_near():
    return {h for k, h, e in D.lattice_h() if k == 'planted' and D.NEAR_LO <= e <= D.NEAR_HI}


@pytest.mark.parametrize('op', sorted(D.ALL_OPS))
def test_device_equals_host_twin_and_integer_reference(op):
    inp, host = D.cases()[op], D.host_outputs(op)
    dev = _full(op)
    assert dev.shape == host.shape
    diff = np.nonzero((dev != host).any(axis=1))[0]
    if op in ('half_scalars', 'lattice_one'):
        near = _planted_near()
        bound = sum(1 for row in inp if _lattice_h(op, row) in near)
        for r in diff:
            h = _lattice_h(op, inp[r])
            assert D.near_2_32(h), '{} case {}: device {} != host {}'.format(op, r, dev[r], host[r])
            assert {_status(op, dev[r]), _status(op, host[r])} == {D.HS_HALF, D.HS_DEFER}, (op, r, dev[r], host[r])
        print('{}: {} near-2^32 cases took the other of HS_HALF / HS_DEFER (bound {})'.format(op, len(diff), bound))
        assert len(diff) <= bound
    else:
        assert len(diff) == 0, '{} case {}: device {} != host {} for input {}'.format(
            op, diff[0], dev[diff[0]], host[diff[0]], inp[diff[0]])
    D.check(op, inp, dev)


@pytest.mark.parametrize('op', sorted(D.ALL_OPS))
def test_batch_sizes_give_the_same_words(op):
    """the case list cut to 1 / 63 / 64 / 65 / 257 cases (1 / 15 / 16 / 17 quads):
    partial waves and blocks return what the same cases return inside the full list"""
    inp, full = D.cases()[op], _full(op)
    for n in (D.QUAD_CUTS if op in D.QUAD_OPS else D.LANE_CUTS):
        out = _dev(op, inp[:n])
        assert (out == full[:n]).all(), (op, n)
