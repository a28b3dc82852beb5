"""fe_sub / fe_sub4 on the device at the edges of the subtrahend contract
(pv_field.h: g <= the limbs of 2p / 4p): the device forms each limb as
|K - g| + f in one v_sad_u32, which equals f + K - g exactly up to g = K.  Each
row runs through the devcheck lane-op entry and is compared limb for limb with
Python integers; no row is skipped and there is no tolerance."""
import numpy as np
import pytest

import _devcheck_cases as D

pytestmark = pytest.mark.gpu


def _boundary_rows(k):
    K = [k * v for v in D.P_LIMBS]
    zero = [0] * 10
    fmax = [D.LOOSE_O if i & 1 else D.LOOSE_E for i in range(10)]
    fmid = [(0x1234567 * (i + 3)) % (D.TIGHT_O if i & 1 else D.TIGHT_E) for i in range(10)]
    gs = [zero, K]                                                            # g = 0, g = K in all limbs
    gs += [[K[i] if i == j else 0 for i in range(10)] for j in range(10)]     # g = K in one limb at a time
    gs += [[K[i] - 1 if i == j else K[i] for i in range(10)] for j in range(10)]   # one below K in one limb
    rows = [f + g for g in gs for f in (zero, fmid, fmax)]
    rows += [fmax + [K[i] if (i & 1) == ph else 0 for i in range(10)] for ph in (0, 1)]
    return np.array(rows, dtype=np.uint32)


@pytest.mark.parametrize('op,k', [('fe_sub', 2), ('fe_sub4', 4)])
def test_sub_boundary_rows_limb_exact(op, k):
    inp = _boundary_rows(k)
    assert len(inp) == 68    # 136 rows over the two ops
    st, out = D.dev_run(op, inp)
    assert st == 0, 'dc_{} returned HIP status {}'.format(op, st)
    K = [k * v for v in D.P_LIMBS]
    for r, (i, o) in enumerate(zip(inp, out)):
        f, g = [int(x) for x in i[:10]], [int(x) for x in i[10:]]
        want = [f[t] + K[t] - g[t] for t in range(10)]
        assert all(0 <= w < 2 ** 32 for w in want)
        assert [int(x) for x in o] == want, '{} row {}: f {} g {}'.format(op, r, f, g)
    host = D.host_run(op, inp)    # the plain C++ form, subtrahend check on: same words, nothing flagged
    assert (host == out).all()
