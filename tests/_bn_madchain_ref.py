"""bn::mul / bn::sqr of pv_bn254.h restated over Python integers (the C++ loops,
int64 column sums), shared by tests/test_bn_madchains.py (the generator's column
lists) and the device check (tests/_devcheck_cases.py)."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(REPO, 'tools', 'gen_bn_madchains.py')


def _gen():
    spec = importlib.util.spec_from_file_location('gen_bn_madchains', GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()
NL, PL = G.NL, G.PL
M28 = (1 << 28) - 1
NP = (-pow(G.P, -1, 1 << 28)) % (1 << 28)


def _s64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _s32(x):
    x &= (1 << 32) - 1
    return x - (1 << 32) if x >> 31 else x


def ref_mul(a, b, sqr=False):
    """pv_bn254.h bn::mul / bn::sqr (C++ loops), int64 column sums."""
    d = [2 * x for x in a]
    m = [0] * NL
    r = [0] * NL
    carry = 0
    for k in range(2 * NL - 1):
        acc = carry
        lo = 0 if k < NL else k - NL + 1
        if sqr:
            i = lo
            while 2 * i < k:
                acc += a[i] * d[k - i]
                i += 1
            if k % 2 == 0:
                acc += a[k // 2] * a[k // 2]
        else:
            for i in range(lo, min(k, NL - 1) + 1):
                acc += a[i] * b[k - i]
        if k < NL:
            for i in range(k):
                if PL[k - i]:
                    acc += m[i] * PL[k - i]
            m[k] = ((acc & 0xffffffff) * NP) & M28
            acc += m[k] * PL[0]
        else:
            for i in range(k - NL + 1, NL):
                if PL[k - i]:
                    acc += m[i] * PL[k - i]
            r[k - NL] = _s32(acc & M28)
        assert -(1 << 63) <= acc < (1 << 63)
        carry = _s64(acc) >> 28
    r[NL - 1] = _s32(carry)
    return r
