"""The Lehmer rounds of the lattice stage on the GPU.

Device check (tools/devcheck): the planted families of tests/_lattice_cases.py
and 4,096 random h go through dc_half_scalars and dc_lattice_one, one case per
lane, and the device words must equal the host twin's bit for bit.  The
families stop at a quotient of 2^32 - 7, so the documented host/device window
around 2^32 (tests/test_gpu_devcheck.py) is not in play and there is no
exception here.  Cut to 1 / 63 / 64 / 65 / 257 cases, and once as waves in
which lanes that take 98 steps sit beside lanes that take none.

Kernel level: 4,160 signatures (65 wave tasks) signed by the oracle's signer
go through k_hash + k_lattice + k_curve_half, through k_chunk_half, and through
the small-batch kernel at n = 1 and 65; verdicts equal the oracle's and the
deferred count equals the host build's.  Exact everywhere: no tolerance."""
import ctypes
import random

import numpy as np
import pytest

import _devcheck_cases as D
import _lattice_cases as LC
import _oracle as orc

pytestmark = pytest.mark.gpu

_state = {'failed': None}


def _dev(op, inp):
    """one dc_<op> call; after a non-zero status nothing more is launched in this module"""
    assert _state['failed'] is None, 'not launched: dc_{} returned HIP status {} earlier'.format(*_state['failed'])
    st, out = D.dev_run(op, inp)
    if st != 0:
        _state['failed'] = (op, st)
    assert st == 0, 'dc_{} returned HIP status {}'.format(op, st)
    return out


def _hs():
    hs = list(LC.planted_all()) + [LC.longest()] + list(LC.random_h(4096))
    assert not any(D.near_2_32(h) for h in hs[:len(hs) - 4096])
    return hs


def _rows(op, hs):
    if op == 'half_scalars':
        return D._rows([D.words(h, 8) for h in hs], 8)
    rnd = random.Random(7700)
    rows = []
    for i, h in enumerate(hs):
        kmax = (2 ** 512 - 1 - h) // D.L
        k = (0, 1, rnd.randrange(kmax + 1), kmax)[i % 4]
        s = (0, 1, D.L - 1, rnd.randrange(D.L))[(i // 4) % 4]
        rows.append(D.words(h + k * D.L, 16) + D.words(rnd.randrange(2 ** 256), 8) + D.words(s, 8) + [0])
    return D._rows(rows, 33)


@pytest.fixture(scope='module')
def full():
    """op -> (input rows, host twin's words, device words), each computed once"""
    out = {}
    for op in ('half_scalars', 'lattice_one'):
        inp = _rows(op, _hs())
        out[op] = (inp, D.host_run(op, inp), _dev(op, inp))
    return out


def _near(op, row):
    return D.near_2_32(D.unwords(row[0:8]) if op == 'half_scalars' else D.unwords(row[0:16]) % D.L)


@pytest.mark.parametrize('op', ['half_scalars', 'lattice_one'])
def test_device_words_equal_host_twin(full, op):
    inp, host, dev = full[op]
    diff = np.nonzero((dev != host).any(axis=1))[0]
    # a random h with a quotient inside the near-2^32 window (chance about 2^-25 each) would be the
    # documented exception; none of the seeded ones has one
    assert not any(_near(op, inp[r]) for r in range(len(inp)))
    assert len(diff) == 0, '{} case {}: device {} != host {} for input {}'.format(
        op, diff[0], dev[diff[0]], host[diff[0]], inp[diff[0]])
    D.check(op, inp, dev)
    st = dev[:, 0] if op == 'half_scalars' else dev[:, 20]
    assert (st == D.HS_HALF).sum() > 4000 and (st == D.HS_DEFER).sum() >= 8    # both outcomes were compared


@pytest.mark.parametrize('op', ['half_scalars', 'lattice_one'])
def test_batch_cuts(full, op):
    inp, host, dev = full[op]
    for n in D.LANE_CUTS:
        assert (_dev(op, inp[:n]) == dev[:n]).all(), (op, n)


@pytest.mark.parametrize('op', ['half_scalars', 'lattice_one'])
def test_waves_of_longest_beside_none(op):
    """three waves and a part of one; in each, lanes with a 98-step h (the most rounds) alternate, in runs of
    one, two and three lanes, with lanes whose h < 2^128 takes no round at all"""
    long_h, small = LC.longest(), LC.small()
    assert len(D.euclid_quotients(long_h)) == 98
    hs = []
    for i in range(64 * 3 + 17):
        hs.append(long_h if (i // (1 + i // 64 % 3)) % 2 == 0 else small[i % len(small)])
    assert all(any(h == long_h for h in hs[w:w + 64]) and any(h < 2 ** 128 for h in hs[w:w + 64])
               for w in range(0, len(hs), 64))
    inp = _rows(op, hs)
    dev, host = _dev(op, inp), D.host_run(op, inp)
    assert (dev == host).all()
    D.check(op, inp, dev)


# ------------------------------------------------------------ kernel level
N_SIG = 65 * 64


@pytest.fixture
def nat():
    """the binding with every tuning knob restored and the key cache cleared afterwards"""
    from plenum_gpu import _native as nat
    nat.ensure_init()
    nat.keycache_clear()
    saved = nat.get_tuning()
    try:
        yield nat
    finally:
        nat.set_tuning(**saved)
        nat.keycache_clear()


@pytest.fixture(scope='module')
def signed():
    """(pk, sig, blob, off, oracle verdicts, host build's deferred count): 4,160
    signatures over 256-byte payloads by the oracle's signer, one in 61 tampered afterwards"""
    rnd = np.random.RandomState(7800)
    seeds = rnd.randint(0, 256, (N_SIG, 32)).astype(np.uint8)
    blob = rnd.randint(0, 256, N_SIG * 256).astype(np.uint8)
    off = np.arange(N_SIG + 1, dtype=np.uint64) * 256
    pk, sig = orc.sign_batch(seeds, blob, off)
    sig[::61, 40] ^= 1                               # S changed: rejected by the curve equation
    want = orc.verify_batch(pk, sig, blob, off).astype(bool)
    assert want.sum() == N_SIG - len(range(0, N_SIG, 61))
    # the host build's deferred count: its half_scalars on h = SHA-512(R || A || M) mod L of every row (all of
    # them pass the pre-checks: honest keys and R, S < L)
    hc = LC.hc()
    c, d, neg = ctypes.create_string_buffer(20), ctypes.create_string_buffer(20), ctypes.c_uint32()
    nd = 0
    for i in range(N_SIG):
        h = orc.hram(sig[i].tobytes(), pk[i].tobytes(), blob[256 * i:256 * i + 256].tobytes())
        assert int.from_bytes(h, 'little') < D.L
        nd += hc.hc_half_scalars(h, c, d, ctypes.byref(neg)) == D.HS_DEFER
    assert nd >= 1
    return pk, sig, blob, off, want, nd


def test_three_kernels(nat, signed):
    """k_hash + k_lattice + k_curve_half (host buffers, unfused): oracle verdicts, the host build's deferred count"""
    pk, sig, blob, off, want, nd = signed
    nat.set_lat_max(0)
    nat.set_host_fused(False)
    got = np.asarray(nat.verify_batch_arrays(pk, sig, blob, off, dedup_keys=False)).astype(bool)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    mode, deferred = nat.curve_stats(0)
    print('deferred: device {}, host build {}'.format(deferred, nd))
    assert mode == 'half' and deferred == nd


def test_fused_chunk_kernel(nat, signed):
    """k_chunk_half, its deferred records through the list kernel"""
    pk, sig, blob, off, want, nd = signed
    nat.set_lat_max(0)
    got = np.asarray(nat.verify_batch_arrays(pk, sig, blob, off, dedup_keys=False)).astype(bool)
    assert (got == want).all(), np.nonzero(got != want)[0][:8]
    assert nat.curve_stats(0)[0] == 'half'


@pytest.mark.parametrize('n', [1, 65])
def test_small_batch_kernel(nat, signed, n):
    """k_verify_quad at n = 1 (a valid row) and 65 (rows 30..94, the tampered row 61 among them)"""
    pk, sig, blob, off, want, nd = signed
    s = 62 if n == 1 else 30
    b = blob[int(off[s]):int(off[s + n])]
    o = (off[s:s + n + 1] - off[s]).astype(np.uint64)
    got = np.asarray(nat.verify_batch_arrays(np.ascontiguousarray(pk[s:s + n]), np.ascontiguousarray(sig[s:s + n]),
                                             np.ascontiguousarray(b), o)).astype(bool)
    assert (got == want[s:s + n]).all() and got.all() == (n == 1)
    assert nat.curve_stats(0)[0] == 'half'
