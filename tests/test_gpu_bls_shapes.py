"""The three BLS check kernels (k_bls_verify_pair / _quad / _oct, csrc/pv_bls.hip)
and the grouping pipeline under them on the cases of tests/_bls_cases.py: ragged
key segments with idle lane groups beside live ones, key sets on both sides of
GROUP_LOCAL_KEYS, both H(m) implementations at the edges of try-and-increment
and SHA-256 padding, point sums that pass through O, and the data generators on
edge scalars.  Every expected value is the C oracle's (tests/test_bls_cases.py
holds the case set's own conditions, on the CPU); the kernel is selected with
pv_tuning (bls_quad_max / bls_oct_max), restored afterwards."""
import contextlib

import numpy as np
import pytest

import _bls_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nat():
    from plenum_gpu import _native
    _native.ensure_init()
    return _native


@contextlib.contextmanager
def kernel(nat, name):
    prev = nat.set_tuning(**C.KERNELS[name])
    try:
        yield
    finally:
        nat.set_tuning(**prev)


def _verify_all_kernels(nat, c):
    """c's checks under each kernel against c['want']; the device key set must hold c['keys']"""
    bad = {}
    for name in C.KERNELS:
        with kernel(nat, name):
            got = nat.bls_verify_arrays(c['sig'], c['blob'], c['off'], c['midx'], c['kidx'])
        assert got.shape == c['want'].shape
        wrong = np.nonzero(got != c['want'].astype(bool))[0]
        if len(wrong):
            bad[name] = ['{} (got {:d})'.format(c['labels'][j], got[j]) for j in wrong]
    assert not bad, bad


def test_kernel_selection_is_restored(nat):
    before = nat.get_tuning()
    assert before['bls_oct_max'] > 0 and before['bls_quad_max'] > before['bls_oct_max']
    for name in C.KERNELS:
        with kernel(nat, name):
            t = nat.get_tuning()
            assert {k: t[k] for k in C.KERNELS[name]} == C.KERNELS[name]
        assert nat.get_tuning() == before


def test_ragged_key_segments(nat):
    """12 key entries with 1, 7, 8, 9, 15, 16, 17, 33, 3 (O), 3 (outside G2), 0 and
    31 checks, shuffled: all 143 verdicts, under every kernel"""
    c = C.ragged()
    st = nat.bls_set_keys(C.generator(), c['keys'])
    assert list(st) == C.RAGGED_STATUS
    assert len(c['want']) == 143
    _verify_all_kernels(nat, c)


@pytest.mark.parametrize('nkeys', [2048, 2049])
def test_key_sets_around_group_local_keys(nat, nkeys):
    """2048 entries keep the grouping kernels' LDS path with a full lc[]; 2049 take
    the global-atomic path"""
    c = C.keyset(nkeys)
    st = nat.bls_set_keys(C.generator(), c['keys'])
    assert st.shape == (nkeys,) and not st.any()
    _verify_all_kernels(nat, c)


def test_hash_one_lane_vs_oracle(nat):
    """k_bls_hash (hash_one) through the signer: 1 * H(m) for every message of the pool, byte for byte"""
    msgs = C.pool()
    blob, off = C.pack(msgs)
    one = np.frombuffer((1).to_bytes(32, 'big'), np.uint8).reshape(1, 32)
    got = nat.bls_sign_arrays(one, blob, off, np.arange(len(msgs), dtype=np.uint32), np.zeros(len(msgs), np.uint32))
    bad = [i for i, m in enumerate(msgs) if got[i].tobytes() != C.hash_to_g1(m)]
    assert not bad, bad


def test_hash_edges_under_every_kernel(nat):
    """hash_group (quad, octet) and k_bls_hash + k_bls_sigprep (pair) on messages
    that need 0..14 increments and on SHA-256's padding edges: 50 checks"""
    c = C.hash_checks()
    st = nat.bls_set_keys(C.generator(), c['keys'])
    assert list(st) == [0]
    _verify_all_kernels(nat, c)


def test_aggregate_sigs_through_infinity(nat):
    """k_bls_agg_g1: sums that reach O and go on (g1j_add_affine's inf = true re-entry)"""
    sets = C.aggregate_sets()
    flat = np.frombuffer(b''.join(b''.join(s) for s in sets), np.uint8).reshape(-1, 128)
    set_off = np.cumsum([0] + [len(s) for s in sets]).astype(np.uint64)
    got = nat.bls_aggregate_sigs(flat, set_off)
    for j, s in enumerate(sets):
        assert got[j].tobytes() == C.aggregate_sigs(s), j
    assert got[0].tobytes() == sets[0][2]
    # the same through the verifier drop-in's create_multi_sig
    from plenum_gpu.bls import (BlsCryptoVerifierGpu, BlsGroupParamsLoaderIndyCrypto, IndyCryptoBlsUtils,
                                MultiSignature, Signature)
    v = BlsCryptoVerifierGpu(BlsGroupParamsLoaderIndyCrypto().load_group_params())
    for s in sets:
        ms = v.create_multi_sig([IndyCryptoBlsUtils.bls_to_str(Signature(x)) for x in s])
        assert IndyCryptoBlsUtils.bls_from_str(ms, MultiSignature).as_bytes() == C.aggregate_sigs(s)


def test_verify_multi_key_sums_through_infinity(nat):
    """k_bls_agg_g2: the key lists [k, -k, k2] and [k, k, -k], a matching and a non-matching sigma each"""
    checks = C.multi_checks()
    blob, off = C.pack([c[1] for c in checks])
    sig = np.frombuffer(b''.join(c[0] for c in checks), np.uint8).reshape(-1, 128)
    pks = np.frombuffer(b''.join(b''.join(c[2]) for c in checks), np.uint8).reshape(-1, 128)
    pk_off = np.cumsum([0] + [len(c[2]) for c in checks]).astype(np.uint64)
    got = nat.bls_verify_multi_arrays(C.generator(), sig, blob, off, np.arange(len(checks), dtype=np.uint32), pks,
                                      pk_off)
    want = [C.verify_multi(*c) for c in checks]
    assert want == [1, 0, 1, 0]
    assert got.tolist() == [bool(w) for w in want]


def test_sign_and_pubkeys_edge_scalars(nat):
    """k_bls_sign and k_bls_pubkeys with the scalars 1, 2, r - 1, r + 1, 2^255 and 2^256 - 1 (taken unreduced)"""
    sks = [k.to_bytes(32, 'big') for k in C.EDGE_SCALARS]
    arr = np.frombuffer(b''.join(sks), np.uint8).reshape(-1, 32)
    pk = nat.bls_pubkeys(C.generator(), arr)
    for i, sk in enumerate(sks):
        assert pk[i].tobytes() == C.pubkey(sk), hex(C.EDGE_SCALARS[i])
    msgs = [C.pool()[j] for j in (0, 9, 13, 16)]        # 0, 9 and 14 increments; 55 bytes
    blob, off = C.pack(msgs)
    midx = np.repeat(np.arange(len(msgs), dtype=np.uint32), len(sks))
    kidx = np.tile(np.arange(len(sks), dtype=np.uint32), len(msgs))
    sig = nat.bls_sign_arrays(arr, blob, off, midx, kidx)
    for j in range(len(midx)):
        assert sig[j].tobytes() == C.sign(sks[kidx[j]], msgs[midx[j]]), (int(midx[j]), hex(C.EDGE_SCALARS[kidx[j]]))
