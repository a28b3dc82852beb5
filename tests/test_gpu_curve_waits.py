"""k_curve_half / k_chunk_half at the wave-task edges, against the oracle.

The throughput curve kernel is a persistent grid whose waves take tasks of 64
signatures from a queue and issue their table reads ahead of use; work on its
memory waits (tools/ab/curve_half_*_notadopted.patch: per-lane
digit words in LDS, reads issued one stage earlier, the task's inputs in one
round trip) must leave every verdict as it is.  Batch sizes 1, 63, 64, 65,
127, 128, 129 and 64*9 + 1 are the task edges (one lane, one short of a wave,
exactly one, one over, ... and a wave that runs several tasks in a row), taken
from fixtures that hold non-decodable A and R and non-canonical R, so rejected
lanes sit beside accepted ones.  Every batch runs through
pv_verify_batch_device (k_curve_half) and once through the host-buffer path
(k_chunk_half), with the latency kernels switched off so that the throughput
kernels run at these sizes."""
import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 64 * 9 + 1)


@pytest.fixture(scope='module')
def half_mode():
    """curve mode 'half' with the latency kernels off: every batch size takes
    k_curve_half (device buffers) / k_chunk_half (host buffers)"""
    import torch
    assert torch.cuda.is_available()
    from plenum_gpu import _native as nat
    nat.ensure_init()
    nat.set_curve_mode('half')
    nat.set_lat_max(0)
    try:
        yield nat
    finally:
        nat.set_curve_mode('half')
        nat.set_lat_max(nat.LAT_MAX_DEFAULT)


def _soa_from_sm(adv):
    """adversarial fixture (pk, sig || msg) -> pk, sig, blob, off"""
    so = adv['sm_off'].astype(np.int64)
    k = len(adv['label'])
    sig = np.zeros((k, 64), np.uint8)
    msgs = []
    off = np.zeros(k + 1, np.uint64)
    for j in range(k):
        sm = adv['sm_blob'][so[j]:so[j + 1]]
        # a signed message shorter than a signature is rejected by every path
        # before the curve stage; pad its signature with zeros (S = 0, R = 0 ...)
        sig[j, :min(64, len(sm))] = sm[:64]
        msgs.append(sm[64:])
        off[j + 1] = off[j] + len(msgs[-1])
    blob = np.concatenate(msgs) if k else np.zeros(0, np.uint8)
    return np.ascontiguousarray(adv['pk'].reshape(k, 32)), sig, np.ascontiguousarray(blob, dtype=np.uint8), off


@pytest.fixture(scope='module')
def cases(raw_vectors, adversarial):
    """name -> (pk, sig, blob, off, oracle verdicts), each computed once"""
    out = {}
    r = raw_vectors
    out['raw'] = (r['pk'], r['sig'], r['blob'], r['off'].astype(np.uint64))
    out['adversarial'] = _soa_from_sm(adversarial)
    for name in list(out):
        pk, sig, blob, off = out[name]
        out[name] = (pk, sig, blob, off, orc.verify_batch(pk, sig, blob, off).astype(bool))
    return out


def _slice(case, start, n):
    """n signatures of a case from `start`, wrapping round its end"""
    pk, sig, blob, off, want = case
    total = pk.shape[0]
    idx = (start + np.arange(n)) % total
    lens = (off[1:] - off[:-1]).astype(np.int64)[idx]
    o = np.zeros(n + 1, np.uint64)
    o[1:] = np.cumsum(lens)
    b = np.concatenate([blob[int(off[i]):int(off[i + 1])] for i in idx]) if n else np.zeros(0, np.uint8)
    return (np.ascontiguousarray(pk[idx]), np.ascontiguousarray(sig[idx]), np.ascontiguousarray(b, dtype=np.uint8), o,
            want[idx])


def _device_verdicts(torch, pk, sig, blob, off):
    from plenum_gpu.device import verify_device
    n = pk.shape[0]
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    blob_p = np.concatenate([blob, np.zeros(16, np.uint8)])
    verdict = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    bitmap = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)   # the half path clears it itself
    verify_device(t(pk), t(sig), t(blob_p), t(off.astype(np.int64)), verdict, bitmap)
    v = verdict.cpu().numpy()
    assert set(np.unique(v)) <= {0, 1}
    bits = np.unpackbits(bitmap.cpu().numpy().view(np.uint8), bitorder='little')[:n].astype(bool)
    assert (bits == v.astype(bool)).all()
    return v.astype(bool)


@pytest.mark.parametrize('name', ['raw', 'adversarial'])
def test_device_path_task_edges(half_mode, cases, name):
    """pv_verify_batch_device (k_curve_half) == oracle at every task-edge size;
    each size starts at another row, so rejected rows meet every lane position"""
    import torch
    case = cases[name]
    assert not case[4].all() and case[4].any()     # the fixture holds both verdicts
    seen_reject = False
    for k, n in enumerate(SIZES):
        pk, sig, blob, off, want = _slice(case, 37 * k, n)
        got = _device_verdicts(torch, pk, sig, blob, off)
        assert (got == want).all(), (name, n, np.nonzero(got != want)[0][:8])
        mode, _ = half_mode.curve_stats(0)
        assert mode == 'half'
        seen_reject |= not want.all()
    assert seen_reject


@pytest.mark.parametrize('name', ['raw', 'adversarial'])
def test_host_path_task_edges(half_mode, cases, name):
    """the same batches through host buffers (k_chunk_half, one fused launch per chunk)"""
    case = cases[name]
    for k, n in enumerate(SIZES):
        pk, sig, blob, off, want = _slice(case, 37 * k, n)
        got = half_mode.verify_batch_arrays(pk, sig, blob, off, dedup_keys=False)
        assert (np.asarray(got).astype(bool) == want).all(), (name, n)


def test_all_deferred_beside_half(half_mode):
    """a synthetic batch with every record deferred to the full-length form
    (curve mode 'full': only k_curve_half's full-length tasks run) beside the
    same batch in 'half' mode, device and host buffers: identical verdicts"""
    import torch
    from plenum_gpu.device import SyntheticBatch
    nat = half_mode
    n = 64 * 9 + 1
    b = SyntheticBatch(0, n, 256, cfg=2, first=4242)
    tamper = b.tamper.cpu().numpy().astype(bool)
    pk, sig = b.pk.cpu().numpy(), b.sig.cpu().numpy()
    blob = b.blob.cpu().numpy()[:n * 256]
    off = np.arange(n + 1, dtype=np.uint64) * 256
    got = {}
    try:
        for mode in ('half', 'full'):
            nat.set_curve_mode(mode)
            b.bitmap.fill_(-1)
            got[mode] = b.verify().cpu().numpy().astype(bool)
            got_mode, deferred = nat.curve_stats(0)
            assert got_mode == mode
            if mode == 'full':
                assert deferred >= int((~tamper).sum())      # every record that reaches the curve stage
            bits = np.unpackbits(b.bitmap.cpu().numpy().view(np.uint8), bitorder='little')[:n].astype(bool)
            assert (bits == got[mode]).all(), mode
            got[mode + '_host'] = np.asarray(nat.verify_batch_arrays(pk, sig, blob, off, dedup_keys=False)).astype(bool)
    finally:
        nat.set_curve_mode('half')
    assert (got['half'] == got['full']).all()
    assert (got['half_host'] == got['half']).all() and (got['full_host'] == got['half']).all()
    assert (got['half'] == ~tamper).all()
    assert (got['half'] == orc.verify_batch(pk, sig, blob, off).astype(bool)).all()
