"""Every device-side form of SHA-512(R || A || M), and the signer's two hashes,
on the length / alignment grid of _hram_cases.py, against the oracle.

A valid signature verifies only if every byte of the hash is right, so each
test pushes the whole grid (every length 0..199, +-2 around every block and
padding edge up to 7 blocks, 1000..1025 and 4096; each at the four start
alignments; ~27 % of the rows made to fail) through ONE route of
csrc/pv_api.cpp and compares verdict by verdict.  The docstrings name the
routing conditions; where the library exposes an observable of the route
(pv_curve_stats, pv_kernel_timing's count of enqueue_verify launches,
pv_keycache_size) it is asserted, so a route that silently changed is seen.
The same grid runs through the host build in test_hram_cases.py."""
import numpy as np
import pytest

import _hram_cases as hcs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def grid():
    return hcs.build()


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
        nat.kernel_timing(0, False)
        nat.set_tuning(**saved)
        nat.keycache_clear()


def _same(route, c, got, want=None):
    want = c.want if want is None else want
    got = np.asarray(got).astype(bool)
    assert got.shape == want.shape, (route, got.shape)
    wrong = np.nonzero(got != want)[0]
    assert len(wrong) == 0, (route, len(wrong), hcs.describe(c, wrong))


def _launches(nat, fn):
    """fn() with the live timing on: (result, enqueue_verify launches it made)"""
    nat.kernel_timing(0, True)
    out = fn()
    return out, nat.kernel_timing(0, False)[2]


def _by_slices(nat, c, **kw):
    """the grid in calls of <= 256 rows that each start at a blob offset = 0 (mod 4)"""
    got = np.zeros(len(c.want), bool)
    slices = hcs.aligned_slices(c, 256)
    for s, e in slices:
        assert e - s <= 256 and int(c.off[s]) % 4 == 0
        got[s:e] = nat.verify_batch_arrays(*hcs.take(c, s, e), **kw)
    assert slices[0][0] == 0 and slices[-1][1] == len(c.want)
    assert all(a[1] == b[0] for a, b in zip(slices, slices[1:]))     # no row skipped
    return got, len(slices)


# ------------------------------------------------------------------ host buffers
def test_host_small_calls_schedule_lanes(nat, grid):
    """k_verify_quad<true> (schedule lanes + keyed_hash).  run_shard: m <=
    lat_max -> run_small; no key cached -> enqueue_verify; lat_fused (no ktab,
    mode != grouped, n <= lat_max) -> launch_verify_quad; n <= KQ_SMALL_MAX (256)."""
    (got, calls), k = _launches(nat, lambda: _by_slices(nat, grid))
    _same('k_verify_quad<true>', grid, got)
    assert k == calls and nat.curve_stats(0)[0] == 'half'


def test_host_one_call_hash_one(nat, grid):
    """k_verify_quad<false> (hash_one).  As above with n = the whole grid >
    KQ_SMALL_MAX, still <= lat_max (32768): one run_small call, one launch."""
    c = grid
    assert 256 < len(c.want) <= nat.LAT_MAX_DEFAULT
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off))
    _same('k_verify_quad<false>', c, got)
    assert k == 1 and nat.curve_stats(0)[0] == 'half'


def test_host_fused_chunk(nat, grid):
    """k_chunk_half, then k_verify_quad_list for its deferred records.
    lat_max = 0 keeps run_shard off run_small; without PV_FLAG_DEDUP_KEYS the
    shard is not keyed; host_fused (default) and mode != grouped -> `fused`:
    launch_chunk_half per chunk + one launch_verify_quad_list, none of them
    through enqueue_verify (0 timed launches)."""
    c = grid
    nat.set_lat_max(0)
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off, dedup_keys=False))
    _same('k_chunk_half', c, got)
    assert k == 0 and nat.curve_stats(0)[0] == 'half'


def test_host_unfused_wave_queue(nat, grid):
    """k_hash (wave queue, pre == nullptr) + k_lattice + k_curve_half.
    lat_max = 0, host_fused = 0: run_shard's chunks go through enqueue_verify;
    half (no ktab, mode half) -> launch_hash(pre = nullptr) + launch_lattice,
    and n > lat_max -> launch_curve_half."""
    c = grid
    nat.set_lat_max(0)
    nat.set_host_fused(False)
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off, dedup_keys=False))
    _same('k_hash + k_lattice + k_curve_half', c, got)
    assert k == 1 and nat.curve_stats(0)[0] == 'half'


def test_host_full_mode_list_kernel(nat, grid):
    """every record through k_verify_quad_list (hash_one per list entry).
    lat_max = 0, curve mode full: the fused chunk kernel defers every record
    (force_full) and the list pass verifies them all.  (pv_curve_stats reports no
    deferred count for the fused chunk path, so the mode and the absence of an
    enqueue_verify launch are what this route shows.)"""
    c = grid
    nat.set_lat_max(0)
    nat.set_curve_mode('full')
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off, dedup_keys=False))
    _same('k_verify_quad_list (full)', c, got)
    assert k == 0 and nat.curve_stats(0)[0] == 'full'


def test_host_grouped_mode_prechecked_hash(nat, grid):
    """k_precheck + k_hash with `pre` + k_curve.  Curve mode grouped rules out
    run_small and `fused`; enqueue_verify with half == false ->
    launch_hash(pre = w.pre) + launch_curve.  The grid's first 64 rows fail the
    pre-checks, so the wave that takes indices 0..63 starts with nothing to hash."""
    c = grid
    assert (c.tamper[:64] == 'precheck').all()
    nat.set_lat_max(0)
    nat.set_curve_mode('grouped')
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off, dedup_keys=False))
    _same('k_precheck + k_hash(pre) + k_curve', c, got)
    assert k == 1 and nat.curve_stats(0)[0] == 'grouped'


def test_host_cached_keys_small_calls(nat, grid):
    """k_verify_quad_keyed<true, 4>.  run_small with every key in the device
    key cache: nk = m, ng = 0 -> launch_verify_quad_keyed with a list, and
    n <= KQ_SMALL_MAX -> the 4-signature block form; not through enqueue_verify."""
    c = grid
    nat.keycache_add(c.pk)
    assert nat.keycache_size() == hcs.N_SEEDS
    (got, _), k = _launches(nat, lambda: _by_slices(nat, c))
    _same('k_verify_quad_keyed<true,4>', c, got)
    assert k == 0


def test_host_cached_keys_one_call(nat, grid):
    """k_verify_quad_keyed<true, 8>: as above in one call of n > KQ_SMALL_MAX."""
    c = grid
    nat.keycache_add(c.pk)
    assert nat.keycache_size() == hcs.N_SEEDS
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off))
    _same('k_verify_quad_keyed<true,8>', c, got)
    assert k == 0


def test_host_half_cached_keys_one_call(nat, grid):
    """keyed list kernel + k_verify_quad_list in one call: every other key of
    the pool cached, so run_small lists the cached rows for
    launch_verify_quad_keyed (nk > 256) and the others (ng > 0) for
    launch_verify_quad_list."""
    c = grid
    upk = np.unique(c.pk, axis=0)
    nat.keycache_add(upk[::2])
    assert nat.keycache_size() == (hcs.N_SEEDS + 1) // 2
    cached = (c.pk[:, None, :] == upk[None, ::2, :]).all(axis=2).any(axis=1)
    assert int(cached.sum()) > 256 and int((~cached).sum()) > 256
    got, k = _launches(nat, lambda: nat.verify_batch_arrays(c.pk, c.sig, c.blob, c.off))
    _same('k_verify_quad_keyed<true,8> + k_verify_quad_list', c, got)
    assert k == 0


# ---------------------------------------------------------------- device buffers
class _Dev:
    """the grid in device tensors; the blob with the 16 spare bytes msg_fetch may read"""

    def __init__(self, c):
        import torch
        self.torch = torch
        self.dev = dev = torch.device('cuda', 0)
        self.n = n = len(c.want)
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        upk, kidx = np.unique(c.pk, axis=0, return_inverse=True)
        self.k = len(upk)
        self.pk, self.sig = put(c.pk), put(c.sig)
        self.upk, self.kidx = put(upk), put(kidx.reshape(-1).astype(np.int32))
        self.blob = torch.zeros(int(c.off[-1]) + 16, dtype=torch.uint8, device=dev)
        self.blob[:int(c.off[-1])] = put(c.blob)
        assert self.blob.data_ptr() % 4 == 0
        self.off = put(c.off.astype(np.int64))
        self.verdict = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        self.bitmap = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev)

    def result(self):
        v = self.verdict.cpu().numpy()
        assert set(np.unique(v)) <= {0, 1}          # every row written
        bits = np.unpackbits(self.bitmap.cpu().numpy().view(np.uint8), bitorder='little')[:self.n]
        assert (bits == v).all(), 'bitmap != verdict bytes'
        return v.astype(bool)


def _keyed_device(nat, d, wide):
    from plenum_gpu.device import _p, _stream
    lib = nat.load()
    words = nat.PV_KEY_WORDS_WIDE if wide else nat.PV_KEY_WORDS
    ktab = d.torch.empty(d.k * words, dtype=d.torch.int32, device=d.dev)
    w = '_wide' if wide else ''
    fp, fv = 'pv_keys_prepare{}_device'.format(w), 'pv_verify_keyed{}_device'.format(w)
    nat._check(fp, getattr(lib, fp)(_p(d.upk), d.k, _p(ktab), 0, _stream(d.dev)))
    nat._check(fv, getattr(lib, fv)(_p(ktab), _p(d.kidx), _p(d.upk), _p(d.sig), _p(d.blob), _p(d.off), d.n,
                                    _p(d.verdict), _p(d.bitmap), 0, _stream(d.dev)))
    return d.result()


def test_device_generic_wave_queue(nat, grid):
    """k_hash with pre == nullptr on caller's device buffers.  verify_device ->
    enqueue_verify; lat_max = 0 -> not lat_fused; half -> launch_hash(pre =
    nullptr) + launch_lattice + launch_curve_half."""
    from plenum_gpu.device import verify_device
    d = _Dev(grid)
    nat.set_lat_max(0)

    def run():
        verify_device(d.pk, d.sig, d.blob, d.off, d.verdict, d.bitmap)
        return d.result()
    got, k = _launches(nat, run)
    _same('device: k_hash + k_lattice + k_curve_half', grid, got)
    assert k == 1 and nat.curve_stats(0)[0] == 'half'


def test_device_keyed_latency_kernel(nat, grid):
    """k_verify_quad_keyed<false, 8>.  pv_verify_keyed_device -> lat_keyed (ktab,
    not wide, n <= lat_keyed_max = 8192) -> launch_verify_quad_keyed without a
    list, key bytes by key index."""
    d = _Dev(grid)
    assert d.n <= nat.get_tuning()['lat_keyed_max'] == nat.LAT_KEYED_MAX_DEFAULT
    got, k = _launches(nat, lambda: _keyed_device(nat, d, wide=False))
    _same('device: k_verify_quad_keyed<false,8>', grid, got)
    assert k == 1 and d.k == hcs.N_SEEDS


def test_device_keyed_throughput_kernel(nat, grid):
    """k_precheck + k_hash with kidx + the keyed k_curve.  lat_keyed_max = 0 ->
    not lat_keyed; ktab -> half == false: launch_hash(pre, kidx) + launch_curve(ktab)."""
    d = _Dev(grid)
    nat.set_lat_keyed_max(0)
    got, k = _launches(nat, lambda: _keyed_device(nat, d, wide=False))
    _same('device: k_hash(kidx) + keyed k_curve', grid, got)
    assert k == 1


def test_device_keyed_wide(nat, grid):
    """k_hash + the wide (radix-256) keyed curve.  pv_keys_prepare_wide_device +
    pv_verify_keyed_wide_device: wide -> never lat_keyed, whatever lat_keyed_max."""
    d = _Dev(grid)
    got, k = _launches(nat, lambda: _keyed_device(nat, d, wide=True))
    _same('device: k_hash(kidx) + wide keyed k_curve', grid, got)
    assert k == 1


# ------------------------------------------------------------------------ signer
def test_signer_on_the_grid(nat, grid):
    """k_sign (sha512_prefixed / msg_bytes8: az-prefix || M and R || A || M) on the
    untampered grid == the oracle's keys and signatures, byte for byte"""
    c = grid
    pk, sig = nat.sign_batch_arrays(c.seeds, c.clean_blob, c.off)
    wrong = np.nonzero((pk != c.pk).any(axis=1) | (sig != c.clean_sig).any(axis=1))[0]
    assert len(wrong) == 0, ('k_sign', len(wrong), hcs.describe(c, wrong))
