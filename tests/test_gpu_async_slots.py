"""Two DISTINCT batches in flight on the async verify slots
(pv_*_device_async, workspaces 0 / 1; pairs and checker: tests/_async_cases.py).

What orders two batches in flight is host code of the C-ABI layer: the
workspaces and their `done` events (ws_begin / ws_end / WsUse), the side
stream of the key preparation (kside / kfork / kjoin), the two key scratches,
the staged bitmap and the regrowth of a workspace buffer under a queued
kernel.  A missing wait or a shared buffer there makes one slot compute from
the other slot's batch; with the same batch in both slots that still gives
the expected bytes.  Here the two batches of a pair differ in every bitmap
word, every output is filled with a sentinel before a schedule and compared
with the expectation of its OWN batch after one torch.cuda.synchronize().

Expectations are exact: the synth spec (expected_tamper), libsodium on a
sample (the oracle) and the recorded raw-vector fixture."""
import ctypes
import threading

import numpy as np
import pytest

import _async_cases as ac
import _oracle as orc

pytestmark = pytest.mark.gpu

ROUNDS = 3


@pytest.fixture(scope='module')
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


class Built:
    """One parameter set's batch, built and checked synchronously once per module."""

    def __init__(self, torch, p):
        from plenum_gpu import _native as nat
        self.p = p
        self.want = ac.expected_outputs(p)
        self.b = b = ac.make_batch(p)
        self.keyed = ac.is_keyed(p)
        tamper = ac.expected_tamper(p)
        assert (b.tamper.cpu().numpy().astype(bool) == tamper).all()
        b.verdict.fill_(ac.SENTINEL_VERDICT)
        b.bitmap.fill_(ac.SENTINEL_WORD)
        if self.keyed:   # padding words of the tables are never written
            b.ktab.fill_(-1)
        torch.cuda.synchronize()
        v = b.verify().cpu().numpy()
        assert (v.astype(bool) == ~tamper).all()
        assert ac.check_outputs(v, b.bitmap.cpu().numpy(), self.want) is None
        # the key table of the synchronous preparation / the deferred count of the generic batch
        self.want_tab = b.ktab.clone() if self.keyed else None
        self.deferred = None if self.keyed else nat.curve_stats(b.device.index)[1]
        # 200 sampled signatures against libsodium
        idx = np.sort(np.random.default_rng(p.first % 1000 + p.n).choice(p.n, 200, replace=False))
        it = torch.from_numpy(idx).to(b.device)
        off = b.off.cpu().numpy().astype(np.uint64)
        msgs = [b.blob[int(off[i]):int(off[i + 1])].cpu().numpy() for i in idx]
        soff = np.zeros(len(idx) + 1, np.uint64)
        soff[1:] = np.cumsum([len(m) for m in msgs])
        got = orc.verify_batch(b.pk[it].cpu().numpy(), b.sig[it].cpu().numpy(), np.concatenate(msgs), soff)
        assert (got == v[idx].astype(bool)).all()
        assert got.any() and not got.all()

    def fill(self, slots=(0, 1)):
        """sentinel in the slot's outputs (and -1 in its key table)"""
        for slot in slots:
            v, bm, kt = self.b.slot_out[slot]
            v.fill_(ac.SENTINEL_VERDICT)
            bm.fill_(ac.SENTINEL_WORD)
            if kt is not None:
                kt.fill_(-1)

    def check(self, torch, slot, what=''):
        """the slot's outputs against this batch's own expectation"""
        v, bm, kt = self.b.slot_out[slot]
        d = ac.check_outputs(v.cpu().numpy(), bm.cpu().numpy(), self.want)
        assert d is None, (what, 'slot', slot, 'n', self.p.n, d)
        if self.keyed:
            assert torch.equal(kt, self.want_tab), (what, 'key table of slot', slot, 'n', self.p.n)


@pytest.fixture(scope='module')
def built(torch_dev):
    cache = {}

    def get(p):
        if p not in cache:
            cache[p] = Built(torch_dev, p)
        return cache[p]
    return get


@pytest.fixture(scope='module')
def streams(torch_dev):
    return [torch_dev.cuda.Stream(0), torch_dev.cuda.Stream(0)]


@pytest.mark.parametrize('p', ac.BATCHES, ids=ac.BATCH_NAMES.get)
def test_synchronous_baseline(built, p):
    """Before any schedule: the synchronous verify() of every batch gives
    ~tamper, the device tamper flags are the spec's, and 200 sampled
    signatures agree with libsodium (all asserted while the batch is built)."""
    x = built(p)
    assert x.b.n == p.n and x.keyed == (x.b.keys is not None)


def _alternate(torch, a, b, streams, beside=True, rounds=ROUNDS, first=0):
    """(a) a on (slot 0, stream 0) and b on (slot 1, stream 1), `rounds` times,
    nothing waited for in between; `first` = 1 enqueues b's pass first."""
    a.fill((0,))
    b.fill((1,))
    torch.cuda.synchronize()
    jobs = [(a, 0), (b, 1)]
    for _ in range(rounds):
        for x, slot in (jobs if first == 0 else jobs[::-1]):
            x.b.verify_async(slot, streams[slot], keys_beside=beside)
    torch.cuda.synchronize()
    a.check(torch, 0, 'alternating')
    b.check(torch, 1, 'alternating')


ALTERNATING = [('generic', True, 'half'), ('generic', True, 'full'), ('generic', True, 'grouped'),
               ('keyed', True, 'half'), ('keyed', False, 'half'), ('wide', True, 'half'), ('wide', False, 'half'),
               ('mixed', True, 'half'), ('mixed', False, 'half'), ('small_beside_large', True, 'half')]


@pytest.mark.parametrize('pair,beside,mode', ALTERNATING)
def test_alternating_slots(torch_dev, built, streams, pair, beside, mode):
    """Schedule (a): A on slot 0 / stream 0, B on slot 1 / stream 1, three
    rounds in flight.  Keyed pairs prepare their keys beside the hash stage
    (side stream) and in line; the generic pair also runs with every record
    through its full-length form and through the grouped kernel."""
    from plenum_gpu import _native as nat
    a, b = (built(p) for p in ac.PAIRS[pair])
    try:
        nat.set_curve_mode(mode)
        _alternate(torch_dev, a, b, streams, beside)
        if mode != 'half':
            assert nat.curve_stats(0)[0] == mode
    finally:
        nat.set_curve_mode('half')


@pytest.mark.parametrize('first', [0, 1])
def test_curve_stats_name_the_last_batch(torch_dev, built, streams, first):
    """(e) pv_curve_stats reports the deferred count of the generic batch
    enqueued LAST, whichever slot it ran on: A's after (B, A) rounds, B's
    after (A, B) rounds.  The two counts differ (read after each batch's
    synchronous pass), so the other slot's counter cannot pass for it."""
    from plenum_gpu import _native as nat
    a, b = (built(p) for p in ac.PAIRS['generic'])
    assert a.deferred != b.deferred, 'pick another `first`: the deferred counts must differ'
    assert 0 < a.deferred < a.p.n // 100 and 0 < b.deferred < b.p.n // 100    # ~0.2 % of random h
    _alternate(torch_dev, a, b, streams, first=first)
    last = a if first == 1 else b
    assert nat.curve_stats(0) == ('half', last.deferred)
    # and a synchronous pass afterwards names itself
    other = b if first == 1 else a
    other.b.verify()
    assert nat.curve_stats(0) == ('half', other.deferred)


@pytest.mark.parametrize('pair,beside', [('generic', True), ('keyed', True), ('keyed', False)])
@pytest.mark.parametrize('first', ['A', 'B'])
def test_one_slot_two_streams(torch_dev, built, streams, pair, beside, first):
    """Schedule (b): both batches through slot 0, A on stream 0 and B on stream
    1, twice each, every batch with output buffers of its own: the slot's
    `done` event is all that orders them.  Starting with B, the engine is shut
    down and initialised again first, so the SMALL batch sizes the fresh
    workspace and A regrows h / hrec / dlist and the key scratch while B is
    still queued."""
    torch = torch_dev
    from plenum_gpu import _native as nat
    a, b = (built(p) for p in ac.PAIRS[pair])
    order = [(a, 0), (b, 1)] if first == 'A' else [(b, 1), (a, 0)]
    if first == 'B':
        torch.cuda.synchronize()
        nat.shutdown()
        nat.ensure_init(1)
    a.fill((0,))
    b.fill((0,))
    torch.cuda.synchronize()
    for _ in range(2):
        for x, s in order:
            x.b.verify_async(0, streams[s], keys_beside=beside)
    torch.cuda.synchronize()
    a.check(torch, 0, 'one slot')
    b.check(torch, 0, 'one slot')


def _tiled(r, times):
    """the raw-vector fixture `times` times over: large enough for the host
    pipeline's chunks (>= 32,768 signatures each) to alternate over both workspaces"""
    n = len(r['pk'])
    blob = r['blob'][:int(r['off'][n])]
    off = np.concatenate([r['off'][:n] + np.uint64(k * len(blob)) for k in range(times)] +
                         [np.array([times * len(blob)], np.uint64)])
    return (np.tile(r['pk'], (times, 1)), np.tile(r['sig'], (times, 1)), np.tile(blob, times), off,
            np.tile(r['verdict'], times).astype(bool))


def test_synchronous_calls_in_between(torch_dev, built, streams, raw_vectors):
    """Schedule (c): with A in flight on (slot 1, stream 1), enqueued twice and
    never waited for, B's synchronous verify() (slot 0, device stream), then
    the host-buffer pv_verify_batch over the raw-vector fixture (one staged
    launch on workspace 0) and over its first 9 rows (the zero-copy route).
    The fixture's 3,000 rows fit one latency launch, so the fixture tiled 24
    times follows: 72,000 signatures in two pipeline chunks, one per
    workspace, through the prepared-key chunks (keys repeat: dedup) and the
    fused generic chunks.  A is enqueued again before each host call, so the
    call finds workspace 1 held by a caller's stream.  Every host call equals
    the fixture's verdicts, B its spec, and after the synchronize A its spec."""
    torch = torch_dev
    from plenum_gpu import _native as nat
    a, b = (built(p) for p in ac.PAIRS['generic'])
    r = raw_vectors
    want = r['verdict'].astype(bool)
    n = len(want)
    assert 2048 < n <= nat.LAT_MAX_DEFAULT        # above the zero-copy size, one latency launch
    tpk, tsig, tblob, toff, twant = _tiled(r, 24)
    a.fill((1,))
    b.fill((0,))
    torch.cuda.synchronize()

    def keep_a_in_flight():
        for _ in range(2):
            a.b.verify_async(1, streams[1])

    keep_a_in_flight()
    b.b.verify()
    b.check(torch, 0, 'sync beside async')
    keep_a_in_flight()
    got = nat.verify_batch_arrays(r['pk'], r['sig'], r['blob'], r['off'])
    assert (got == want).all()
    keep_a_in_flight()
    o = r['off'][:10]
    got = nat.verify_batch_arrays(r['pk'][:9], r['sig'][:9], r['blob'][:int(o[-1])], o)
    assert (got == want[:9]).all()
    assert want[:9].any() and not want.all()
    for dedup in (True, False):
        keep_a_in_flight()
        got = nat.verify_batch_arrays(tpk, tsig, tblob, toff, dedup_keys=dedup)
        bad = np.flatnonzero(got != twant)
        assert bad.size == 0, (dedup, bad[:8].tolist())
    torch.cuda.synchronize()
    a.check(torch, 1, 'async beside sync and host calls')


def test_verify_then_tally_on_one_stream(torch_dev, built, streams):
    """Schedule (d): per slot, verify_async and then tally_device_async on the
    same stream, the tally reading that slot's verdict tensor with no host wait
    in between; both slots in flight, two rounds.  Votes and quorum flags are
    the spec's (synth.c3_expected) of each slot's OWN batch: 25 nodes in slot
    0, 16 in slot 1."""
    torch = torch_dev
    from plenum_gpu import synth
    from plenum_gpu.device import tally_device_async
    from plenum_gpu.quorums import Quorums
    pair = [built(p) for p in ac.PAIRS['wide']]
    outs = []
    for slot, x in enumerate(pair):
        b0, nb = ac.commit_batches(x.p)
        dev = x.b.device
        outs.append((torch.arange(nb + 1, dtype=torch.int64, device=dev) * x.p.n_nodes,
                     torch.full((nb,), -1, dtype=torch.int32, device=dev),
                     torch.full((nb,), 7, dtype=torch.uint8, device=dev),
                     torch.zeros(1, dtype=torch.int32, device=dev)))
        x.fill((slot,))
    torch.cuda.synchronize()
    for _ in range(2):
        for slot, x in enumerate(pair):
            boff, votes, reached, bad = outs[slot]
            v, _ = x.b.verify_async(slot, streams[slot])
            tally_device_async(v, x.b.sender, boff, x.p.n_nodes, Quorums(x.p.n_nodes).commit.value, votes, reached,
                               bad, stream=streams[slot])
    torch.cuda.synchronize()
    assert (Quorums(25).commit.value, Quorums(16).commit.value) == (17, 11)
    for slot, x in enumerate(pair):
        x.check(torch, slot, 'verify then tally')
        b0, nb = ac.commit_batches(x.p)
        _, votes, reached, bad = outs[slot]
        want_votes, want_reached = synth.c3_expected(b0, nb, x.p.n_nodes, Quorums(x.p.n_nodes).commit.value)
        assert int(bad.item()) == 0
        assert (votes.cpu().numpy() == want_votes.astype(np.int32)).all(), slot
        assert (reached.cpu().numpy() == want_reached.astype(np.uint8)).all(), slot
        assert 0.1 < want_reached.mean() < 0.95


def test_two_host_threads(torch_dev, built):
    """(f) Two host threads (ctypes releases the GIL), each with one batch of
    the generic pair, one slot and one stream: 10 x (verify_async,
    stream.synchronize(), check).  After every fifth pass thread 0 makes a
    refused call (slot 2) and reads ITS pv_last_error; in the same iteration
    thread 1 finds its own last error still the null-buffer refusal it
    provoked before the loop."""
    torch = torch_dev
    from plenum_gpu import _native as nat
    from plenum_gpu.device import _p
    lib = nat.load()
    pair = [built(p) for p in ac.PAIRS['generic']]
    for slot, x in enumerate(pair):
        x.fill((slot,))
    torch.cuda.synchronize()
    errors = []
    meet = threading.Barrier(2)

    def refused(x, s, slot, pk):
        b = x.b
        v, bm, _ = b.slot_out[1]
        rc = lib.pv_verify_batch_device_async(pk, _p(b.sig), _p(b.blob), _p(b.off), b.n, _p(v), _p(bm),
                                              b.device.index, ctypes.c_void_p(s.cuda_stream), slot)
        assert rc != 0
        return lib.pv_last_error().decode()

    def work(slot):
        try:
            x = pair[slot]
            torch.cuda.set_device(x.b.device)
            s = torch.cuda.Stream(x.b.device)
            if slot == 1:
                assert refused(x, s, 1, ctypes.c_void_p(0)) == 'null device buffer'
            for k in range(10):
                with torch.cuda.stream(s):
                    x.fill((slot,))
                    x.b.verify_async(slot, s)
                    s.synchronize()
                    x.check(torch, slot, 'thread {} pass {}'.format(slot, k))
                if k % 5 == 4:
                    if slot == 0:
                        assert refused(x, s, 2, _p(x.b.pk)) == 'slot must be 0 or 1'
                        meet.wait(60)
                    else:
                        meet.wait(60)
                        assert lib.pv_last_error().decode() == 'null device buffer'
        except BaseException as e:   # noqa: B036 -- re-raised in the test
            errors.append((slot, e))
            meet.abort()

    threads = [threading.Thread(target=work, args=(slot,), daemon=True) for slot in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), 'a thread is still running after 120 s'
    for slot, e in errors:
        if not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert not errors, errors
