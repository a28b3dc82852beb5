"""Batched SHA3-256 and state-proof verification on the GPU (pv_sha3_256_batch,
pv_state_proof_verify, plenum_gpu.state_proofs) against hashlib, the reference
fixture tests/golden/state_proofs.json and the same routines built for the host
(tools/hostcheck/stateproofcheck.cpp)."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import _state_proofs as sp

pytestmark = pytest.mark.gpu

PV_EINVAL = -22
BOUNDARY = [0, 1, 135, 136, 137, 271, 272, 273, 407, 408, 1000]


@pytest.fixture(scope='module')
def rows():
    return sp.fixture()


@pytest.fixture(scope='module')
def nat():
    from plenum_gpu import _native
    _native.ensure_init()
    return _native


@pytest.fixture(scope='module')
def packed(rows):
    """every fixture row in one call, and the host build's statuses for it"""
    pk = sp.Packed(rows, sp.host_split)
    return pk, sp.host_statuses(pk)


@pytest.fixture
def all_gpu(monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    return state_proofs


def _sha3(nat, msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs])
    blob = np.frombuffer(b''.join(msgs), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    out = np.full((len(msgs), 32), 0xee, np.uint8)
    rc = nat.load().pv_sha3_256_batch(sp.ptr(blob), sp.ptr(off), len(msgs), sp.ptr(out))
    assert rc == 0, nat.load().pv_last_error()
    return [out[i].tobytes() for i in range(len(msgs))]


def _verify(nat, pk):
    st = np.full(pk.Q, 0xee, np.uint8)
    rc = nat.load().pv_state_proof_verify(sp.ptr(pk.blob), pk.blob_len, sp.ptr(pk.beg), sp.ptr(pk.end),
                                          sp.ptr(pk.first), sp.ptr(pk.roots), sp.ptr(pk.pidx), sp.ptr(pk.keys),
                                          sp.ptr(pk.koff), sp.ptr(pk.vals), sp.ptr(pk.voff), pk.N, pk.P, pk.Q,
                                          sp.ptr(st))
    assert rc == 0, nat.load().pv_last_error()
    return st


def test_sha3_boundary_lengths_back_to_back(nat):
    rng = random.Random(11)
    msgs = [bytes(rng.getrandbits(8) for _ in range(n)) for n in BOUNDARY + [2] + BOUNDARY + [1] + BOUNDARY[::-1]]
    starts = {}
    for i, m in enumerate(msgs):
        starts.setdefault(len(m), set()).add(sum(len(x) for x in msgs[:i]) % 4)
    assert all(len(starts[n]) >= 2 for n in BOUNDARY) and set().union(*starts.values()) == {0, 1, 2, 3}
    assert _sha3(nat, msgs) == [hashlib.sha3_256(m).digest() for m in msgs]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_sha3_ragged_batches(nat, n):
    rng = random.Random(n)
    msgs = [rng.randbytes(rng.randint(0, 700)) for _ in range(n)]
    assert _sha3(nat, msgs) == [hashlib.sha3_256(m).digest() for m in msgs]


def test_sha3_empty_batch_and_bad_offsets(nat):
    out = np.full(64, 0xee, np.uint8)
    off = np.zeros(1, np.uint64)
    assert nat.load().pv_sha3_256_batch(None, sp.ptr(off), 0, sp.ptr(out)) == 0
    blob = np.zeros(8, np.uint8)
    off = np.array([0, 4, 2], np.uint64)
    assert nat.load().pv_sha3_256_batch(sp.ptr(blob), sp.ptr(off), 2, sp.ptr(out)) == PV_EINVAL
    assert (out == 0xee).all()


def test_sha3_device_form(nat):
    import torch
    rng = random.Random(12)
    msgs = [rng.randbytes(rng.randint(0, 700)) for _ in range(300)] + [b'', rng.randbytes(1000)]
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    dev = torch.device('cuda:0')
    blob = torch.frombuffer(bytearray(b''.join(msgs) + b'\0' * 16), dtype=torch.uint8).to(dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    out = torch.zeros(len(msgs) * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = nat.load().pv_sha3_256_batch_device(blob.data_ptr(), doff.data_ptr(), len(msgs), out.data_ptr(), 0, None)
    assert rc == 0, nat.load().pv_last_error()
    got = out.cpu().numpy().reshape(-1, 32)
    assert [got[i].tobytes() for i in range(len(msgs))] == [hashlib.sha3_256(m).digest() for m in msgs]
    assert got.tobytes() == b''.join(_sha3(nat, msgs))
    # a blob that is not 4-byte aligned is refused before any launch
    out.fill_(0xee)
    torch.cuda.synchronize()
    rc = nat.load().pv_sha3_256_batch_device(blob.data_ptr() + 1, doff.data_ptr(), 4, out.data_ptr(), 0, None)
    assert rc == PV_EINVAL and bool((out == 0xee).all())


def test_all_fixture_rows_in_one_call(nat, rows, packed):
    pk, host = packed
    assert pk.Q > 1000 and pk.P > 900 and len({r.trie for r in rows}) >= 5
    assert any(q is not None and q[1] > 1 for q in pk.row_queries)     # proofs shared by several queries
    st = _verify(nat, pk)
    assert (st == host).all(), np.nonzero(st != host)[0][:10]
    got = pk.verdicts(st)
    bad = [(r.trie, r.kind) for r, g in zip(rows, got) if g != r.expected]
    assert not bad, bad[:10]


@pytest.mark.parametrize('batch', [1, 64, 65])
def test_same_statuses_in_small_batches(nat, rows, packed, batch):
    pk, host = packed
    # every row at every batch size; one at a time that includes the empty proof with the
    # blank root alone in a call (N == 0: no node buffers, nothing hashed, only the walk)
    picked = rows
    alone_without_nodes = 0
    want = {id(r): host[q[0]:q[0] + q[1]] for r, q in zip(rows, pk.row_queries) if q is not None}
    for s in range(0, len(picked), batch):
        part = picked[s:s + batch]
        sub = sp.Packed(part, sp.host_split, pad_front=s % 4)
        if sub.Q == 0:
            continue
        alone_without_nodes += batch == 1 and sub.N == 0
        st = _verify(nat, sub)
        for r, q in zip(part, sub.row_queries):
            if q is not None:
                assert (st[q[0]:q[0] + q[1]] == want[id(r)]).all(), (r.trie, r.kind)
    assert alone_without_nodes == (2 if batch == 1 else 0)


def test_device_form_equals_host_form(nat, packed):
    import torch
    pk, host = packed
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else   # noqa: E731
                                   (a.view(np.int32) if a.dtype == np.uint32 else a)).to(dev)
    blob, beg, end, first, roots = t(pk.blob), t(pk.beg), t(pk.end), t(pk.first), t(pk.roots)
    pidx, keys, koff, vals, voff = t(pk.pidx), t(pk.keys), t(pk.koff), t(pk.vals), t(pk.voff)
    status = torch.full((pk.Q,), 0xee, dtype=torch.uint8, device=dev)
    dig = torch.zeros(pk.N * 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = nat.load().pv_state_proof_verify_device(
        blob.data_ptr(), beg.data_ptr(), end.data_ptr(), first.data_ptr(), roots.data_ptr(), pidx.data_ptr(),
        keys.data_ptr(), koff.data_ptr(), vals.data_ptr(), voff.data_ptr(), pk.N, pk.P, pk.Q, status.data_ptr(),
        dig.data_ptr(), 0, None)
    assert rc == 0, nat.load().pv_last_error()
    assert (status.cpu().numpy() == host).all()
    d = dig.cpu().numpy().reshape(-1, 32)
    raw = pk.blob.tobytes()
    for j in range(0, pk.N, 97):
        assert d[j].tobytes() == hashlib.sha3_256(raw[int(pk.beg[j]):int(pk.end[j])]).digest()


def test_einval_cases_leave_status_untouched(nat, rows):
    part = [r for r in rows if r.kind == 'own'][:6] + [r for r in rows if r.multi][:1]
    pk = sp.Packed(part, sp.host_split)

    def call(**kw):
        a = dict(beg=pk.beg, end=pk.end, first=pk.first, pidx=pk.pidx, koff=pk.koff, voff=pk.voff, N=pk.N, P=pk.P,
                 blob_len=pk.blob_len)
        a.update(kw)
        st = np.full(pk.Q, 0xee, np.uint8)
        rc = nat.load().pv_state_proof_verify(sp.ptr(pk.blob), a['blob_len'], sp.ptr(a['beg']), sp.ptr(a['end']),
                                              sp.ptr(a['first']), sp.ptr(pk.roots), sp.ptr(a['pidx']),
                                              sp.ptr(pk.keys), sp.ptr(a['koff']), sp.ptr(pk.vals), sp.ptr(a['voff']),
                                              a['N'], a['P'], pk.Q, sp.ptr(st))
        return rc, st

    rc, st = call()
    assert rc == 0 and (st == sp.OK).all()

    def bump(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    bad = {
        'key_off not monotone': dict(koff=bump(pk.koff, 2, int(pk.koff[3]) + 1)),
        'val_off not monotone': dict(voff=bump(pk.voff, 1, int(pk.voff[2]) + 5)),
        'node end past the blob': dict(end=bump(pk.end, pk.N - 1, pk.blob_len + 1)),
        'node begin past its end': dict(beg=bump(pk.beg, 0, int(pk.end[0]) + 1)),
        'blob shorter than the nodes': dict(blob_len=pk.blob_len - 1),
        'proof_first not monotone': dict(first=bump(pk.first, 1, int(pk.first[2]) + 1)),
        'proof_first does not end at N': dict(first=bump(pk.first, pk.P, pk.N - 1)),
        'proof_first past N': dict(first=bump(pk.first, pk.P, pk.N + 1)),
        'proof_idx == P': dict(pidx=bump(pk.pidx, 3, pk.P)),
        'proof_idx huge': dict(pidx=bump(pk.pidx, 0, 0xffffffff)),
    }
    for name, kw in bad.items():
        rc, st = call(**kw)
        assert rc == PV_EINVAL, name
        assert (st == 0xee).all(), name
        assert nat.load().pv_last_error(), name


def test_no_queries_succeeds(nat):
    z64 = np.zeros(1, np.uint64)
    st = np.full(4, 0xee, np.uint8)
    rc = nat.load().pv_state_proof_verify(None, 0, None, None, sp.ptr(z64), None, None, None, sp.ptr(z64), None,
                                          sp.ptr(z64), 0, 0, 0, sp.ptr(st))
    assert rc == 0 and (st == 0xee).all()


def test_rlp_split_list_entry_point(nat, rows):
    lib = nat.load()
    ser = next(r for r in rows if r.kind == 'own' and len(r.nodes) >= 4).serialized
    for data in (ser, ser[:-1], ser + b'\0', b'\xc0', b'\x80', b''):
        buf = np.frombuffer(data, np.uint8).copy() if data else np.zeros(1, np.uint8)
        beg, end = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
        count = ctypes.c_uint64(99)
        rc = lib.pv_rlp_split_list(sp.ptr(buf), len(data), sp.ptr(beg), sp.ptr(end), 64, ctypes.byref(count))
        want = sp.host_split(data)
        assert (rc == 0) == (want is not None)
        if want is not None:
            assert list(zip(beg[:count.value].tolist(), end[:count.value].tolist())) == want
        else:
            assert rc == PV_EINVAL
    buf = np.frombuffer(ser, np.uint8).copy()
    beg, end = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    count = ctypes.c_uint64(0)
    assert lib.pv_rlp_split_list(sp.ptr(buf), len(ser), sp.ptr(beg), sp.ptr(end), 2, ctypes.byref(count)) == PV_EINVAL


def test_python_verifier_on_the_gpu(all_gpu, rows):
    V = all_gpu.GpuStateVerifier
    picked = [r for r in rows if not r.multi][::60] + [r for r in rows if r.multi]
    for r in picked:
        if r.multi:
            assert V.verify_state_proof_multi(r.root, dict(r.kvs), r.serialized, serialized=True) == r.expected
            if not r.lenient:
                nodes = [sp.decode(n) for n in r.nodes]
                assert V.verify_state_proof_multi(r.root, dict(r.kvs), nodes) == r.expected
        else:
            k, v = r.kvs[0]
            assert V.verify_state_proof(r.root, k, v, r.serialized, serialized=True) == r.expected
            if not r.lenient and r.kind not in ('flipped', 'dropped'):
                assert V.verify_state_proof(r.root, k, v, [sp.decode(n) for n in r.nodes]) == r.expected
    items = [(r.root, dict(r.kvs), r.serialized) if r.multi else (r.root, r.kvs[0][0], r.kvs[0][1], r.serialized)
             for r in rows]
    items[5] = items[5][:3] + ([sp.decode(n) for n in rows[5].nodes],)     # one unserialized among them
    got = all_gpu.verify_state_proofs_batch(items)
    assert got.dtype == bool and got.tolist() == [r.expected for r in rows]
    r = next(r for r in rows if r.kind == 'own' and len(r.nodes) >= 3)
    without = [n for n in r.nodes if hashlib.sha3_256(n).digest() != r.root]
    assert V.verify_state_proof_multi(r.root, {}, r.serialized, serialized=True) is True       # no pairs: the root
    assert V.verify_state_proof_multi(r.root, {}, sp.serialize(without), serialized=True) is False   # node alone
    msgs = [bytes([i & 255]) * i for i in range(300)]
    assert all_gpu.sha3_256_batch(msgs) == [hashlib.sha3_256(m).digest() for m in msgs]
    assert all_gpu.sha3_256_batch([]) == []


def test_unsplittable_serialized_proof_is_false_on_the_gpu(all_gpu, rows):
    r = next(r for r in rows if r.kind == 'own')
    k, v = r.kvs[0]
    V = all_gpu.GpuStateVerifier
    assert V.verify_state_proof(r.root, k, v, r.serialized, serialized=True) is True
    assert V.verify_state_proof(r.root, k, v, r.serialized[:-1], serialized=True) is False
    assert V.verify_state_proof_multi(r.root, {k: v}, b'\x83abc', serialized=True) is False
    got = all_gpu.verify_state_proofs_batch([(r.root, k, v, r.serialized + b'\0'), (r.root, k, v, r.serialized)])
    assert got.tolist() == [False, True]
