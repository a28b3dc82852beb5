"""Reads from the resident trie node store on the GPU (pv_state_store_get[_device]: k_trie_get, the
scan, k_trie_get_copy) against the host build of the same header (tools/hostcheck/stategetcheck.cpp)
and the Python mirror, in both decode modes and through both entry points.  The scenarios are those
of tests/test_state_get_host.py (tests/_state_get.py): the smallest tries at which the walk, the
decode or the copy can go wrong."""
import ctypes

import numpy as np
import pytest

import _state_get as sg

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -22


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


@pytest.fixture(scope='module')
def wants():
    """the host build's answer to every scenario in both modes (checked against the mirror), once"""
    return {(name, dec): sg.run_host(sc, dec)[0] for name, sc in sg.scenarios().items() for dec in (False, True)}


def as_result(got):
    res = sg.Result(len(got.status))
    res.status, res.found, res.val_off, res.blob = got.status, got.found, got.val_off, got.blob
    return res


def device_get(st, roots, ridx, keys, decode, val_cap=None, sizing=False):
    """pv_state_store_get_device over device tensors -> (rc, Result)"""
    import torch
    from plenum_gpu import _native as nat
    lib = nat.load()
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)             # noqa: E731
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())           # noqa: E731
    n = len(keys)
    kblob, koff = sg.ss.pack(keys)
    d_roots = t(np.frombuffer(b''.join(roots), np.uint8).copy())
    d_ridx = None if ridx is None else t(np.asarray(ridx, np.int32))
    d_kblob, d_koff = t(kblob), t(koff.view(np.int64))
    status, found = (torch.full((n,), 0xee, dtype=torch.uint8, device=dev) for _ in range(2))
    voff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def call(vals, cap):
        return lib.pv_state_store_get_device(st._id, p(d_roots), p(d_ridx), len(roots), p(d_kblob), p(d_koff), n,
                                             int(decode), p(status), p(found), p(voff), p(vals), cap, None)
    rc = call(None, 0)
    res = sg.Result(n)
    total = int(voff[-1]) if rc == OK else 0
    if rc == OK and not sizing:
        vals = torch.zeros(max(total, 1), dtype=torch.uint8, device=dev)
        rc = call(vals, total if val_cap is None else val_cap)
        if rc == OK:
            res.blob = vals.cpu().numpy()[:total]
    res.status, res.found = status.cpu().numpy(), found.cpu().numpy()
    res.val_off = voff.cpu().numpy().view(np.uint64)
    return rc, res


@pytest.fixture(scope='module')
def stores(mod):
    """one resident store per distinct node set of the scenarios"""
    made = {}
    for name, sc in sg.scenarios().items():
        key = 'count' if name.startswith('count') else name
        if key not in made:
            st = mod.GpuStateStore(node_hint=1)
            for b in sc[0]:
                st.add_nodes(b)
            made[key] = st
    yield lambda name: made['count' if name.startswith('count') else name]
    for st in made.values():
        st.close()


# ------------------------------------------------------------------ GPU == host build == mirror
@pytest.mark.parametrize('name', sorted(sg.scenarios()))
@pytest.mark.parametrize('decode', [False, True], ids=['raw', 'decode'])
def test_host_entry(mod, stores, wants, name, decode):
    batches, roots, ridx, keys = sg.scenarios()[name]
    got = as_result(stores(name).get(roots, ridx, keys, decode))
    want = wants[name, decode]
    assert want.same(got) is None, want.same(got)


@pytest.mark.parametrize('name', sorted(sg.scenarios()))
@pytest.mark.parametrize('decode', [False, True], ids=['raw', 'decode'])
def test_device_entry(mod, stores, wants, name, decode):
    batches, roots, ridx, keys = sg.scenarios()[name]
    rc, got = device_get(stores(name), roots, ridx, keys, decode)
    assert rc == OK
    want = wants[name, decode]
    assert want.same(got) is None, want.same(got)


# ------------------------------------------------------------------ what the scenarios are about
def test_shapes_payloads_roots_and_hostile_values(mod, stores):
    from plenum_gpu.state_store import rlp_decode
    batches, roots, ridx, keys = sg.sc_shapes()
    got = stores('shapes').get(roots, ridx, keys, True)
    want = dict(sg.SHAPE_PAIRS)
    n = len(sg.SHAPE_PAIRS) + len(sg.SHAPE_ABSENT)
    assert [got.value(q) for q in range(n)] == [rlp_decode(want[k])[0] if k in want else None for k in keys[:n]]
    assert got.value(n) is not None and [got.value(q) for q in range(n + 1, len(keys))] == [None] * 6
    assert (got.status == sg.OK).all()

    batches, roots, ridx, keys = sg.sc_payloads()
    pls = sg.payloads()
    got = stores('payloads').get(roots, ridx, keys, True)
    assert [got.value(q) for q in range(len(pls))] == [p for _, p in pls]
    assert got.found.tolist() == [1] * len(pls) + [0] and got.value(0) == b''      # found, of length 0

    batches, roots, ridx, keys = sg.sc_roots()
    got = stores('roots').get(roots, ridx, keys, True)
    assert got.value(2) == sg._v(40, 62) and got.value(8) == b'new value'
    assert got.status[12:].tolist() == [sg.NODE_MISSING, sg.OK, sg.NODE_MISSING, sg.OK, sg.OK]

    batches, roots, ridx, keys = sg.sc_hostile()
    dec = stores('hostile').get(roots, ridx, keys, True)
    raw = stores('hostile').get(roots, ridx, keys, False)
    for i, v in enumerate(sg.HOSTILE_VALUES):
        assert raw.value(2 * i + 1) == v
        assert (dec.status[2 * i + 1], dec.found[2 * i + 1]) == (sg.MALFORMED, 0), v
        assert dec.status[2 * i] == sg.OK and dec.value(2 * i) == sg._v(20 + i, 40 + i)
    for i, (v, payload) in enumerate(sg.LENIENT_VALUES):
        assert dec.value(2 * len(sg.HOSTILE_VALUES) + i) == payload, v


def test_get_batch_raises_where_the_reference_does(mod, stores):
    batches, roots, ridx, keys = sg.sc_roots()
    st = stores('roots')
    assert st.get_batch([(roots[0], keys[2]), (roots[1], keys[2]), (roots[0], b'none')]) == \
        [sg._v(40, 62), b'new value', None]
    assert st.get_batch([(roots[1], keys[2])], decode=False) == [sg.enc(b'new value')]
    with pytest.raises(KeyError):
        st.get_batch([(roots[0], keys[0]), (b'\x11' * 32, keys[0])])
    batches, roots, ridx, keys = sg.sc_hostile()
    with pytest.raises(ValueError):
        stores('hostile').get_batch([(roots[0], keys[1])])
    assert st.get_batch([]) == []


def test_no_root_idx_means_root_q_for_query_q(mod, stores):
    batches, roots, ridx, keys = sg.sc_roots()
    st = stores('roots')
    got = st.get([roots[0], roots[1], roots[2]], None, [keys[2]] * 3, True)
    assert [got.value(q) for q in range(3)] == [sg._v(40, 62), b'new value', None]
    assert got.status.tolist() == [sg.OK, sg.OK, sg.NODE_MISSING]
    rc, dev = device_get(st, [roots[0], roots[1], roots[2]], None, [keys[2]] * 3, True)
    assert rc == OK and as_result(got).same(dev) is None


# ------------------------------------------------------------------ sizing, capacity, refusals
def test_sizing_call_capacity_and_refusals(mod, stores):
    from plenum_gpu import _native as nat
    lib = nat.load()
    batches, roots, ridx, keys = sg.sc_count(65)
    st = stores('count65')
    full = st.get(roots, ridx, keys, True)
    total = int(full.val_off[-1])
    assert total > 0

    def host_call(decode=1, vals=True, cap=None, koff=None, ridx_=ridx, n_roots=len(roots)):
        n = len(keys)
        kblob, ko = sg.ss.pack(keys)
        ko = ko if koff is None else koff
        rts = np.frombuffer(b''.join(roots), np.uint8).copy()
        ri = np.asarray(ridx_, np.uint32)
        res = sg.Result(n)
        blob = np.zeros(max(total, 1), np.uint8)
        ptr = lambda a: a.ctypes.data                                           # noqa: E731
        rc = lib.pv_state_store_get(st._id, ptr(rts), ptr(ri), n_roots, ptr(kblob), ptr(ko), n, decode,
                                    ptr(res.status), ptr(res.found), ptr(res.val_off), ptr(blob) if vals else None,
                                    total if cap is None else cap)
        return rc, lib.pv_last_error().decode(), res

    rc, _, res = host_call(vals=False)                                          # the sizing call
    assert rc == OK and (res.val_off == full.val_off).all() and (res.found == full.found).all()
    rc, text, res = host_call(cap=total - 1)
    assert rc == EINVAL and text == 'val_cap {} is below the {} bytes of the values'.format(total - 1, total)
    assert (res.val_off == full.val_off).all() and (res.status == full.status).all()      # already written
    assert host_call(decode=2)[:2] == (EINVAL, 'decode must be 0 or 1')
    assert host_call(decode=-1)[:2] == (EINVAL, 'decode must be 0 or 1')
    bad = sg.ss.pack(keys)[1].copy()
    bad[3] = bad[2] - 1
    assert host_call(koff=bad)[:2] == (EINVAL, 'key_off not monotone at 2')
    assert host_call(ridx_=[0] * 64 + [1])[:2] == (EINVAL, 'root_idx[64] = 1 is not below n_roots 1')
    assert host_call(n_roots=0)[:2] == (EINVAL, 'queries without roots')
    assert lib.pv_state_store_get(12345, None, None, 0, None, None, 0, 0, None, None, None, None, 0) == EINVAL
    assert lib.pv_last_error() == b'no state store with id 12345'
    assert lib.pv_state_store_get(st._id, None, None, 0, None, None, 0, 0, None, None, None, None, 0) == OK
    assert lib.pv_state_store_get_device(st._id, None, None, 0, None, None, 0, 0, None, None, None, None, 0,
                                         None) == OK

    rc, dev = device_get(st, roots, ridx, keys, True, sizing=True)
    assert rc == OK and (dev.val_off == full.val_off).all() and (dev.found == full.found).all()
    rc, dev = device_get(st, roots, ridx, keys, True, val_cap=total - 1)
    assert rc == EINVAL
    assert lib.pv_last_error().decode() == 'val_cap {} is below the {} bytes of the values'.format(total - 1, total)
    assert (dev.val_off == full.val_off).all()
    rc, _ = device_get(st, roots, ridx, keys, 2)
    assert rc == EINVAL and lib.pv_last_error() == b'decode must be 0 or 1'
    rc, dev = device_get(st, roots, [0] * 64 + [7], keys, True)                 # not checked on the host: malformed
    assert rc == OK and dev.status[64] == sg.MALFORMED and dev.found[64] == 0
    assert (dev.status[:64] == full.status[:64]).all()


def test_prove_outputs_are_what_they_were(mod, stores):
    """the walk behind k_trie_prove is the template the read shares: its outputs at the read's
    scenarios equal the mirror's, node ids and the max_nodes bound included"""
    import _state_store as ss
    batches, roots, ridx, keys = sg.sc_shapes()
    st = stores('shapes')
    host = ss.HostStore(1)
    for b in batches:
        host.add(b)
    for max_nodes in (None, 1):
        got = st.prove(roots, ridx, keys, max_nodes)
        want = ss.mirror_prove(host.db, host.id_of, roots, ridx, keys, max_nodes)
        assert want.same(got, ids=False) is None
    assert (st.prove(roots, ridx, keys, 1).status == ss.PATH_TOO_LONG).any()
