"""Sets onto a committed root on the GPU (pv_state_update / pv_state_update_device,
k_trie_update_count / k_trie_update_emit and the k_trie_build_* kernels over the merged list)
against the host build of the same headers (tools/hostcheck/stateupdatecheck.cpp), the Python
mirror, the fixture recorded from the reference and the verified rebuild.  The cases are those of
tests/test_state_update_host.py (tests/_state_update.py)."""
import ctypes
import random

import numpy as np
import pytest

import _state_build as sb
import _state_update as su

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -22
U8P = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


def device_update(store, root, prs, n_nodes, n_bytes, insert=True, blob_cap=None, node_cap=None, outputs=True):
    """pv_state_update_device over (key, encoded value) pairs as given, with output buffers of
    exactly n_bytes / n_nodes (or the capacities given) -> Built"""
    import torch
    from plenum_gpu import _native as nat
    lib = nat.load()
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                  # noqa: E731
    kb, ko = sb.pack([k for k, _ in prs])
    vb, vo = sb.pack([v for _, v in prs])
    d_kb, d_ko, d_vb, d_vo = t(kb), t(ko.view(np.int64)), t(vb), t(vo.view(np.int64))
    bc = n_bytes if blob_cap is None else blob_cap
    nc = n_nodes if node_cap is None else node_cap
    blob = torch.full((max(bc, 1),), 0x5a, dtype=torch.uint8, device=dev)
    off = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    dig = torch.zeros(max(nc, 1) * 32, dtype=torch.uint8, device=dev)
    old = np.frombuffer(bytes(root), np.uint8).copy()
    new = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    outs = (p(blob), bc, p(off), nc, p(dig)) if outputs else (None, 0, None, 0, None)
    rc = lib.pv_state_update_device(store, old.ctypes.data_as(U8P), p(d_kb), p(d_ko), p(d_vb), p(d_vo), len(prs),
                                    1 if insert else 0, new.ctypes.data_as(U8P), ctypes.byref(nn), ctypes.byref(nb),
                                    *outs, None)
    torch.cuda.synchronize()
    b = sb.Built()
    b.rc, b.root, b.n_nodes, b.n_bytes = rc, new.tobytes(), nn.value, nb.value
    b.blob, b.off, b.dig = blob.cpu().numpy(), off.cpu().numpy().view(np.uint64), dig.cpu().numpy().reshape(-1, 32)
    b.untouched = bool((b.blob == 0x5a).all() and not b.off.any() and not b.dig.any())
    if rc == OK and outputs:
        b.blob, b.dig = b.blob[:b.n_bytes], b.dig[:b.n_nodes]
    return b


def last_error():
    from plenum_gpu import _native as nat
    return nat.load().pv_last_error().decode()


def check_shape(mod, name):
    """every batch of one shape: device == host twin byte for byte (blob, offsets, digests, root,
    counts), inserted batch after batch into one store -> (store info at the end, host outputs)"""
    _, base, batches = next(s for s in su.all_shapes() if s[0] == name)
    b0, outs, _ = su.host_run(name, base, batches)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        root, nodes = b0.root, st.info()['n_nodes']
        for prs, want in zip(batches, outs):
            got = device_update(st._id, root, prs, want.n_nodes, want.n_bytes)
            assert got.rc == OK, last_error()
            assert want.same(got) is None, want.same(got)
            nodes += want.n_nodes
            assert st.info()['n_nodes'] == nodes
            root = want.root
        # the host form over the last batch, computing only: any order, the same nodes
        if batches:
            shuffled = list(batches[-1])
            random.Random(1).shuffle(shuffled)
            prev = outs[-2].root if len(outs) > 1 else b0.root
            r, nn, nb, blob, off, dig = mod._update_gpu(st._id, prev, shuffled, insert=False, want_nodes=True)
            want = outs[-1]
            assert (r, nn, nb) == (want.root, want.n_nodes, want.n_bytes)
            assert (blob == want.blob).all() and (off == want.off).all() and (dig == want.dig).all()
            assert st.info()['n_nodes'] == nodes
    return outs


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize('name', [c.name for c in su.fixture()])
def test_fixture_case_equals_host_twin_and_reference(mod, name):
    c = su.case(name)
    outs = check_shape(mod, 'fx/' + name)
    held = set(c.base_reachable)
    for want, got in zip(c.batches, outs):
        assert got.root == want.root
        emitted = set(got.dig[i].tobytes() for i in range(got.n_nodes))
        assert emitted <= want.reachable
        held |= emitted
        assert want.reachable <= held


def test_fixture_states_are_served_from_the_store(mod):
    """through update_state: after every batch each key of the state has its value at the new root"""
    for name in ('dogs', 'inline_branch', 'short_root', 'empty_key_into_a_state_with_it', 'mixed300'):
        c = su.case(name)
        with mod.GpuStateStore(node_hint=1) as st:
            root = st.update_state(mod.BLANK_ROOT, c.base)
            assert root == c.base_root
            state = dict(c.base)
            for b in c.batches:
                root = st.update_state(root, b.items)
                assert root == b.root
                state.update(b.items)
                keys = list(state)
                assert st.get_for_root_hash_batch([(root, k) for k in keys]) == [state[k] for k in keys]


def test_resetting_existing_values_keeps_root_and_unique_count(mod):
    c = su.case('reset_same_values')
    with mod.GpuStateStore(node_hint=1) as st:
        root = st.build_state(c.base)
        before = st.info()
        assert st.update_state(root, c.batches[0].items) == root == c.base_root
        after = st.info()
        assert after['n_unique'] == before['n_unique'] and after['n_nodes'] > before['n_nodes']


# ------------------------------------------------------------------ 2. device against the host twin
@pytest.mark.parametrize('name', [s[0] for s in su.shapes()])
def test_shape_equals_host_twin(mod, name):
    check_shape(mod, name)


# ------------------------------------------------------------------ 3. against the verified rebuild
def test_eight_batches_onto_20000_keys(mod, monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    rng = random.Random(20000)
    state = {rng.getrandbits(256).to_bytes(32, 'big'): b'value %d' % i for i in range(20000)}
    snapshots, batch_keys = [], []
    with mod.GpuStateStore(node_hint=1 << 16) as st:
        root = st.build_state(list(state.items()))
        for b in range(8):
            batch = [(k, b'batch %d over %d' % (b, i)) for i, k in enumerate(rng.sample(sorted(state), 32))]
            batch += [(rng.getrandbits(256).to_bytes(32, 'big'), b'batch %d new %d' % (b, i)) for i in range(32)]
            root = st.update_state(root, batch)
            state.update(batch)
            assert root == mod.build_host(list(state.items()))[0]
            snapshots.append((root, dict(state)))
            batch_keys += [k for k, _ in batch]
        # at every intermediate root: each batch key's value as of that root, absent where a later batch added it
        queries = [(r, k) for r, _ in snapshots for k in batch_keys]
        expect = [snap.get(k) for _, snap in snapshots for k in batch_keys]
        res = st.generate_state_proofs_batch(queries)
    # a key that batch b added is absent at the b roots before it, wherever it occurs among the batch keys
    added_at = {k: min(b for b, (_, snap) in enumerate(snapshots) if k in snap) for k in set(batch_keys)}
    assert len(queries) == 8 * 8 * 64 and sum(added_at.values()) == 32 * 28
    assert sum(e is None for e in expect) == sum(added_at[k] for k in batch_keys)
    assert all(x is not None for x in res) and [x[1] for x in res] == expect
    ok = state_proofs.verify_state_proofs_batch([(r, k, e, x[0]) for (r, k), e, x in zip(queries, expect, res)])
    assert ok.all()


# ------------------------------------------------------------------ 4. refusals and edges
def test_empty_batch_blank_root_and_compute_only(mod):
    prs = sb.mixed_pairs(200, 51)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 40, 51)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        got = device_update(st._id, b0.root, [], 0, 0)
        assert (got.rc, got.root, got.n_nodes, got.n_bytes, int(got.off[0])) == (OK, b0.root, 0, 0, 0)
        assert mod._update_gpu(st._id, b0.root, []) == (b0.root, 0, 0) and st.info() == before
        got = device_update(st._id, mod.BLANK_ROOT, prs, b0.n_nodes, b0.n_bytes, insert=False)
        assert b0.same(got) is None and st.info() == before            # the result of pv_state_build
        with su.HostStore() as hs:
            hs.add_nodes(b0.nodes())
            want = hs.update(b0.root, batch, insert=False)
        got = device_update(st._id, b0.root, batch, want.n_nodes, want.n_bytes, insert=False)
        assert want.same(got) is None and st.info() == before          # insert == 0 only computes
        sizes = device_update(st._id, b0.root, batch, 0, 0, insert=False, outputs=False)
        assert (sizes.rc, sizes.root, sizes.n_nodes, sizes.n_bytes) == (OK, want.root, want.n_nodes, want.n_bytes)


def test_too_small_capacity_then_retry(mod):
    prs = sb.mixed_pairs(200, 52)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 40, 52)
    with su.HostStore() as hs:
        hs.add_nodes(b0.nodes())
        want = hs.update(b0.root, batch, insert=False)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        for kw in ({'blob_cap': want.n_bytes - 1}, {'node_cap': want.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            got = device_update(st._id, b0.root, batch, want.n_nodes, want.n_bytes, **kw)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'node capacity too small: the build has {} nodes of {} bytes'.format(
                want.n_nodes, want.n_bytes)
            assert (got.n_nodes, got.n_bytes) == (want.n_nodes, want.n_bytes)
            assert st.info() == before
        got = device_update(st._id, b0.root, batch, got.n_nodes, got.n_bytes)       # the retry, with the sizes reported
        assert want.same(got) is None
        assert st.info()['n_nodes'] == before['n_nodes'] + want.n_nodes


def test_unsorted_duplicate_and_empty_value_device_input(mod):
    prs = sb.mixed_pairs(200, 53)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 40, 53)
    swapped = list(batch)
    swapped[20], swapped[21] = swapped[21], swapped[20]
    dup = batch[:30] + [batch[29]] + batch[30:]
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        for bad, idx in ((swapped, 21), (dup, 30), ([(b'ab', b'\x01'), (b'a', b'\x01')], 1)):
            got = device_update(st._id, b0.root, bad, 100, 10000)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'keys not strictly increasing at index {0} (key {0} is not above key {1})'.format(
                idx, idx - 1)
            assert st.info() == before
        got = device_update(st._id, b0.root, batch[:10] + [(batch[10][0], b'')] + batch[11:], 100, 10000)
        assert got.rc == EINVAL and got.untouched and last_error() == 'value 10 is empty or above 2^30 bytes'
        assert st.info() == before


def test_missing_root_and_withheld_node(mod):
    prs = sb.mixed_pairs(200, 54)
    b0 = sb.host_build(prs)
    db = b0.db()
    batch = su._batch_onto(prs, 40, 54)
    nodes = mod.walk_host(db, b0.root, batch[7][0])[1]
    held = nodes[1]
    first = next(j for j, (k, _) in enumerate(batch) if held in mod.walk_host(db, b0.root, k)[1])
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes([n for n in b0.nodes() if n != held])
        before = st.info()
        got = device_update(st._id, sb.sha3(b'no such root'), batch, 100, 10000)
        assert got.rc == EINVAL and got.untouched and st.info() == before
        assert last_error() == ('state update: key 0: the root or a node on its path is not in the store '
                                '(status 2)')
        got = device_update(st._id, b0.root, batch, 100, 10000)
        assert got.rc == EINVAL and got.untouched and st.info() == before
        assert last_error() == ('state update: key {}: the root or a node on its path is not in the store '
                                '(status 2)'.format(first))
        with pytest.raises(KeyError, match='key {}:'.format(first)):
            st.update_state(b0.root, [(k, b'raw') for k, _ in batch])
        assert st.info() == before


def test_refusals_before_any_launch(mod):
    from plenum_gpu import _native as nat
    import torch
    lib = nat.load()
    dev = torch.device('cuda:0')

    def err(rc, code, text):
        assert rc == code and last_error() == text, (rc, last_error())

    u64 = lambda *v: np.asarray(v, np.uint64)                                   # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rptr = lambda a: None if a is None else a.ctypes.data_as(U8P)              # noqa: E731
    old, new = np.frombuffer(mod.BLANK_ROOT, np.uint8).copy(), np.zeros(32, np.uint8)
    keys = np.frombuffer(b'abcd' + b'\0' * 16, np.uint8).copy()
    vals = np.frombuffer(b'\x01\x02' + b'\0' * 16, np.uint8).copy()
    koff, voff = u64(0, 2, 4), u64(0, 1, 2)
    with mod.GpuStateStore(node_hint=1) as st:
        sid = st._id

        def upd(store=sid, rt=old, kb=keys, ko=koff, vb=vals, vo=voff, n=2, out=new):
            return lib.pv_state_update(store, rptr(rt), ptr(kb), ptr(ko), ptr(vb), ptr(vo), n, 0, rptr(out), None, None,
                                       None, 0, None, 0, None)

        assert upd() == OK and new.tobytes() == mod.build_encoded_host([(b'ab', b'\x01'), (b'cd', b'\x02')])[0]
        for bad in (0, -1, 12345):
            err(upd(store=bad), EINVAL, 'no state store with id {}'.format(bad))
            assert upd(store=bad, n=0) == OK                                    # the empty batch looks at nothing
        err(upd(rt=None), EINVAL, 'null pointer')
        err(upd(out=None), EINVAL, 'null pointer')
        err(upd(ko=None), EINVAL, 'null buffer')
        err(upd(vb=None), EINVAL, 'null buffer')
        err(upd(kb=None), EINVAL, 'null buffer')
        err(upd(ko=u64(0, 3, 2)), EINVAL, 'key_off not monotone at 1')
        err(upd(vo=u64(0, 1, 1)), EINVAL, 'value 1 is empty')
        t = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
        d_k, d_v = t(keys), t(vals)
        d_ko, d_vo = t(koff.view(np.int64)), t(voff.view(np.int64))

        def dupd(store=sid, kb=d_k.data_ptr(), ko=d_ko.data_ptr(), vb=d_v.data_ptr(), vo=d_vo.data_ptr(), n=2, rt=old):
            return lib.pv_state_update_device(store, rptr(rt), kb, ko, vb, vo, n, 0, rptr(new), None, None, None, 0, None,
                                              0, None, None)

        assert dupd() == OK
        err(dupd(store=777), EINVAL, 'no state store with id 777')
        err(dupd(rt=None), EINVAL, 'null pointer')
        err(dupd(kb=None), EINVAL, 'null device buffer')
        err(dupd(vo=None), EINVAL, 'null device buffer')
        err(dupd(kb=d_k.data_ptr() + 1), EINVAL, 'key_blob and val_blob must be 4-byte aligned')
        err(dupd(vb=d_v.data_ptr() + 2), EINVAL, 'key_blob and val_blob must be 4-byte aligned')
        d_back = t(u64(0, 3, 2).view(np.int64))
        err(dupd(ko=d_back.data_ptr()), EINVAL,
            'key_off or val_off decreases, or a key is above 2^20 bytes, at index 1')
        assert st.info()['n_nodes'] == 0
