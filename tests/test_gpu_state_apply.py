"""Sets and removals onto a committed root on the GPU (pv_state_apply / pv_state_apply_device,
k_trie_apply_count / k_trie_apply_emit and the k_trie_build_* kernels over the merged list)
against the host build of the same headers (tools/hostcheck/stateapplycheck.cpp), the fixture
recorded from the reference and the proofs served at the new root.  The cases are those of
tests/test_state_apply_host.py (tests/_state_apply.py)."""
import ctypes
import random

import numpy as np
import pytest

import _state_apply as sa
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


def device_apply(store, root, prs, n_nodes, n_bytes, insert=True, blob_cap=None, node_cap=None, outputs=True,
                 entry='pv_state_apply_device'):
    """pv_state_apply_device over (key, encoded value or b'') pairs as given, with output buffers
    of exactly n_bytes / n_nodes (or the capacities given) -> Built"""
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
    rc = getattr(lib, entry)(store, old.ctypes.data_as(U8P), p(d_kb), p(d_ko), p(d_vb), p(d_vo), len(prs),
                             1 if insert else 0, new.ctypes.data_as(U8P), ctypes.byref(nn), ctypes.byref(nb), *outs, None)
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
    counts), inserted batch after batch into one store -> the host outputs"""
    _, base, batches = next(s for s in sa.all_shapes() if s[0] == name)
    b0, outs, _ = sa.host_run(name, base, batches)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        root, nodes = b0.root, st.info()['n_nodes']
        for prs, want in zip(batches, outs):
            got = device_apply(st._id, root, prs, want.n_nodes, want.n_bytes)
            assert got.rc == OK, last_error()
            assert want.same(got) is None, want.same(got)
            nodes += want.n_nodes
            assert st.info()['n_nodes'] == nodes
            root = want.root
        # the host form over the last batch, computing only: any order, the same nodes
        shuffled = list(batches[-1])
        random.Random(1).shuffle(shuffled)
        prev = outs[-2].root if len(outs) > 1 else b0.root
        r, nn, nb, blob, off, dig = mod._apply_gpu(st._id, prev, shuffled, insert=False, want_nodes=True)
        want = outs[-1]
        assert (r, nn, nb) == (want.root, want.n_nodes, want.n_bytes)
        assert (blob == want.blob).all() and (off == want.off).all() and (dig == want.dig).all()
        assert st.info()['n_nodes'] == nodes
    return outs


# ------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize('name', [c.name for c in sa.fixture()])
def test_fixture_case_equals_host_twin_and_reference(mod, name):
    c = sa.case(name)
    outs = check_shape(mod, 'fx/' + name)
    held = set(c.base_reachable)
    for want, got in zip(c.batches, outs):
        assert got.root == want.root
        emitted = set(got.dig[i].tobytes() for i in range(got.n_nodes))
        assert emitted <= want.reachable
        held |= emitted
        assert want.reachable <= held


# ------------------------------------------------------------------ 2. device against the host twin
@pytest.mark.parametrize('name', [s[0] for s in sa.shapes()])
def test_shape_equals_host_twin(mod, name):
    check_shape(mod, name)


def test_batch_without_removal_equals_update(mod):
    prs = sb.mixed_pairs(300, 31)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 64, 164)
    with su.HostStore() as hs:
        hs.add_nodes(b0.nodes())
        want = hs.update(b0.root, batch, insert=False)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        a = device_apply(st._id, b0.root, batch, want.n_nodes, want.n_bytes, insert=False)
        u = device_apply(st._id, b0.root, batch, want.n_nodes, want.n_bytes, insert=False, entry='pv_state_update_device')
        assert want.same(a) is None and want.same(u) is None


# ------------------------------------------------------------------ 3. through the store's interface
def test_removed_keys_are_proven_absent_at_the_new_root_and_present_at_the_old(mod, monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    rng = random.Random(7)
    state = {rng.getrandbits(256).to_bytes(32, 'big'): b'value %d' % i for i in range(2000)}
    state.update({b'attr:%d' % i: b'x' * (i % 90 + 1) for i in range(200)})
    verifier = state_proofs.GpuStateVerifier()
    with mod.GpuStateStore(node_hint=1 << 12) as st:
        old = st.build_state(list(state.items()))
        gone = rng.sample(sorted(state), 100)
        absent = [rng.getrandbits(256).to_bytes(32, 'big') for _ in range(20)]
        sets = [(rng.getrandbits(256).to_bytes(32, 'big'), b'new %d' % i) for i in range(30)]
        new = st.apply_batch(old, [(k, None) for k in gone + absent] + sets)
        after = dict(state)
        after.update(sets)
        for k in gone:
            del after[k]
        assert new == mod.build_host(list(after.items()))[0]
        assert st.remove_keys(new, absent) == new
        res = st.generate_state_proofs_batch([(new, k) for k in gone] + [(old, k) for k in gone])
        assert all(r is not None for r in res)
        assert [r[1] for r in res] == [None] * len(gone) + [state[k] for k in gone]
        for k, r in list(zip(gone, res))[:8]:
            assert verifier.verify_state_proof(new, k, None, r[0], True)
        for k, r in list(zip(gone, res[len(gone):]))[:8]:
            assert verifier.verify_state_proof(old, k, state[k], r[0], True)
        ok = state_proofs.verify_state_proofs_batch(
            [(new, k, None, r[0]) for k, r in zip(gone, res)] +
            [(old, k, state[k], r[0]) for k, r in zip(gone, res[len(gone):])])
        assert ok.all()
        keys = list(after)
        assert st.get_for_root_hash_batch([(new, k) for k in keys]) == [after[k] for k in keys]
        # everything removed: the blank root, which serves the empty proof
        assert st.remove_keys(new, keys) == mod.BLANK_ROOT


def test_fixture_states_are_served_from_the_store(mod):
    for name in ('collapse_under_extension_inline_branch', 'full_branch_loses_14_then_15', 'branch_value_removed',
                 'remove_key_set_key_with_suffix', 'mixed300'):
        c = sa.case(name)
        with mod.GpuStateStore(node_hint=1) as st:
            root = st.build_state(c.base)
            assert root == c.base_root
            state = dict(c.base)
            for b in c.batches:
                root = st.apply_batch(root, b.items)
                assert root == b.root
                for k, v in b.items:
                    state[k] = v
                keys = list(state)
                assert st.get_for_root_hash_batch([(root, k) for k in keys]) == [state[k] for k in keys]


def test_sizing_call_then_insert_inserts_each_node_once(mod):
    prs = sb.mixed_pairs(200, 52)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 40, 52)
    with sa.HostStore() as hs:
        hs.add_nodes(b0.nodes())
        want = hs.apply(b0.root, batch, insert=False)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        sizes = device_apply(st._id, b0.root, batch, 0, 0, insert=False, outputs=False)
        assert (sizes.rc, sizes.root, sizes.n_nodes, sizes.n_bytes) == (OK, want.root, want.n_nodes, want.n_bytes)
        assert st.info() == before
        got = device_apply(st._id, b0.root, batch, want.n_nodes, want.n_bytes, insert=False)
        assert want.same(got) is None and st.info() == before            # insert == 0 only computes
        got = device_apply(st._id, b0.root, batch, want.n_nodes, want.n_bytes, insert=True)
        assert want.same(got) is None
        after = st.info()
        assert after['n_nodes'] == before['n_nodes'] + want.n_nodes
        new = len(set(want.db()) - set(b0.db()))
        assert after['n_unique'] == before['n_unique'] + new and 0 < new < want.n_nodes
        # the host form: the sizing call computes only, the retry inserts
        r = mod._apply_gpu(st._id, b0.root, batch, insert=True, want_nodes=True)
        assert r[0] == want.root and st.info()['n_nodes'] == after['n_nodes'] + want.n_nodes
        assert st.info()['n_unique'] == after['n_unique']


# ------------------------------------------------------------------ 4. refusals and edges
def test_empty_batch_blank_root_and_nothing_left(mod):
    prs = sb.mixed_pairs(100, 41)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 20, 41)
    kept = sb.host_build([p for p in batch if p[1]])
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        got = device_apply(st._id, b0.root, [], 0, 0)
        assert (got.rc, got.root, got.n_nodes, got.n_bytes, int(got.off[0])) == (OK, b0.root, 0, 0, 0)
        got = device_apply(st._id, mod.BLANK_ROOT, batch, kept.n_nodes, kept.n_bytes, insert=False)
        assert kept.same(got) is None                                    # removals of nothing are dropped
        got = device_apply(st._id, mod.BLANK_ROOT, [(k, b'') for k, _ in batch], 0, 0)
        assert (got.rc, got.root, got.n_nodes, got.n_bytes, int(got.off[0])) == (OK, mod.BLANK_ROOT, 0, 0, 0)
        got = device_apply(st._id, b0.root, [(k, b'') for k, _ in prs], 0, 0)
        assert (got.rc, got.root, got.n_nodes, got.n_bytes, int(got.off[0])) == (OK, mod.BLANK_ROOT, 0, 0, 0)
        assert mod._apply_gpu(st._id, b0.root, [(k, b'') for k, _ in prs]) == (mod.BLANK_ROOT, 0, 0)
        assert st.info() == before


def test_too_small_capacity_then_retry(mod):
    prs = sb.mixed_pairs(200, 52)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 40, 53)
    with sa.HostStore() as hs:
        hs.add_nodes(b0.nodes())
        want = hs.apply(b0.root, batch, insert=False)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        for kw in ({'blob_cap': want.n_bytes - 1}, {'node_cap': want.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            got = device_apply(st._id, b0.root, batch, want.n_nodes, want.n_bytes, **kw)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'node capacity too small: the build has {} nodes of {} bytes'.format(
                want.n_nodes, want.n_bytes)
            assert (got.n_nodes, got.n_bytes) == (want.n_nodes, want.n_bytes)
            assert st.info() == before
        got = device_apply(st._id, b0.root, batch, got.n_nodes, got.n_bytes)
        assert want.same(got) is None
        assert st.info()['n_nodes'] == before['n_nodes'] + want.n_nodes


def test_unsorted_and_duplicate_device_input(mod):
    prs = sb.mixed_pairs(200, 53)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 40, 54)
    swapped = list(batch)
    swapped[20], swapped[21] = swapped[21], swapped[20]
    dup = batch[:30] + [batch[29]] + batch[30:]
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        for bad, idx in ((swapped, 21), (dup, 30), ([(b'ab', b''), (b'a', b'\x01')], 1)):
            got = device_apply(st._id, b0.root, bad, 100, 10000)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'keys not strictly increasing at index {0} (key {0} is not above key {1})'.format(
                idx, idx - 1)
            assert st.info() == before


def test_missing_sibling_and_malformed_opened_node(mod):
    from plenum_gpu.state_proofs import rlp_encode
    prs, b0, key, proof = sa.sibling_case()
    two = sorted([(key, b''), (b'\x00 a new key below every other', sb._encode(b'v'))])
    at = two.index((key, b''))
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(proof)                              # the removed key's proof nodes only
        before = st.info()
        got = device_apply(st._id, b0.root, two, 100, 10000)
        assert got.rc == EINVAL and got.untouched and st.info() == before
        assert (got.n_nodes, got.n_bytes) == (0, 0)
        assert last_error() == ('state apply: key {}: the root or a node on its path is not in the store '
                                '(status 2)'.format(at))
        with pytest.raises(KeyError, match='key 0:'):
            st.remove_keys(b0.root, [key])
        assert st.update_state(b0.root, [(key, b'set instead')]) != b0.root   # a set needs no sibling
    junk = b'\xc3\x01\x02\x03' + b'\x00' * 40
    leaf = rlp_encode([b'\x20', sb._encode(b'x' * 40)])
    root_node = rlp_encode([b'', sb.sha3(junk), sb.sha3(leaf)] + [b''] * 14)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes([junk, leaf, root_node])
        before = st.info()
        got = device_apply(st._id, sb.sha3(root_node), [(b'\x20', b'')], 100, 10000)
        assert got.rc == EINVAL and got.untouched and st.info() == before
        assert last_error() == 'state apply: key 0: a node on its path is not a well-formed trie node (status 3)'
        with pytest.raises(ValueError, match='key 0:'):
            st.apply_batch(sb.sha3(root_node), [(b'\x20', None)])


def test_update_and_build_still_refuse_an_empty_value(mod):
    prs = sb.mixed_pairs(50, 55)
    b0 = sb.host_build(prs)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        with pytest.raises(ValueError):
            st.update_state(b0.root, [(prs[0][0], b'')])
        with pytest.raises(ValueError):
            st.build_state([(b'k', b'')])
        with pytest.raises(ValueError):
            st.apply_batch(b0.root, [(prs[0][0], b'')])
        got = device_apply(st._id, b0.root, [(prs[0][0], b'')], 100, 10000, entry='pv_state_update_device')
        assert got.rc == EINVAL and got.untouched and last_error() == 'value 0 is empty or above 2^30 bytes'
        from plenum_gpu import _native as nat
        kb, ko = sb.pack([prs[0][0]])
        vb, vo = sb.pack([b''])
        old, new = np.frombuffer(b0.root, np.uint8).copy(), np.zeros(32, np.uint8)
        rc = nat.load().pv_state_update(st._id, old.ctypes.data_as(U8P), kb.ctypes.data, ko.ctypes.data, vb.ctypes.data,
                                        vo.ctypes.data, 1, 0, new.ctypes.data_as(U8P), None, None, None, 0, None, 0, None)
        assert rc == EINVAL and last_error() == 'value 0 is empty'
        assert st.info() == before
