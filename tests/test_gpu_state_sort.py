"""State keys sorted on the GPU (pv_state_sort_device, the k_trie_sort_* kernels) against the
Python mirror, and the fused forms (pv_state_build_unsorted_device,
pv_state_apply_unsorted_device) against the sorted device forms over the sorted distinct pairs,
byte for byte.  The case lists are those of tests/test_state_sort_host.py (tests/_state_sort.py).
Every comparison is exact, and every call's input buffers are compared before and after."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import _state_apply as sa
import _state_build as sb
import _state_sort as so
import _state_update as su

pytestmark = pytest.mark.gpu

OK, EINVAL, ENOTINIT = 0, -22, -77
U8P = ctypes.POINTER(ctypes.c_uint8)
T = so.TILE


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    assert state_store.SORT_TILE == T
    return state_store


def lib():
    from plenum_gpu import _native as nat
    return nat.load()


def last_error():
    return lib().pv_last_error().decode()


class Inputs:
    """host arrays on the device, and whether they still hold the same bytes"""

    def __init__(self, *arrays):
        import torch
        self.host = [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]
        self.dev = [torch.from_numpy(h).to('cuda:0') for h in self.host]
        torch.cuda.synchronize()

    def ptr(self, i):
        return ctypes.c_void_p(self.dev[i].data_ptr())

    def unchanged(self):
        return all((d.cpu().numpy() == h).all() for d, h in zip(self.dev, self.host))


def device_sort(keys, lead=0, blob=None, off=None):
    """pv_state_sort_device -> (rc, perm (n words, 0xffffffff where not written), n_kept)"""
    import torch
    if blob is None:
        blob, off = so.pack(keys, lead=lead)
    n = len(off) - 1
    inp = Inputs(blob, off)
    perm = torch.full((max(n, 1),), -1, dtype=torch.int32, device='cuda:0')
    kept = ctypes.c_uint64(12345)
    torch.cuda.synchronize()
    rc = lib().pv_state_sort_device(inp.ptr(0), inp.ptr(1), n, ctypes.c_void_p(perm.data_ptr()), ctypes.byref(kept),
                                    0, None)
    torch.cuda.synchronize()
    assert inp.unchanged()
    return rc, perm.cpu().numpy().view(np.uint32), kept.value


def check_sort(keys, **kw):
    want = so.mirror(keys)
    rc, perm, kept = device_sort(keys, **kw)
    assert rc == OK, last_error()
    assert kept == len(want)
    assert (perm[:kept] == want).all()
    assert (perm[kept:] == 0xffffffff).all()


def device_call(entry, prs, n_nodes, n_bytes, store=-1, root=None, insert=True, blob_cap=None, node_cap=None,
                outputs=True):
    """pv_state_build[_unsorted]_device (root None) or pv_state_apply[_unsorted]_device over (key,
    encoded value) pairs as given, with output buffers of exactly n_bytes / n_nodes (or the
    capacities given) -> Built"""
    import torch
    dev = torch.device('cuda:0')
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                  # noqa: E731
    kb, ko = sb.pack([k for k, _ in prs])
    vb, vo = sb.pack([v for _, v in prs])
    inp = Inputs(kb, ko, vb, vo)
    bc = n_bytes if blob_cap is None else blob_cap
    nc = n_nodes if node_cap is None else node_cap
    blob = torch.full((max(bc, 1),), 0x5a, dtype=torch.uint8, device=dev)
    off = torch.zeros(nc + 1, dtype=torch.int64, device=dev)
    dig = torch.zeros(max(nc, 1) * 32, dtype=torch.uint8, device=dev)
    new = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    outs = (p(blob), bc, p(off), nc, p(dig)) if outputs else (None, 0, None, 0, None)
    torch.cuda.synchronize()
    if root is None:
        rc = getattr(lib(), entry)(inp.ptr(0), inp.ptr(1), inp.ptr(2), inp.ptr(3), len(prs), store,
                                   new.ctypes.data_as(U8P), ctypes.byref(nn), ctypes.byref(nb), *outs, 0, None)
    else:
        old = np.frombuffer(bytes(root), np.uint8).copy()
        rc = getattr(lib(), entry)(store, old.ctypes.data_as(U8P), inp.ptr(0), inp.ptr(1), inp.ptr(2), inp.ptr(3),
                                   len(prs), 1 if insert else 0, new.ctypes.data_as(U8P), ctypes.byref(nn),
                                   ctypes.byref(nb), *outs, None)
    torch.cuda.synchronize()
    assert inp.unchanged()
    b = sb.Built()
    b.rc, b.root, b.n_nodes, b.n_bytes = rc, new.tobytes(), nn.value, nb.value
    b.blob, b.off, b.dig = blob.cpu().numpy(), off.cpu().numpy().view(np.uint64), dig.cpu().numpy().reshape(-1, 32)
    b.untouched = bool((b.blob == 0x5a).all() and not b.off.any() and not b.dig.any())
    if rc == OK and outputs:
        b.blob, b.dig = b.blob[:b.n_bytes], b.dig[:b.n_nodes]
    return b


def with_stale(prs, seed, removals=False):
    """sorted distinct (key, encoded value) pairs -> the same pairs shuffled, with a stale earlier
    occurrence of every seventh key: another value, or (removals) a removal before a set, a set
    before a removal and, for every other such set, another set"""
    rng = random.Random(seed)
    order = list(prs)
    rng.shuffle(order)
    rank = {k: i for i, (k, _) in enumerate(prs)}
    out = []
    for k, v in order:
        if rank[k] % 7 == 0:
            stale = sb._encode(b'stale ' + k[:6])
            if stale == v:
                stale = sb._encode(b'another stale value')
            if removals and v and rank[k] % 14 == 0:
                stale = b''
            out.insert(rng.randrange(len(out) + 1), (k, stale))
        out.append((k, v))
    return out


def check_build(prs, seed, root=None):
    """the fused build over the shuffled pairs with stale occurrences == pv_state_build_device over prs"""
    sizes = device_call('pv_state_build_device', prs, 0, 0, outputs=False)
    assert sizes.rc == OK, last_error()
    want = device_call('pv_state_build_device', prs, sizes.n_nodes, sizes.n_bytes)
    got = device_call('pv_state_build_unsorted_device', with_stale(prs, seed), sizes.n_nodes, sizes.n_bytes)
    assert want.rc == OK and got.rc == OK, last_error()
    assert want.same(got) is None, want.same(got)
    if root is not None:
        assert got.root == root
    return want


# ------------------------------------------------------------------ 1. the sort alone
@pytest.mark.parametrize('n', so.SIZES)
def test_sort_sizes(mod, n):
    check_sort(so.shuffled(so.size_keys(n), 2000 + n))


@pytest.mark.parametrize('name', ['edges', 'shared200', 'long1024', 'multiplicity', 'tile_run', 'equal789',
                                  'mixed4096', 'chain', 'chain_dup', 'empty_keys'])
def test_sort_case(mod, name):
    check_sort(dict(so.accepted_cases())[name])


def test_sort_key_starts_on_every_residue(mod):
    keys = so.edge_keys()
    _, off = so.pack(keys)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8))
    for lead in (1, 4, 7):
        check_sort(keys, lead=lead)


def test_sort_equal_keys(mod):
    rc, perm, kept = device_sort([b'\x11' * 32] * 1000)
    assert (rc, kept, int(perm[0])) == (OK, 1, 999) and (perm[1:] == 0xffffffff).all()
    keys = so.tile_run_keys()
    assert len(set(keys[T - 20:T + 20])) == 1 and keys[T - 21] != keys[T - 20] != keys[T + 20]
    rc, perm, kept = device_sort(keys)
    assert rc == OK and kept == len(keys) - 39 and T + 19 in perm[:kept]
    assert not set(range(T - 20, T + 19)) & set(int(x) for x in perm[:kept])


def test_sort_python_entry(mod):
    keys = so.mixed_keys()[:500] + so.mixed_keys()[:50]
    assert (mod.sort_keys_gpu(keys) == mod.sort_keys_host(keys)).all()
    assert mod.sort_keys_gpu([]).shape == (0,)


def test_sort_refusals(mod):
    import torch
    keys = so.too_long_keys()
    rc, perm, kept = device_sort(keys)
    assert rc == EINVAL and (perm == 0xffffffff).all() and kept == 0
    assert last_error() == ('key 17 is above 1024 bytes: the device sort takes keys up to 1024 bytes, the host forms '
                            '(pv_state_build, pv_state_update, pv_state_apply) sort keys of any length')
    blob, off = so.pack([b'abc', b'de', b'f'])
    off[2] = 2
    rc, perm, kept = device_sort(None, blob=blob, off=off)
    assert rc == EINVAL and (perm == 0xffffffff).all() and kept == 0
    assert last_error() == 'key_off or val_off decreases at index 1'
    # before any launch
    d = torch.zeros(64, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    kept = ctypes.c_uint64(7)
    fn = lib().pv_state_sort_device
    p = d.data_ptr()
    assert fn(None, None, 0, None, None, 0, None) == OK
    assert fn(None, None, 0, None, ctypes.byref(kept), 0, None) == OK and kept.value == 0
    for args, code, text in (
            ((p, p, 1, p, ctypes.byref(kept), 63, None), ENOTINIT, 'device 63 not initialised (call pv_init)'),
            ((p, p, 1, p, None, 0, None), EINVAL, 'null pointer'),
            ((None, p, 1, p, ctypes.byref(kept), 0, None), EINVAL, 'null device buffer'),
            ((p, None, 1, p, ctypes.byref(kept), 0, None), EINVAL, 'null device buffer'),
            ((p, p, 1, None, ctypes.byref(kept), 0, None), EINVAL, 'null device buffer'),
            ((p, p, (1 << 28) + 1, p, ctypes.byref(kept), 0, None), EINVAL, 'more than 2^28 keys in one build'),
            ((p + 2, p, 1, p, ctypes.byref(kept), 0, None), EINVAL, 'key_blob must be 4-byte aligned')):
        assert fn(*args) == code and last_error() == text, (args, last_error())
    assert not d.cpu().numpy().any()


# ------------------------------------------------------------------ 2. the fused build
@pytest.mark.parametrize('name', [c.name for c in sb.fixture()])
def test_fused_build_fixture_case(mod, name):
    c = next(x for x in sb.fixture() if x.name == name)
    check_build(sb.pairs(c.items), 70, root=c.root)


def test_fused_build_proof_fixture_tries(mod):
    for k, (name, prs, root, db) in enumerate(sb.proof_fixture_tries()):
        want = check_build(prs, 71 + k, root=root)
        assert want.db() == db


@pytest.mark.parametrize('name', [n for n, _ in sb.boundary_pairs()])
def test_fused_build_list_header_boundaries(mod, name):
    check_build(dict(sb.boundary_pairs())[name], 72)


def test_fused_build_chain(mod):
    check_build(sb.chain_pairs(), 73)


def test_fused_build_4096_mixed(mod):
    prs = sb.mixed_pairs(4096, 13)
    want = check_build(prs, 74)
    assert want.root == mod.build_encoded_host(prs)[0]


def test_fused_build_capacity_insert_and_empty(mod):
    prs = sb.mixed_pairs(200, 24)
    unsorted = with_stale(prs, 75)
    sizes = device_call('pv_state_build_device', prs, 0, 0, outputs=False)
    want = device_call('pv_state_build_device', prs, sizes.n_nodes, sizes.n_bytes)
    entry = 'pv_state_build_unsorted_device'
    with mod.GpuStateStore(node_hint=1) as st:
        before = st.info()
        for kw in ({'blob_cap': want.n_bytes - 1}, {'node_cap': want.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            got = device_call(entry, unsorted, want.n_nodes, want.n_bytes, store=st._id, **kw)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'node capacity too small: the build has {} nodes of {} bytes'.format(
                want.n_nodes, want.n_bytes)
            assert (got.n_nodes, got.n_bytes) == (want.n_nodes, want.n_bytes) and st.info() == before
        got = device_call(entry, unsorted, 0, 0, outputs=False)                   # no store: nothing inserted
        assert (got.rc, got.root, got.n_nodes, got.n_bytes) == (OK, want.root, want.n_nodes, want.n_bytes)
        assert st.info() == before
        got = device_call(entry, unsorted, want.n_nodes, want.n_bytes, store=st._id)   # the retry
        assert want.same(got) is None and st.info()['n_nodes'] == want.n_nodes
    nn, nb, root = ctypes.c_uint64(7), ctypes.c_uint64(7), np.zeros(32, np.uint8)
    assert getattr(lib(), entry)(None, None, None, None, 0, 777, root.ctypes.data_as(U8P), ctypes.byref(nn),
                                 ctypes.byref(nb), None, 0, None, 0, None, 0, None) == OK
    assert root.tobytes() == mod.BLANK_ROOT and (nn.value, nb.value) == (0, 0)


def test_fused_build_refusals(mod):
    import torch
    prs = sb.mixed_pairs(50, 25)
    sizes = device_call('pv_state_build_device', prs, 0, 0, outputs=False)
    entry = 'pv_state_build_unsorted_device'
    with mod.GpuStateStore(node_hint=1) as st:
        before = st.info()
        long_key = [(b'k' * 1025, sb._encode(b'v'))]
        for bad, text in ((prs[:9] + long_key + prs[9:], 'key 9 is above 1024 bytes'),
                          (prs[:10] + [(prs[10][0], b'')] + prs[11:], 'value 10 is empty or above 2^30 bytes')):
            got = device_call(entry, bad, sizes.n_nodes + 2, sizes.n_bytes + 2000, store=st._id)
            assert got.rc == EINVAL and got.untouched and last_error().startswith(text), last_error()
            assert st.info() == before
        d = torch.zeros(64, dtype=torch.uint8, device='cuda:0')
        back = torch.from_numpy(np.array([0, 3, 2], np.int64)).to('cuda:0')
        torch.cuda.synchronize()
        root = np.zeros(32, np.uint8)
        p, rp = d.data_ptr(), root.ctypes.data_as(U8P)
        fn = getattr(lib(), entry)

        def call(kb=p, ko=p, vb=p, vo=p, n=1, store=-1, rt=rp, dig=None, device=0):
            return fn(kb, ko, vb, vo, n, store, rt, None, None, None, 0, None, 0, dig, device, None)

        for kw, code, text in (
                ({'device': 63}, ENOTINIT, 'device 63 not initialised (call pv_init)'),
                ({'rt': None}, EINVAL, 'null pointer'),
                ({'kb': None}, EINVAL, 'null device buffer'),
                ({'vo': None}, EINVAL, 'null device buffer'),
                ({'n': (1 << 28) + 1}, EINVAL, 'more than 2^28 keys in one build'),
                ({'kb': p + 1}, EINVAL, 'key_blob and val_blob must be 4-byte aligned'),
                ({'vb': p + 2}, EINVAL, 'key_blob and val_blob must be 4-byte aligned'),
                ({'dig': p + 4}, EINVAL, 'digest buffers must be 16-byte aligned'),
                ({'store': 777}, EINVAL, 'no state store with id 777'),
                ({'ko': back.data_ptr(), 'n': 2, 'store': st._id}, EINVAL, 'key_off or val_off decreases at index 1'),
                ({'vo': back.data_ptr(), 'n': 2, 'store': st._id}, EINVAL, 'key_off or val_off decreases at index 1')):
            assert call(**kw) == code and last_error() == text, (kw, last_error())
        assert st.info() == before and not d.cpu().numpy().any()


# ------------------------------------------------------------------ 3. the fused apply
def check_apply(mod, base, batches, roots, seed):
    """every batch of one shape: pv_state_apply_unsorted_device over the shuffled batch with stale
    occurrences == pv_state_apply_device over the sorted distinct batch, inserted batch after batch"""
    b0 = sb.host_build(base)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        root, nodes = b0.root, st.info()['n_nodes']
        for k, prs in enumerate(batches):
            sizes = device_call('pv_state_apply_device', prs, 0, 0, store=st._id, root=root, insert=False,
                                outputs=False)
            assert sizes.rc == OK, last_error()
            want = device_call('pv_state_apply_device', prs, sizes.n_nodes, sizes.n_bytes, store=st._id, root=root,
                               insert=False)
            unsorted = with_stale(prs, seed + k, removals=True)
            # compute only, then one node short (sizes, nothing written, nothing inserted), then the retry
            got = device_call('pv_state_apply_unsorted_device', unsorted, sizes.n_nodes, sizes.n_bytes, store=st._id,
                              root=root, insert=False)
            assert want.rc == OK and want.same(got) is None, (last_error(), want.same(got))
            assert st.info()['n_nodes'] == nodes
            if want.n_nodes:
                short = device_call('pv_state_apply_unsorted_device', unsorted, sizes.n_nodes, sizes.n_bytes,
                                    store=st._id, root=root, node_cap=want.n_nodes - 1)
                assert short.rc == EINVAL and short.untouched and st.info()['n_nodes'] == nodes
                assert last_error() == 'node capacity too small: the build has {} nodes of {} bytes'.format(
                    want.n_nodes, want.n_bytes)
                assert (short.n_nodes, short.n_bytes) == (want.n_nodes, want.n_bytes)
            got = device_call('pv_state_apply_unsorted_device', unsorted, sizes.n_nodes, sizes.n_bytes, store=st._id,
                              root=root)
            assert want.same(got) is None, want.same(got)
            nodes += want.n_nodes
            assert st.info()['n_nodes'] == nodes
            root = want.root
            if roots is not None:
                assert root == roots[k]


@pytest.mark.parametrize('name', [c.name for c in su.fixture()])
def test_fused_apply_update_fixture(mod, name):
    c = su.case(name)
    check_apply(mod, sb.pairs(c.base), [sb.pairs(b.items) for b in c.batches], [b.root for b in c.batches], 80)


@pytest.mark.parametrize('name', [c.name for c in sa.fixture()])
def test_fused_apply_remove_fixture(mod, name):
    c = sa.case(name)
    check_apply(mod, sb.pairs(c.base), [sa.ops(b.items) for b in c.batches], [b.root for b in c.batches], 81)


def test_fused_apply_without_removal_equals_update(mod):
    prs = sb.mixed_pairs(300, 31)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 64, 164)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        sizes = device_call('pv_state_update_device', batch, 0, 0, store=st._id, root=b0.root, insert=False,
                            outputs=False)
        want = device_call('pv_state_update_device', batch, sizes.n_nodes, sizes.n_bytes, store=st._id, root=b0.root,
                           insert=False)
        got = device_call('pv_state_apply_unsorted_device', with_stale(batch, 82), sizes.n_nodes, sizes.n_bytes,
                          store=st._id, root=b0.root, insert=False)
        assert want.rc == OK and want.same(got) is None


def test_fused_apply_refusals_and_empty(mod):
    prs = sb.mixed_pairs(50, 26)
    b0 = sb.host_build(prs)
    entry = 'pv_state_apply_unsorted_device'
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        batch = [(prs[3][0], b''), (b'k' * 1025, b''), (prs[4][0], sb._encode(b'x'))]
        got = device_call(entry, batch, 64, 4096, store=st._id, root=b0.root)
        assert got.rc == EINVAL and got.untouched and last_error().startswith('key 1 is above 1024 bytes')
        assert st.info() == before
        got = device_call(entry, prs[:3], 64, 4096, store=777, root=b0.root)
        assert got.rc == EINVAL and got.untouched and last_error() == 'no state store with id 777'
        # n == 0: the root stays, the store is not looked at
        old, new = np.frombuffer(b0.root, np.uint8).copy(), np.zeros(32, np.uint8)
        nn, nb = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert getattr(lib(), entry)(777, old.ctypes.data_as(U8P), None, None, None, None, 0, 1,
                                     new.ctypes.data_as(U8P), ctypes.byref(nn), ctypes.byref(nb), None, 0, None, 0,
                                     None, None) == OK
        assert new.tobytes() == b0.root and (nn.value, nb.value) == (0, 0) and st.info() == before


# ------------------------------------------------------------------ 4. the Python entries and the NYM path
def test_build_state_and_apply_batch_with_device_sort(mod):
    rng = random.Random(90)
    items = [(k, bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 80)))) for k, _ in sb.mixed_pairs(300, 27)]
    stale = [(k, b'stale') for k, _ in items[::7]]
    ops = [(k, None) for k, _ in items[:40]] + [(items[5][0], b'back again'), (b'new key', b'new'), (b'new key', None),
                                                (items[50][0], None), (items[50][0], b'set after the removal')]
    rng.shuffle(items)
    with mod.GpuStateStore(node_hint=1) as a, mod.GpuStateStore(node_hint=1) as b:
        ra, rb = a.build_state(stale + items), b.build_state(stale + items, device_sort=True)
        assert ra == rb == mod.build_host(stale + items)[0] and a.info() == b.info()
        ra, rb = a.apply_batch(ra, ops), b.apply_batch(rb, ops, device_sort=True)
        assert ra == rb and a.info() == b.info()
        assert b.apply_batch(rb, [], device_sort=True) == rb


def test_apply_batch_sha256_is_the_nym_path(mod, monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    dids = [b'did:sov:%022d' % (7919 * i) for i in range(1000)]
    items = [(d, b'{"verkey": "~%d", "seqNo": %d}' % (i, i)) for i, d in enumerate(dids)]
    random.Random(91).shuffle(items)
    items = [(dids[3], b'an earlier NYM of the same DID')] + items
    keyed = [(hashlib.sha256(d).digest(), v) for d, v in items]
    second = [(d, None if i % 5 == 0 else b'rotated %d' % i) for i, d in enumerate(dids[:200])]
    second += [(b'did:sov:new%d' % i, b'fresh %d' % i) for i in range(50)]
    random.Random(92).shuffle(second)
    keyed2 = [(hashlib.sha256(d).digest(), v) for d, v in second]
    with mod.GpuStateStore(node_hint=1) as st:
        r1 = st.apply_batch_sha256(mod.BLANK_ROOT, items)
        want1, db = mod.build_host(keyed)
        assert r1 == want1 and st.info()['n_unique'] == len(db)
        r2 = st.apply_batch_sha256(r1, second)
        want2, added = mod.apply_host(db, r1, keyed2)
        assert r2 == want2
        state = dict(keyed)
        for k, v in keyed2:
            if v is None:
                state.pop(k, None)
            else:
                state[k] = v
        gone = [k for k, v in keyed2 if v is None]
        keys = sorted(state)[:300] + gone[:20]
        res = st.generate_state_proofs_batch([(r2, k) for k in keys])
        assert [r[1] for r in res] == [state.get(k) for k in keys]
        ok = state_proofs.verify_state_proofs_batch([(r2, k, state.get(k), r[0]) for k, r in zip(keys, res)])
        assert ok.all()
        assert st.apply_batch_sha256(r2, []) == r2
