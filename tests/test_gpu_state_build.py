"""The batch trie build on the GPU (pv_state_build / pv_state_build_device, k_trie_build_*)
against the host build of the same header (tools/hostcheck/statebuildcheck.cpp), the Python
mirror and the fixture recorded from the reference.  The cases are those of
tests/test_state_build_host.py (tests/_state_build.py)."""
import ctypes
import random

import numpy as np
import pytest

import _state_build as sb

pytestmark = pytest.mark.gpu

OK, EINVAL, ENOTINIT = 0, -22, -77
U8P = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


def device_build(prs, n_nodes, n_bytes, store=-1, blob_cap=None, node_cap=None, outputs=True):
    """pv_state_build_device over (key, encoded value) pairs as given, with output buffers of
    exactly n_bytes / n_nodes (or the capacities given) -> (rc, Built)"""
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
    root = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    outs = (p(blob), bc, p(off), nc, p(dig)) if outputs else (None, 0, None, 0, None)
    rc = lib.pv_state_build_device(p(d_kb), p(d_ko), p(d_vb), p(d_vo), len(prs), store, root.ctypes.data_as(U8P),
                                   ctypes.byref(nn), ctypes.byref(nb), *outs, 0, None)
    torch.cuda.synchronize()
    b = sb.Built()
    b.rc, b.root, b.n_nodes, b.n_bytes = rc, root.tobytes(), nn.value, nb.value
    b.blob, b.off, b.dig = blob.cpu().numpy(), off.cpu().numpy().view(np.uint64), dig.cpu().numpy().reshape(-1, 32)
    b.untouched = bool((b.blob == 0x5a).all() and not b.off.any() and not b.dig.any())
    if rc == OK and outputs:
        b.blob, b.dig = b.blob[:b.n_bytes], b.dig[:b.n_nodes]
    return b


def check_equal(prs, name=None):
    """device == host build: root, counts, offsets, blob and digests, byte for byte"""
    want = sb.host_build_cached(name, prs) if name else sb.host_build(prs)
    assert want.rc == sb.OK
    got = device_build(prs, want.n_nodes, want.n_bytes)
    assert want.same(got) is None, want.same(got)
    return want


def last_error():
    from plenum_gpu import _native as nat
    return nat.load().pv_last_error().decode()


# ------------------------------------------------------------------ 1. fixture and boundaries
@pytest.mark.parametrize('name', [c.name for c in sb.fixture()])
def test_fixture_case_equals_host_build(mod, name):
    c = next(x for x in sb.fixture() if x.name == name)
    want = check_equal(sb.pairs(c.items), 'fx/' + name)
    assert want.root == c.root
    # the host form: any order, the last of equal keys wins
    root, n_nodes, n_bytes, blob, off, dig = mod._build_gpu(
        [(k, mod.rlp_encode([v])) for k, v in c.items], -1, want_nodes=True)
    assert (root, n_nodes, n_bytes) == (c.root, want.n_nodes, want.n_bytes)
    assert (blob == want.blob).all() and (off == want.off).all() and (dig == want.dig).all()
    assert sorted(set(dig[i].tobytes() for i in range(n_nodes))) == c.digests


def test_proof_fixture_tries(mod):
    for name, prs, root, db in sb.proof_fixture_tries():
        want = check_equal(prs, 'pf/' + name)
        assert want.root == root and want.db() == db


@pytest.mark.parametrize('name', [n for n, _ in sb.boundary_pairs()])
def test_list_header_boundaries(mod, name):
    check_equal(dict(sb.boundary_pairs())[name], 'bd/' + name)


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize('n', [63, 64, 65])
def test_wave_edge(mod, n):
    check_equal(sb.random_pairs(n, 40 + n))


def test_chain(mod):
    want = check_equal(sb.chain_pairs(), 'chain')
    assert want.max_level == 63


def test_4096_mixed_against_the_mirror(mod):
    prs = sb.mixed_pairs(4096, 13)
    want = check_equal(prs)
    root, db = mod.build_encoded_host(prs)
    assert want.root == root and want.db() == db


def test_65536_random_keys(mod):
    rng = random.Random(65536)
    keys = sorted({rng.getrandbits(256).to_bytes(32, 'big') for _ in range(65536)})
    assert len(keys) == 65536
    val = mod.rlp_encode([b'v' * 40])
    check_equal([(k, val) for k in keys])


# ------------------------------------------------------------------ 3. into a store
def test_build_state_serves_proofs(mod, monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    rng = random.Random(21)
    items = [(k, bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 120))))
             for k, _ in sb.mixed_pairs(600, 21)]
    present = [k for k, _ in items]
    absent = [sb.sha3(k + b'?') for k in present[:100]] + [present[0][:-1], present[1] + b'\x01']
    want = sb.host_build(sb.pairs(items))
    with mod.GpuStateStore(node_hint=1) as st:
        root = st.build_state(items)
        assert root == want.root == mod.build_host(items)[0]
        info = st.info()
        assert info['n_nodes'] == want.n_nodes and info['n_bytes'] == want.n_bytes
        assert info['n_unique'] == len(set(want.dig[i].tobytes() for i in range(want.n_nodes)))
        res = st.generate_state_proofs_batch([(root, k) for k in present + absent])
        assert [r[1] for r in res] == [v for _, v in items] + [None] * len(absent)
        assert st.get_for_root_hash_batch([(root, k) for k in present[:50]]) == [v for _, v in items[:50]]
        proof, val = st.generate_state_proof(present[5], root, serialize=True, get_value=True)
        assert val == mod.rlp_encode([items[5][1]])
    values = [v for _, v in items] + [None] * len(absent)
    ok = state_proofs.verify_state_proofs_batch([(root, k, v, r[0]) for k, v, r in zip(present + absent, values, res)])
    assert ok.all()


def test_overlapping_states_share_nodes(mod):
    items0 = [(k, b'value %d' % i * 3) for i, (k, _) in enumerate(sb.mixed_pairs(400, 22))]
    items1 = items0[:390] + [(k, b'changed') for k, _ in items0[390:]] + [(b'new key', b'new value')]
    with mod.GpuStateStore(node_hint=64) as st:
        r0, r1 = st.build_state(items0), st.build_state(items1)
        info = st.info()
        assert r0 != r1 and info['n_nodes'] - info['n_unique'] > 0
        a = st.get_for_root_hash_batch([(r0, k) for k, _ in items0])
        b = st.get_for_root_hash_batch([(r1, k) for k, _ in items1])
        assert a == [v for _, v in items0] and b == [v for _, v in items1]
        assert st.get_for_root_hash_batch([(r0, b'new key')]) == [None]


def test_state_root_batch_dispatch(mod, monkeypatch):
    items = next(c for c in sb.fixture() if c.name == 'mixed300').items
    root = next(c for c in sb.fixture() if c.name == 'mixed300').root
    assert len(items) >= mod.BUILD_GPU_MIN_ITEMS
    assert mod.state_root_batch(items) == root
    monkeypatch.setattr(mod, 'BUILD_GPU_MIN_ITEMS', 0)
    assert mod.state_root_batch([]) == mod.BLANK_ROOT
    assert mod.state_root_batch([(b'k', b'v')]) == mod.build_host([(b'k', b'v')])[0]


# ------------------------------------------------------------------ 4. refusals
def test_unsorted_and_duplicate_device_input(mod):
    prs = sb.mixed_pairs(200, 23)
    want = sb.host_build(prs)
    swapped = list(prs)
    swapped[120], swapped[121] = swapped[121], swapped[120]
    dup = prs[:70] + [prs[69]] + prs[70:]
    with mod.GpuStateStore(node_hint=1) as st:
        st.build_state([(b'seed', b'value')])
        before = st.info()
        for bad, idx in ((swapped, 121), (dup, 70), ([(b'ab', b'\x01'), (b'a', b'\x01')], 1)):
            got = device_build(bad, want.n_nodes, want.n_bytes, store=st._id)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'keys not strictly increasing at index {0} (key {0} is not above key {1})'.format(
                idx, idx - 1)
            assert st.info() == before
        got = device_build(prs[:10] + [(prs[10][0], b'')] + prs[11:], want.n_nodes, want.n_bytes, store=st._id)
        assert got.rc == EINVAL and got.untouched and last_error() == 'value 10 is empty or above 2^30 bytes'
        assert st.info() == before


def test_too_small_capacity_then_retry(mod):
    prs = sb.mixed_pairs(200, 24)
    want = sb.host_build(prs)
    with mod.GpuStateStore(node_hint=1) as st:
        before = st.info()
        for kw in ({'blob_cap': want.n_bytes - 1}, {'node_cap': want.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            got = device_build(prs, want.n_nodes, want.n_bytes, store=st._id, **kw)
            assert got.rc == EINVAL and got.untouched
            assert last_error() == 'node capacity too small: the build has {} nodes of {} bytes'.format(
                want.n_nodes, want.n_bytes)
            assert (got.n_nodes, got.n_bytes) == (want.n_nodes, want.n_bytes)
            assert st.info() == before
        got = device_build(prs, got.n_nodes, got.n_bytes, store=st._id)            # the retry, with the sizes reported
        assert want.same(got) is None
        assert st.info()['n_nodes'] == want.n_nodes
    # some outputs only: each capacity counts for the outputs it sizes (the digests alone need no blob_cap)
    from plenum_gpu import _native as nat
    kb, ko = sb.pack([k for k, _ in prs])
    vb, vo = sb.pack([v for _, v in prs])
    root, dig = np.zeros(32, np.uint8), np.zeros((want.n_nodes, 32), np.uint8)
    args = [kb.ctypes.data, ko.ctypes.data, vb.ctypes.data, vo.ctypes.data, len(prs), -1, root.ctypes.data_as(U8P),
            None, None]
    assert nat.load().pv_state_build(*args, None, 0, None, want.n_nodes, dig.ctypes.data) == OK
    assert root.tobytes() == want.root and (dig == want.dig).all()
    blob = np.zeros(want.n_bytes, np.uint8)
    assert nat.load().pv_state_build(*args, blob.ctypes.data, want.n_bytes, None, 0, None) == OK
    assert (blob == want.blob).all()
    assert nat.load().pv_state_build(*args, None, 1 << 40, None, want.n_nodes - 1, dig.ctypes.data) == EINVAL
    sizes = device_build(prs, 0, 0, outputs=False)                                 # no outputs: sizes and root alone
    assert (sizes.rc, sizes.root, sizes.n_nodes, sizes.n_bytes) == (OK, want.root, want.n_nodes, want.n_bytes)


def test_refusals(mod):
    from plenum_gpu import _native as nat
    lib = nat.load()
    import torch
    dev = torch.device('cuda:0')

    def err(rc, code, text):
        assert rc == code and last_error() == text, (rc, last_error())

    u64 = lambda *v: np.asarray(v, np.uint64)                                   # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rptr = lambda a: None if a is None else a.ctypes.data_as(U8P)              # noqa: E731
    root = np.zeros(32, np.uint8)
    keys = np.frombuffer(b'abcd' + b'\0' * 16, np.uint8).copy()
    vals = np.frombuffer(b'\x01\x02' + b'\0' * 16, np.uint8).copy()
    koff, voff = u64(0, 2, 4), u64(0, 1, 2)

    def build(kb=keys, ko=koff, vb=vals, vo=voff, n=2, store=-1, rt=root):
        return lib.pv_state_build(ptr(kb), ptr(ko), ptr(vb), ptr(vo), n, store, rptr(rt), None, None, None, 0, None, 0,
                                  None)

    assert build() == OK and root.tobytes() == mod.build_encoded_host([(b'ab', b'\x01'), (b'cd', b'\x02')])[0]
    # the empty batch: the blank root and sizes of 0 into whatever is given; the store is not looked at
    nn, nb, noff = ctypes.c_uint64(7), ctypes.c_uint64(7), u64(9, 9)
    assert lib.pv_state_build(None, None, None, None, 0, -1, rptr(root), ctypes.byref(nn), ctypes.byref(nb), None, 0,
                              ptr(noff), 0, None) == OK
    assert root.tobytes() == mod.BLANK_ROOT and (nn.value, nb.value, list(noff)) == (0, 0, [0, 9])
    assert build() == OK and build(n=0) == OK and root.tobytes() == mod.BLANK_ROOT
    assert lib.pv_state_build(None, None, None, None, 0, -1, None, None, None, None, 0, None, 0, None) == OK
    err(build(rt=None), EINVAL, 'null pointer')
    err(build(ko=None), EINVAL, 'null buffer')
    err(build(vo=None), EINVAL, 'null buffer')
    err(build(vb=None), EINVAL, 'null buffer')
    err(build(kb=None), EINVAL, 'null buffer')
    err(build(ko=u64(0, 3, 2)), EINVAL, 'key_off not monotone at 1')
    err(build(vo=u64(2, 1, 2)), EINVAL, 'val_off not monotone at 0')
    err(build(vo=u64(0, 1, 1)), EINVAL, 'value 1 is empty')
    for bad in (0, -2, 12345):
        err(build(store=bad), EINVAL, 'no state store with id {}'.format(bad))
    # the device form
    t = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
    d_k, d_v = t(keys), t(vals)
    d_ko, d_vo = t(koff.view(np.int64)), t(voff.view(np.int64))

    def dbuild(kb=d_k.data_ptr(), ko=d_ko.data_ptr(), vb=d_v.data_ptr(), vo=d_vo.data_ptr(), n=2, store=-1,
               rt=root, device=0):
        return lib.pv_state_build_device(kb, ko, vb, vo, n, store, rptr(rt), None, None, None, 0, None, 0, None, device,
                                         None)

    assert dbuild() == OK and root.tobytes() == mod.build_encoded_host([(b'ab', b'\x01'), (b'cd', b'\x02')])[0]
    d_noff = t(u64(9, 9).view(np.int64))
    nn, nb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.pv_state_build_device(None, None, None, None, 0, -1, rptr(root), ctypes.byref(nn), ctypes.byref(nb),
                                     None, 0, d_noff.data_ptr(), 0, None, 0, None) == OK
    assert root.tobytes() == mod.BLANK_ROOT and (nn.value, nb.value, d_noff.cpu().tolist()) == (0, 0, [0, 9])
    assert dbuild(n=0, rt=None, kb=None) == OK
    err(dbuild(rt=None), EINVAL, 'null pointer')
    err(dbuild(kb=None), EINVAL, 'null device buffer')
    err(dbuild(vo=None), EINVAL, 'null device buffer')
    err(dbuild(kb=d_k.data_ptr() + 1), EINVAL, 'key_blob and val_blob must be 4-byte aligned')
    err(dbuild(vb=d_v.data_ptr() + 2), EINVAL, 'key_blob and val_blob must be 4-byte aligned')
    err(dbuild(store=777), EINVAL, 'no state store with id 777')
    err(dbuild(device=63), ENOTINIT, 'device 63 not initialised (call pv_init)')
    d_back = t(u64(0, 3, 2).view(np.int64))
    err(dbuild(ko=d_back.data_ptr()), EINVAL,
        'key_off or val_off decreases, or a key is above 2^20 bytes, at index 1')
