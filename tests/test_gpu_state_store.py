"""The resident trie node store on the GPU (pv_state_store_*, k_trie_store_insert /
_rehash, k_trie_prove, k_trie_proof_pack) against the host build of the same header
(tools/hostcheck/statestorecheck.cpp), the Python mirror and the reference fixture.
The scenarios are those of tests/test_state_store_host.py (tests/_state_store.py)."""
import ctypes
import random

import numpy as np
import pytest

import _state_proofs as sp
import _state_store as ss

pytestmark = pytest.mark.gpu

OK, EINVAL, ENOTINIT = 0, -22, -77


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


def run_gpu(mod, sc, node_hint=1):
    """one scenario on the device and on the host build: every field and byte must agree"""
    batches, roots, ridx, keys, max_nodes = sc
    host = ss.HostStore(node_hint)
    with mod.GpuStateStore(node_hint=node_hint) as st:
        for b in batches:
            assert st.add_nodes(b) == host.add(b)
        assert st.info() == host.info()
        got = st.prove(roots, ridx, keys, max_nodes)
    want = host.prove(roots, ridx, keys, max_nodes)
    assert want.same(got, ids=False) is None, want.same(got, ids=False)
    return got, host


# ------------------------------------------------------------------ 1. the fixture in one store
def test_fixture_in_one_store(mod, monkeypatch):
    from plenum_gpu import state_proofs
    from plenum_gpu.state_proofs import rlp_split_list
    tr = ss.tries()
    names = sorted(tr)
    nodes = [n for name in names for n in tr[name][1].values()] + ss.extra_nodes()
    assert len(ss.extra_nodes()) > 0 and len(nodes) == 365 + len(ss.extra_nodes())
    a, b = nodes[:150], nodes[:75] + nodes[150:260]          # the second add repeats half of the first
    c = nodes[260:]
    host = ss.HostStore(1)
    with mod.GpuStateStore(node_hint=1) as st:
        assert st.info() == {'n_nodes': 0, 'n_unique': 0, 'n_bytes': 0, 'n_slots': 64}
        added, dig = st.add_nodes(a, want_digests=True)
        assert added == 150 and dig == [ss.sha3(n) for n in a]
        assert st.add_nodes(b) == 110 and st.add_nodes(c) == len(c)
        for batch in (a, b, c):
            host.add(batch)
        info = st.info()
        assert info == host.info()
        assert info['n_nodes'] == len(nodes) + 75 and info['n_unique'] == len(nodes)
        assert info['n_bytes'] == sum(len(n) for n in a + b + c) and info['n_slots'] >= 2 * info['n_nodes']
        rows = ss.proof_rows()
        roots, ridx = [tr[n][0] for n in names], [names.index(r.trie) for r in rows]
        keys = [r.kvs[0][0] for r in rows]
        got = st.prove(roots, ridx, keys)
        batch = st.generate_state_proofs_batch([(r.root, r.kvs[0][0]) for r in rows])
    want = host.prove(roots, ridx, keys)
    assert want.same(got, ids=False) is None, want.same(got, ids=False)
    assert len(rows) == 409 and (got.status == ss.OK).all()
    for q, r in enumerate(rows):
        proof = got.proof(q)
        split = [proof[x:y] for x, y in rlp_split_list(proof)]
        assert sorted(split) == sorted(r.nodes) and ss.sha3(split[-1]) == r.root
        assert got.value(q) == sp.encode_value(r.kvs[0][1])
        assert batch[q] == (proof, r.kvs[0][1])
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    ok = state_proofs.verify_state_proofs_batch([(r.root, r.kvs[0][0], r.kvs[0][1], got.proof(q))
                                                 for q, r in enumerate(rows)])
    assert ok.all()


def test_python_interface(mod):
    from plenum_gpu.state_proofs import BLANK_ROOT
    tr = ss.tries()
    rows = [r for r in ss.proof_rows()][::40]
    with mod.GpuStateStore(node_hint=8) as st:
        for r in ss.proof_rows():
            if r.kind == 'own':
                st.add_serialized_proof(r.serialized)
        assert st.info()['n_unique'] == 365
        for r in rows:
            key, value = r.kvs[0]
            root_node = sp.decode(next(n for n in r.nodes if ss.sha3(n) == r.root))
            proof, val = st.generate_state_proof(key, r.root, serialize=True, get_value=True)
            assert val == (sp.encode_value(value) or None)
            nodes = st.generate_state_proof(key, root_node)          # a decoded root node, unserialized
            assert sorted(mod.rlp_encode(n) for n in nodes) == sorted(r.nodes) and nodes[-1] == root_node
            assert st.generate_state_proof(key.decode('latin-1') if max(key, default=0) < 128 else key, r.root,
                                           serialize=True) == proof
        assert st.get_for_root_hash_batch([(r.root, r.kvs[0][0]) for r in rows]) == [r.kvs[0][1] for r in rows]
        assert st.generate_state_proof(b'k', BLANK_ROOT, serialize=True, get_value=True) == (b'\xc0', None)
        assert st.generate_state_proof(b'k', b'') == []
        with pytest.raises(KeyError):
            st.generate_state_proof(b'k', b'\x11' * 32)
        with pytest.raises(KeyError):
            st.get_for_root_hash_batch([(b'\x11' * 32, b'k')])
        assert st.generate_state_proofs_batch([(b'\x11' * 32, b'k'), (BLANK_ROOT, b'k')]) == [None, (b'\xc0', None)]
        assert st.generate_state_proofs_batch([]) == [] and st.add_nodes([]) == 0
    assert len(tr) == 5


# ------------------------------------------------------------------ 2. - 5., 9.
def test_history_on_the_device(mod):
    kv0, kv1, _, _ = ss.history()
    got, _ = run_gpu(mod, ss.sc_history())
    keys = sorted(set(kv0) | set(kv1))
    for q, k in enumerate(keys):
        assert got.value(q) == kv0.get(k, b'') and got.value(len(keys) + q) == kv1.get(k, b'')
    q = keys.index(next(iter(set(kv0) - set(kv1))))
    assert got.val_len[q] > 0 and got.val_len[len(keys) + q] == 0 and got.status[len(keys) + q] == ss.OK


def test_missing_nodes_unknown_root_blank_root(mod):
    cases = ss.sc_missing()
    assert len(cases) - 1 >= 6
    for i, sc in enumerate(cases[:-1]):
        got, _ = run_gpu(mod, sc)
        assert got.status[0] == ss.NODE_MISSING and got.node_count[0] == i and got.proof_off[1] == 0
    got, _ = run_gpu(mod, cases[-1])
    assert got.status.tolist() == [ss.NODE_MISSING, ss.OK] and got.node_count.tolist() == [0, 0]
    assert got.proof(0) == b'' and got.proof(1) == b'\xc0'


def test_path_too_long_and_retry(mod):
    batches, roots, ridx, keys, max_nodes = ss.sc_too_long()
    got, host = run_gpu(mod, (batches, roots, ridx, keys, max_nodes))
    assert max_nodes == 2 and (got.status == ss.PATH_TOO_LONG).all() and (got.node_count == 9).all()
    assert got.proof_off[-1] == 0
    again, _ = run_gpu(mod, (batches, roots, ridx, keys, int(got.node_count.max())))
    assert (again.status == ss.OK).all() and (again.node_count == 9).all()


def test_list_header_boundaries_on_the_device(mod):
    got, _ = run_gpu(mod, ss.sc_boundaries())
    sizes = (55, 56, 255, 256, 65535, 65536)
    assert [int(got.proof_off[q + 1] - got.proof_off[q]) - n for q, n in enumerate(sizes)] == [1, 2, 2, 3, 3, 4]
    root, db, value = ss.leaf_trie(70000)                  # a 70 KB leaf
    got, _ = run_gpu(mod, ([list(db.values())], [root], None, [b'k'], None))
    assert got.value(0) == value and len(got.proof(0)) == 70004


def test_hostile_root_nodes_on_the_device(mod):
    """well-defined inputs that the walk must bound-check; the statuses are the host build's"""
    got, _ = run_gpu(mod, ss.sc_hostile())
    assert set(got.status.tolist()) <= {ss.OK, ss.NODE_MISSING, ss.MALFORMED} and (got.status == ss.MALFORMED).any()


# ------------------------------------------------------------------ 6. the device forms
def test_device_forms_give_the_host_forms_bytes(mod):
    import torch
    from plenum_gpu import _native as nat
    lib = nat.load()
    batches, roots, ridx, keys, _ = ss.sc_built()
    host = ss.HostStore(1)
    host.add(batches[0])
    want = host.prove(roots, ridx, keys)
    n, max_nodes = len(keys), want.max_nodes
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                  # noqa: E731
    nblob, noff = ss.pack(batches[0])
    kblob, koff = ss.pack(keys)
    with mod.GpuStateStore(node_hint=1) as st:
        d_nblob, d_noff = t(nblob), t(noff.view(np.int64))
        dig = torch.zeros(len(batches[0]) * 32, dtype=torch.uint8, device=dev)
        nat._check('add_device', lib.pv_state_store_add_device(st._id, p(d_nblob), p(d_noff), len(batches[0]), p(dig),
                                                               None))
        assert dig.cpu().numpy().tobytes() == b''.join(ss.sha3(x) for x in batches[0])
        assert st.info() == host.info()
        d_roots = t(np.frombuffer(b''.join(roots), np.uint8).copy())
        d_ridx, d_kblob, d_koff = t(np.asarray(ridx, np.int32)), t(kblob), t(koff.view(np.int64))
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        count = torch.zeros(n, dtype=torch.int32, device=dev)
        ids = torch.zeros(n * max_nodes, dtype=torch.int32, device=dev)
        plen, vrel, vlen = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
        nat._check('walk_device', lib.pv_state_store_walk_device(
            st._id, p(d_roots), p(d_ridx), len(roots), p(d_kblob), p(d_koff), n, max_nodes, p(status), p(count),
            p(ids), p(plen), p(vrel), p(vlen), None))
        poff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        poff[1:] = torch.cumsum(plen, 0)
        total = int(poff[-1])
        out = torch.zeros(total, dtype=torch.uint8, device=dev)
        nat._check('pack_device', lib.pv_state_store_pack_device(st._id, p(ids), p(count), max_nodes, p(poff), n,
                                                                 p(out), None))
        torch.cuda.synchronize()
    got = ss.Result(n, max_nodes)
    got.status, got.node_count = status.cpu().numpy(), count.cpu().numpy().view(np.uint32)
    got.node_ids = ids.cpu().numpy().view(np.uint32).reshape(n, max_nodes)
    got.proof_off = poff.cpu().numpy().view(np.uint64)
    got.val_rel, got.val_len = vrel.cpu().numpy().view(np.uint64), vlen.cpu().numpy().view(np.uint64)
    got.blob = out.cpu().numpy()
    assert want.same(got) is None, want.same(got)


# ------------------------------------------------------------------ 7. scale
@pytest.fixture(scope='module')
def big():
    """the 4,096-key trie and 65,536 queries, a quarter of them absent keys of each kind"""
    from plenum_gpu.state_proofs import rlp_encode
    rng = random.Random(1600)
    kv = []
    for i in range(4096):
        key = ss.sha3(b'did:%d' % i) if i % 3 else b'attr:%d' % i
        kv.append((key, rlp_encode([bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 250)))])))
    root, db = ss.build_trie(kv)
    present = [k for k, _ in kv]
    keys = [present[rng.randrange(4096)] for _ in range(49152)] + ss.absent_keys(rng, present, 16384)
    rng.shuffle(keys)
    return root, db, dict(kv), keys


def test_scale_65536_queries(mod, big):
    root, db, kv, keys = big
    nodes = list(db.values())
    got, host = run_gpu(mod, ([nodes], [root], [0] * len(keys), keys, None), node_hint=len(nodes))
    assert (got.status == ss.OK).all()
    absent = int((got.val_len == 0).sum())
    assert absent == sum(k not in kv for k in keys) == 16384
    pick = list(range(0, len(keys), len(keys) // 2000))[:2000]
    want = ss.mirror_prove(host.db, host.id_of, [root], [0] * len(pick), [keys[q] for q in pick])
    for i, q in enumerate(pick):
        assert got.proof(q) == want.proof(i) and got.value(q) == kv.get(keys[q], b'')


def test_scale_duplicate_heavy_batches(mod, big):
    """64 adds into a store that starts at 64 slots, each batch holding every one of its nodes
    twice plus nodes of earlier batches: lanes of one launch race for the same slots"""
    root, db, kv, keys = big
    nodes = list(db.values())
    rng = random.Random(7)
    step = (len(nodes) + 63) // 64
    host = ss.HostStore(1)
    with mod.GpuStateStore(node_hint=1) as st:
        total = 0
        for i in range(64):
            chunk = nodes[i * step:(i + 1) * step]
            batch = chunk + chunk + [nodes[rng.randrange(max(i * step, 1))] for _ in range(50)]
            rng.shuffle(batch)
            assert st.add_nodes(batch) == host.add(batch)
            total += len(batch)
        info = st.info()
        assert info == host.info()
        assert info['n_unique'] == len(db) and info['n_nodes'] == total
        got = st.prove([root], [0] * 4096, keys[:4096])
    want = host.prove([root], [0] * 4096, keys[:4096])
    assert want.same(got, ids=False) is None and (got.status == ss.OK).all()


# ------------------------------------------------------------------ 8. refusals and their texts
def test_refusals_and_their_texts(mod):
    from plenum_gpu import _native as nat
    lib = nat.load()
    u64 = lambda *v: np.array(v, np.uint64)     # noqa: E731
    u32 = lambda *v: np.array(v, np.uint32)     # noqa: E731
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)   # noqa: E731
    sid = ctypes.c_int32(0)

    def err(rc, want_rc, text):
        assert rc == want_rc and lib.pv_last_error().decode() == text, (rc, lib.pv_last_error())

    # device 99 first, also with every pointer NULL
    err(lib.pv_state_store_create(1, 1, 99, ctypes.byref(sid)), ENOTINIT, 'device 99 not initialised (call pv_init)')
    err(lib.pv_state_store_create(1, 1, 99, None), ENOTINIT, 'device 99 not initialised (call pv_init)')
    err(lib.pv_state_store_create(1, 1, 0, None), EINVAL, 'null pointer')
    err(lib.pv_state_store_create(1 << 32, 1, 0, ctypes.byref(sid)), EINVAL, 'node_hint above 2^32 - 2 nodes')
    assert lib.pv_state_store_create(1, 0, 0, ctypes.byref(sid)) == OK and sid.value > 0
    s = sid.value
    node = np.frombuffer(b'\xc5\x83\x20\x6b\x31\x76', np.uint8).copy()
    status, count = np.zeros(2, np.uint8), np.zeros(2, np.uint32)
    poff, vrel, vlen = np.full(3, 77, np.uint64), np.zeros(2, np.uint64), np.zeros(2, np.uint64)
    roots = np.frombuffer(ss.sha3(node.tobytes()) * 2, np.uint8).copy()
    keys = np.frombuffer(b'k1k2', np.uint8).copy()
    blob = np.zeros(64, np.uint8)
    one, three, back = u64(0, 6), u64(0, 3, 3, 6), u64(0, 4, 2)

    def prove(store=s, roots=roots, ridx=None, n_roots=2, kblob=keys, koff=u64(0, 2, 4), nq=2, max_nodes=5,
              status=status, proof_blob=blob, cap=64):
        return lib.pv_state_store_prove(store, ptr(roots), ptr(ridx), n_roots, ptr(kblob), ptr(koff), nq, max_nodes,
                                        ptr(status), ptr(count), ptr(poff), ptr(vrel), ptr(vlen), ptr(proof_blob), cap)

    # zero counts with NULL buffers: PV_OK, nothing launched
    assert lib.pv_state_store_add(s, None, None, 0, None, None) == OK
    assert lib.pv_state_store_add_device(s, None, None, 0, None, None) == OK
    assert lib.pv_state_store_prove(s, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, 0) == OK
    assert lib.pv_state_store_walk_device(s, None, None, 0, None, None, 0, 0, *([None] * 7)) == OK
    assert lib.pv_state_store_pack_device(s, None, None, 0, None, 0, None, None) == OK
    assert lib.pv_state_store_info(s, None, None, None, None) == OK
    # a freed or foreign store, before the count and the buffers are looked at
    for bad in (0, -1, s + 1000):
        text = 'no state store with id {}'.format(bad)
        err(lib.pv_state_store_add(bad, None, None, 0, None, None), EINVAL, text)
        err(lib.pv_state_store_add_device(bad, None, None, 1, None, None), EINVAL, text)
        err(lib.pv_state_store_info(bad, None, None, None, None), EINVAL, text)
        err(prove(store=bad), EINVAL, text)
        err(lib.pv_state_store_walk_device(bad, None, None, 0, None, None, 0, 0, *([None] * 7)), EINVAL, text)
        err(lib.pv_state_store_pack_device(bad, None, None, 0, None, 0, None, None), EINVAL, text)
        err(lib.pv_state_store_free(bad), EINVAL, text)
    # NULL buffers
    err(lib.pv_state_store_add(s, None, ptr(one), 1, None, None), EINVAL, 'null buffer')
    err(lib.pv_state_store_add(s, ptr(node), None, 1, None, None), EINVAL, 'null buffer')
    err(lib.pv_state_store_add_device(s, None, None, 1, None, None), EINVAL, 'null device buffer')
    err(prove(roots=None), EINVAL, 'null buffer')
    err(prove(status=None), EINVAL, 'null buffer')
    err(prove(kblob=None), EINVAL, 'null buffer')
    err(lib.pv_state_store_walk_device(s, None, None, 1, None, None, 1, 1, *([None] * 7)), EINVAL,
        'null device buffer')
    err(lib.pv_state_store_pack_device(s, None, None, 1, None, 1, None, None), EINVAL, 'null device buffer')
    # an empty node; offsets that go back
    err(lib.pv_state_store_add(s, ptr(node), ptr(three), 3, None, None), EINVAL,
        'node_off not strictly increasing at 1 (an empty node)')
    err(lib.pv_state_store_add(s, ptr(node), ptr(back), 2, None, None), EINVAL,
        'node_off not strictly increasing at 1 (an empty node)')
    info = [ctypes.c_uint64(9) for _ in range(4)]
    assert lib.pv_state_store_info(s, *[ctypes.byref(x) for x in info]) == OK
    assert [x.value for x in info] == [0, 0, 0, 64]          # nothing was added by the refused calls
    added = ctypes.c_uint64(0)
    assert lib.pv_state_store_add(s, ptr(node), ptr(one), 1, None, ctypes.byref(added)) == OK
    assert added.value == 1
    # the prove call's own checks, in this order
    err(prove(max_nodes=0, koff=u64(0, 4, 2)), EINVAL, 'max_nodes must be >= 1')
    err(prove(n_roots=0), EINVAL, 'queries without roots')
    err(prove(n_roots=1), EINVAL, '1 roots for 2 queries without root_idx')
    err(prove(koff=u64(0, 4, 2), ridx=u32(0, 2)), EINVAL, 'key_off not monotone at 1')
    err(prove(ridx=u32(0, 2)), EINVAL, 'root_idx[1] = 2 is not below n_roots 2')
    assert (poff == 77).all()                                 # ... before anything is written
    # proof_cap too small: both numbers, and proof_off is already valid
    # (k1 is the leaf's key; k2 is proven absent by the same leaf: two proofs of 1 + 6 bytes)
    err(prove(cap=13), EINVAL, 'proof_cap 13 is below the 14 bytes of the proofs')
    assert poff.tolist() == [0, 7, 14] and status.tolist() == [ss.OK, ss.OK] and count.tolist() == [1, 1]
    assert vlen.tolist() == [1, 0] and vrel.tolist() == [6, 0]
    assert not blob.any()
    poff[:] = 77
    assert prove(proof_blob=None, cap=0) == OK and poff.tolist() == [0, 7, 14] and not blob.any()   # the sizing call
    assert prove(cap=14) == OK and blob[:14].tobytes() == (b'\xc6' + node.tobytes()) * 2 and not blob[14:].any()
    assert lib.pv_state_store_free(s) == OK
    err(lib.pv_state_store_free(s), EINVAL, 'no state store with id {}'.format(s))
    err(prove(), EINVAL, 'no state store with id {}'.format(s))
