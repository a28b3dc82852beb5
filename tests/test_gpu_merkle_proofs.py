"""Batched Merkle audit paths and consistency proofs on the GPU
(pv_merkle_verify_inclusion / _consistency, the resident tree pv_merkle_tree_*,
plenum_gpu.merkle_proofs) against the reference fixture
tests/golden/merkle_proofs.json, the per-proof routines built for the host
(tools/hostcheck/merklecheck.cpp) and the hashlib restatement."""
import ctypes
import hashlib

import numpy as np
import pytest

import _merkle as mk
import _merkle_proofs as mp

pytestmark = pytest.mark.gpu

PV_EINVAL = -22
STEPS = [1, 1, 3, 7, 16, 100, 5, 1, 300, 64, 2, 500]   # the steps of tests/golden/merkle_compact.json


@pytest.fixture(scope='module')
def fx():
    return mp.fixture()


@pytest.fixture(scope='module')
def leaves():
    return mk.fixture()['leaves']


@pytest.fixture(scope='module')
def tree(leaves):
    return mp.LevelTree([mp.leaf(d) for d in leaves])


@pytest.fixture(scope='module')
def host():
    """the per-proof routines on the host: (inclusion, consistency)"""
    so = mp.host_lib()
    return (lambda *a: mp.host_inclusion(so, *a)), (lambda *a: mp.host_consistency(so, *a))


@pytest.fixture(scope='module')
def nat():
    from plenum_gpu import _native
    _native.ensure_init()
    return _native


@pytest.fixture
def all_gpu(monkeypatch):
    from plenum_gpu import merkle_proofs
    monkeypatch.setattr(merkle_proofs, 'GPU_MIN_ITEMS', 0)


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def _dig(items):
    return np.frombuffer(b''.join(items), np.uint8).reshape(len(items), 32).copy() if items else np.zeros((0, 32),
                                                                                                           np.uint8)


def _pack(proofs):
    off = np.zeros(len(proofs) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in proofs])
    return _dig([h for p in proofs for h in p]), off


def gpu_inclusion(nat, items, root_table=None, leaf_data=None):
    """items: (leaf_hash, index, tree_size, path, root or root index) -> status, computed, stop"""
    n = len(items)
    index = np.array([it[1] for it in items], np.uint64)
    size = np.array([it[2] for it in items], np.uint64)
    nodes, poff = _pack([it[3] for it in items])
    if root_table is None:
        roots, ridx, nr = _dig([it[4] for it in items]), None, 0
    else:
        roots, ridx, nr = _dig(root_table), np.array([it[4] for it in items], np.uint32), len(root_table)
    if leaf_data is None:
        lh, blob, loff = _dig([it[0] for it in items]), None, None
    else:
        lh = None
        loff = np.zeros(n + 1, np.uint64)
        loff[1:] = np.cumsum([len(d) for d in leaf_data])
        blob = np.frombuffer(b''.join(leaf_data) + b'\0', np.uint8).copy()
    status, comp, stop = np.full(n, 0xee, np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint64)
    rc = nat.load().pv_merkle_verify_inclusion(_p(lh), _p(blob), _p(loff), _p(index), _p(size), _p(nodes), _p(poff),
                                               _p(roots), _p(ridx), nr, n, _p(status), _p(comp), _p(stop))
    assert rc == 0, nat.load().pv_last_error()
    return status, comp, stop


def gpu_consistency(nat, items):
    """items: (old, new, old_root, new_root, proof)"""
    n = len(items)
    old = np.array([it[0] for it in items], np.uint64)
    new = np.array([it[1] for it in items], np.uint64)
    r0, r1 = _dig([it[2] for it in items]), _dig([it[3] for it in items])
    nodes, poff = _pack([it[4] for it in items])
    status, c0, c1 = np.full(n, 0xee, np.uint8), np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    rc = nat.load().pv_merkle_verify_consistency(_p(old), _p(new), _p(r0), _p(r1), None, None, 0, _p(nodes), _p(poff),
                                                 n, _p(status), _p(c0), _p(c1))
    assert rc == 0, nat.load().pv_last_error()
    return status, c0, c1


def incl_items(fx, tree):
    """every inclusion row of the fixture a 64-bit interface can carry, with the expectation"""
    items, want = [], []
    for r in fx['audit_paths']:
        rt = bytes.fromhex(fx['roots'][str(r['s'])])
        items.append((tree.lv[0][r['m']], r['m'], r['s'], mp.unhex(r['path']), rt))
        want.append((mp.OK, rt, 0))
    for r in fx['neg_inclusion'] + fx['wide']:
        if not mp.negative(r):
            items.append((bytes.fromhex(r['leaf_hash']), r['index'], r['tree_size'], mp.unhex(r['path']),
                          bytes.fromhex(r['root'])))
            want.append(mp.expect_inclusion(r))
    return items, want


def cons_items(fx):
    items, want = [], []
    for r in fx['consistency']:
        a, b = r['a'], r['b']
        rb = bytes.fromhex(fx['roots'][str(b)])
        items.append((a, b, bytes.fromhex(fx['roots'][str(a)]) if a else rb, rb, mp.unhex(r['proof'])))
        want.append((mp.OK, None, None))
    for r in fx['neg_consistency']:
        if not mp.negative(r):
            items.append((r['old'], r['new'], bytes.fromhex(r['old_root']), bytes.fromhex(r['new_root']),
                          mp.unhex(r['proof'])))
            want.append(mp.expect_consistency(r))
    return items, want


def _same_as_host_incl(host, items, got):
    status, comp, stop = got
    for j, it in enumerate(items):
        st, c, sp = host[0](*it)
        assert (int(status[j]), comp[j].tobytes(), int(stop[j])) == (st, c, sp), j


def test_every_inclusion_row_through_the_c_abi(nat, host, fx, tree):
    items, want = incl_items(fx, tree)
    assert len(items) >= 550 and any(it[2] >= 2 ** 63 for it in items)
    got = gpu_inclusion(nat, items)
    _same_as_host_incl(host, items, got)
    for j, (st, comp, stop) in enumerate(want):
        assert int(got[0][j]) == st, j
        if comp is not None:
            assert got[1][j].tobytes() == comp, j
        if stop is not None:
            assert int(got[2][j]) == stop, j


def test_every_consistency_row_through_the_c_abi(nat, host, fx):
    items, want = cons_items(fx)
    status, c0, c1 = gpu_consistency(nat, items)
    for j, it in enumerate(items):
        assert (int(status[j]), c0[j].tobytes(), c1[j].tobytes()) == host[1](*it), j
    for j, (st, w0, w1) in enumerate(want):
        assert int(status[j]) == st, j
        if w0 is not None:
            assert c0[j].tobytes() == w0, j
        if w1 is not None:
            assert c1[j].tobytes() == w1, j


def _exc_class(name):
    from plenum_gpu import exceptions
    return ValueError if name == 'ValueError' else getattr(exceptions, name)


def _assert_outcomes(rows, got):
    assert len(got) == len(rows)
    for r, e in zip(rows, got):
        if r['exc'] is None:
            assert e is None, (r['what'], e)
        else:
            assert type(e) is _exc_class(r['exc']) and str(e) == r['msg'], (r['what'], e)


def test_python_batches_return_the_reference_exceptions(all_gpu, nat, fx, tree, leaves):
    from plenum_gpu.merkle_proofs import STH, GpuMerkleVerifier
    v = GpuMerkleVerifier()
    rows = fx['neg_inclusion'] + fx['wide']
    got = v.verify_leaf_hash_inclusion_batch([bytes.fromhex(r['leaf_hash']) for r in rows],
                                             [r['index'] for r in rows], [mp.unhex(r['path']) for r in rows],
                                             [STH(r['tree_size'], bytes.fromhex(r['root'])) for r in rows])
    _assert_outcomes(rows, got)
    rows = fx['neg_consistency']
    got = v.verify_tree_consistency_batch([(r['old'], r['new'], bytes.fromhex(r['old_root']),
                                            bytes.fromhex(r['new_root']), mp.unhex(r['proof'])) for r in rows])
    _assert_outcomes(rows, got)
    # the positive rows, from the leaf data, and operands that are not 32 bytes long
    ap = fx['audit_paths']
    sths = [STH(r['s'], bytes.fromhex(fx['roots'][str(r['s'])])) for r in ap]
    got = v.verify_leaf_inclusion_batch([leaves[r['m']] for r in ap], [r['m'] for r in ap],
                                        [mp.unhex(r['path']) for r in ap], sths)
    assert got == [None] * len(ap)
    odd = v.verify_leaf_hash_inclusion_batch([b'short', tree.lv[0][0]], [0, 0], [[tree.lv[0][1]], [b'x' * 31]],
                                             [STH(2, tree.root(2)), STH(2, tree.root(2))])
    want = [v._single(v.verify_leaf_hash_inclusion, b'short', 0, [tree.lv[0][1]], STH(2, tree.root(2))),
            v._single(v.verify_leaf_hash_inclusion, tree.lv[0][0], 0, [b'x' * 31], STH(2, tree.root(2)))]
    assert [(type(e), str(e)) for e in odd] == [(type(e), str(e)) for e in want]
    assert all(type(e).__name__ == 'ProofError' for e in odd)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_partial_waves_and_blocks(nat, host, fx, tree, n):
    items, _ = incl_items(fx, tree)
    pick = [items[(7 * j) % len(items)] for j in range(n)]
    _same_as_host_incl(host, pick, gpu_inclusion(nat, pick))
    citems, _ = cons_items(fx)
    cpick = [citems[(5 * j) % len(citems)] for j in range(n)]
    status, c0, c1 = gpu_consistency(nat, cpick)
    for j, it in enumerate(cpick):
        assert (int(status[j]), c0[j].tobytes(), c1[j].tobytes()) == host[1](*it), j


def test_zero_levels_beside_depth_ten_in_one_wave(nat, host, tree):
    items = []
    for j in range(64):
        if j % 2:
            m = (37 * j) % 1000
            items.append((tree.lv[0][m], m, 1000, tree.audit_path(m, 1000), tree.root(1000)))
        else:
            items.append((tree.lv[0][0], 0, 1, [], tree.lv[0][0] if j % 4 else tree.lv[0][1]))
    assert max(len(it[3]) for it in items) == 10
    got = gpu_inclusion(nat, items)
    _same_as_host_incl(host, items, got)
    assert [int(s) for s in got[0]] == [mp.OK if j % 4 else mp.ROOT_MISMATCH for j in range(64)]


def test_shared_root_table(nat, host, tree):
    sizes = [70, 513, 1030]
    table = [tree.root(s) for s in sizes]
    items, plain = [], []
    for j in range(200):
        t = j % 3
        s = sizes[t]
        m = (91 * j) % s
        ridx = t if j % 11 else (t + 1) % 3      # every eleventh proof points at a wrong root
        items.append((tree.lv[0][m], m, s, tree.audit_path(m, s), ridx))
        plain.append(items[-1][:4] + (table[ridx],))
    got = gpu_inclusion(nat, items, root_table=table)
    _same_as_host_incl(host, plain, got)
    assert [int(s) for s in got[0]] == [mp.OK if j % 11 else mp.ROOT_MISMATCH for j in range(200)]
    # a root index outside the table is refused before any launch
    index = np.zeros(1, np.uint64)
    size = np.ones(1, np.uint64)
    poff = np.zeros(2, np.uint64)
    lh, roots, ridx = _dig([tree.lv[0][0]]), _dig(table), np.array([3], np.uint32)
    status, comp, stop = np.full(1, 0xee, np.uint8), np.zeros((1, 32), np.uint8), np.zeros(1, np.uint64)
    rc = nat.load().pv_merkle_verify_inclusion(_p(lh), None, None, _p(index), _p(size), None, _p(poff), _p(roots),
                                               _p(ridx), 3, 1, _p(status), _p(comp), _p(stop))
    assert rc == PV_EINVAL and status[0] == 0xee


def test_leaf_mode_hashes_the_leaves_on_the_gpu(nat, host, tree, leaves):
    by_len = {}
    for i, d in enumerate(leaves):
        by_len.setdefault(len(d), i)
    picks = [by_len[k] for k in (0, 1, 55, 56, 4097)]
    items = [(tree.lv[0][m], m, 1030, tree.audit_path(m, 1030), tree.root(1030)) for m in picks]
    items.append((tree.lv[0][picks[4]], picks[4], 1030, tree.audit_path(picks[4], 1030), tree.root(1029)))
    data = [leaves[it[1]] for it in items]
    got = gpu_inclusion(nat, items, leaf_data=data)
    _same_as_host_incl(host, items, got)
    assert [int(s) for s in got[0]] == [mp.OK] * 5 + [mp.ROOT_MISMATCH]


def _paths_equal(t, tree, pairs):
    got = t.inclusion_proofs(pairs)
    for (m, s), p in zip(pairs, got):
        assert p == tree.audit_path(m, s), (m, s)


def test_tree_extend_sequence_keeps_every_path(nat, tree, leaves):
    from plenum_gpu.merkle_proofs import GpuMerkleTree
    states = mk.compact_fixture()
    t = GpuMerkleTree(capacity_hint=4)
    assert t.root_hash == hashlib.sha256(b'').digest() and t.tree_size == 0
    pos = 0
    for k, state in zip(STEPS, states):
        t.extend(leaves[pos:pos + k])
        pos += k
        assert t.tree_size == pos == state['tree_size']
        assert t.root_hash.hex() == state['root'], pos
        assert t.depth == (pos - 1).bit_length()
        for s in sorted({pos, 1, pos // 2, pos - 1} - {0}):
            _paths_equal(t, tree, [(m, s) for m in range(s)])
            assert t.merkle_tree_hash(0, s) == tree.root(s)
    assert pos == 1000
    with pytest.raises(NotImplementedError):
        t.merkle_tree_hash(1, 5)
    with pytest.raises(ValueError):
        t.merkle_tree_hash(5, 5)
    t.close()


@pytest.fixture(scope='module')
def gpu_tree(nat, leaves):
    from plenum_gpu.merkle_proofs import GpuMerkleTree
    t = GpuMerkleTree(capacity_hint=64)
    t.extend(leaves[:700])
    for d in leaves[700:703]:
        t.append(d)
    t.extend_hashes([mp.leaf(d) for d in leaves[703:]])
    yield t
    t.close()


def test_ledger_dicts_and_consistency_proofs(gpu_tree, fx, tree):
    from plenum_gpu import base58
    b58 = lambda h: base58._py_b58encode(h).decode()   # noqa: E731
    assert gpu_tree.tree_size == 1030 and gpu_tree.root_hash == tree.root(1030)
    seq = [1, 2, 3, 64, 65, 512, 513, 1029, 1030]
    assert gpu_tree.merkle_infos(seq) == [
        {'rootHash': b58(tree.root(s)), 'auditPath': [b58(h) for h in tree.audit_path(s - 1, s)]} for s in seq]
    assert gpu_tree.audit_proofs(seq) == [
        {'rootHash': b58(tree.root(1030)), 'auditPath': [b58(h) for h in tree.audit_path(s - 1, 1030)],
         'ledgerSize': 1030} for s in seq]
    for bad in (0, -4):
        with pytest.raises(ValueError, match="variable 'seqNo', value {}, expected: > 0".format(bad)):
            gpu_tree.merkle_infos([1, bad])
        with pytest.raises(ValueError):
            gpu_tree.audit_proofs([bad])
    rows = fx['consistency']
    got = gpu_tree.consistency_proofs([(r['a'], r['b']) for r in rows])
    assert [[h.hex() for h in p] for p in got] == [r['proof'] for r in rows]
    assert gpu_tree.consistency_proof(512, 1030) == tree.consistency_proof(512, 1030)
    pairs = [(a, b) for b in range(1, 71) for a in range(1, b + 1)]
    d = hashlib.sha256()
    for p in gpu_tree.consistency_proofs(pairs):
        d.update(b''.join(p))
    assert d.hexdigest() == fx['digest_cons_le70']
    d = hashlib.sha256()
    for p in gpu_tree.inclusion_proofs([(m, s) for s in range(1, 71) for m in range(s)]):
        d.update(b''.join(p))
    assert d.hexdigest() == fx['digest_paths_le70']
    rows = fx['audit_paths']
    got = gpu_tree.inclusion_proofs([(r['m'], r['s']) for r in rows])
    assert [[h.hex() for h in p] for p in got] == [r['path'] for r in rows]


def test_large_tree_paths_and_proofs_verify(nat):
    from plenum_gpu.merkle_proofs import GpuMerkleTree
    n = 2 ** 16 + 3
    hashes = [hashlib.sha256(i.to_bytes(8, 'little')).digest() for i in range(n)]
    ref = mp.LevelTree(hashes)
    t = GpuMerkleTree(capacity_hint=1024)
    arr = np.frombuffer(b''.join(hashes), np.uint8).reshape(n, 32)
    t.extend_hashes(arr[:40000])
    t.extend_hashes(arr[40000:])
    assert t.root_hash == ref.root(n) and t.depth == 17
    rng = np.random.default_rng(6962)
    size = rng.integers(1, n + 1, 4096).astype(np.uint64)
    size[:64] = n                                    # the whole tree: read from the levels, nothing hashed
    size[64:72] = [1, 2, 3, 2 ** 16, 2 ** 16 + 1, 2 ** 16 + 2, 4097, 32768]
    index = (rng.integers(0, 2 ** 62, 4096).astype(np.uint64) % size).astype(np.uint64)
    index[:2] = [0, n - 1]
    nodes, lens, roots = t.paths_arrays(index, size)
    for j in range(4096):
        m, s = int(index[j]), int(size[j])
        assert [nodes[j, i].tobytes() for i in range(int(lens[j]))] == ref.audit_path(m, s), (m, s)
        assert roots[j].tobytes() == ref.root(s), s
    # the generated paths, fed back: every one verifies
    keep = np.arange(nodes.shape[1])[None, :] < lens[:, None]
    flat = np.ascontiguousarray(nodes[keep])
    poff = np.zeros(4097, np.uint64)
    poff[1:] = np.cumsum(lens)
    lh = np.ascontiguousarray(arr[index.astype(np.int64)])
    status, comp, stop = np.full(4096, 0xee, np.uint8), np.zeros((4096, 32), np.uint8), np.zeros(4096, np.uint64)
    rc = nat.load().pv_merkle_verify_inclusion(_p(lh), None, None, _p(index), _p(size), _p(flat), _p(poff),
                                               _p(roots), None, 0, 4096, _p(status), _p(comp), _p(stop))
    assert rc == 0 and not status.any() and (comp == roots).all()
    second = rng.integers(2, n + 1, 1024).astype(np.uint64)
    second[:16] = n
    first = (1 + rng.integers(0, 2 ** 62, 1024).astype(np.uint64) % (second - 1)).astype(np.uint64)
    first[16:20] = second[16:20]
    first[20:24] = 0
    pn, pl = t.proofs_arrays(first, second)
    for j in range(1024):
        a, b = int(first[j]), int(second[j])
        assert [pn[j, i].tobytes() for i in range(int(pl[j]))] == ref.consistency_proof(a, b), (a, b)
    keep = np.arange(pn.shape[1])[None, :] < pl[:, None]
    flat = np.ascontiguousarray(pn[keep])
    poff = np.zeros(1025, np.uint64)
    poff[1:] = np.cumsum(pl)
    r0 = _dig([ref.root(int(a)) if a else ref.root(1) for a in first])
    r1 = _dig([ref.root(int(b)) for b in second])
    status, c0, c1 = np.full(1024, 0xee, np.uint8), np.zeros((1024, 32), np.uint8), np.zeros((1024, 32), np.uint8)
    rc = nat.load().pv_merkle_verify_consistency(_p(first), _p(second), _p(r0), _p(r1), None, None, 0, _p(flat),
                                                 _p(poff), 1024, _p(status), _p(c0), _p(c1))
    assert rc == 0 and not status.any()
    t.close()


def test_refusals_return_einval_and_write_nothing(nat, gpu_tree):
    lib = nat.load()
    h = gpu_tree._h()
    stride = gpu_tree.depth + 1

    def paths(handle, index, size):
        index, size = np.array(index, np.uint64), np.array(size, np.uint64)
        k = len(index)
        nodes, lens, roots = np.full((k, stride, 32), 0xee, np.uint8), np.full(k, 0xeeeeeeee, np.uint32), \
            np.full((k, 32), 0xee, np.uint8)
        rc = lib.pv_merkle_audit_paths(handle, _p(index), _p(size), k, _p(nodes), _p(lens), _p(roots))
        return rc, (nodes == 0xee).all() and (lens == 0xeeeeeeee).all() and (roots == 0xee).all()

    assert paths(h, [0, 5], [1030, 1030]) == (0, False)
    assert paths(h, [0, 7], [1030, 7]) == (PV_EINVAL, True)        # index >= tree_size
    assert paths(h, [0, 7], [1030, 1031]) == (PV_EINVAL, True)     # tree_size > n
    assert paths(h, [0, 0], [1030, 0]) == (PV_EINVAL, True)        # tree_size == 0
    first, second = np.array([3, 9], np.uint64), np.array([8, 8], np.uint64)
    nodes, lens = np.full((2, stride, 32), 0xee, np.uint8), np.full(2, 0xeeeeeeee, np.uint32)
    assert lib.pv_merkle_consistency_proofs(h, _p(first), _p(second), 2, _p(nodes), _p(lens)) == PV_EINVAL
    second[1] = 1031
    first[1] = 5
    assert lib.pv_merkle_consistency_proofs(h, _p(first), _p(second), 2, _p(nodes), _p(lens)) == PV_EINVAL
    assert (nodes == 0xee).all() and (lens == 0xeeeeeeee).all()
    # a freed handle, a handle that never was
    hh = ctypes.c_int32(0)
    assert lib.pv_merkle_tree_create(4, 0, ctypes.byref(hh)) == 0 and hh.value > 0 and hh.value != h
    assert lib.pv_merkle_tree_free(hh.value) == 0
    assert paths(hh.value, [0], [1]) == (PV_EINVAL, True)
    assert lib.pv_merkle_tree_free(hh.value) == PV_EINVAL
    assert lib.pv_merkle_tree_extend_hashes(hh.value, _p(np.zeros(32, np.uint8)), 1) == PV_EINVAL
    assert paths(12345, [0], [1]) == (PV_EINVAL, True) and paths(0, [0], [1]) == (PV_EINVAL, True)
    n = ctypes.c_uint64(0)
    assert lib.pv_merkle_tree_info(hh.value, ctypes.byref(n), None, None) == PV_EINVAL
    assert b'handle' in lib.pv_last_error()
