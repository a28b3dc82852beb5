"""The ledger write cycle on the resident Merkle tree (pv_merkle_tree_stage* /
_commit / _discard / _sizes / _frontier / _hash_store / _check_nodes,
plenum_gpu.ledger_tree.GpuLedgerTree) against the reference fixture
tests/golden/ledger_cycle.json, a second tree filled with extend_hashes, and
the hashlib restatement.  Everything is bit-exact."""
import ctypes
import hashlib

import numpy as np
import pytest

import _ledger_tree as lt
import _merkle as mk
import _merkle_proofs as mp

pytestmark = pytest.mark.gpu

PV_EINVAL = -22
U64_MAX = 2 ** 64 - 1
S = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


@pytest.fixture(scope='module')
def fx():
    return lt.fixture()


@pytest.fixture(scope='module')
def leaves():
    return mk.fixture()['leaves']


@pytest.fixture(scope='module')
def lh(leaves):
    return [mp.leaf(d) for d in leaves]


@pytest.fixture(scope='module')
def tree(lh):
    return mp.LevelTree(lh)


@pytest.fixture(scope='module')
def nat():
    from plenum_gpu import _native
    _native.ensure_init()
    return _native


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def _dig(items):
    return (np.frombuffer(b''.join(items), np.uint8).reshape(len(items), 32).copy() if items
            else np.zeros((0, 32), np.uint8))


def _rows(a):
    return [x.tobytes() for x in a]


class Tree:
    """one resident tree through the C ABI; every method returns (rc, ...) as the library answers"""

    def __init__(self, nat, hint=16):
        self.lib = nat.load()
        h = ctypes.c_int32(0)
        assert self.lib.pv_merkle_tree_create(hint, 0, ctypes.byref(h)) == 0
        self.h = h.value

    def free(self):
        return self.lib.pv_merkle_tree_free(self.h)

    def stage_hashes(self, hashes):
        arr, root = _dig(hashes), np.zeros(32, np.uint8)
        return self.lib.pv_merkle_tree_stage_hashes(self.h, _p(arr), len(hashes), _p(root)), root.tobytes()

    def stage(self, leaves):
        off = np.zeros(len(leaves) + 1, np.uint64)
        off[1:] = np.cumsum([len(d) for d in leaves])
        blob = np.frombuffer(b''.join(leaves) + b'\0' * 16, np.uint8).copy()
        root = np.zeros(32, np.uint8)
        return self.lib.pv_merkle_tree_stage(self.h, _p(blob), _p(off), len(leaves), _p(root)), root.tobytes()

    def extend_hashes(self, hashes):
        arr = _dig(hashes)
        return self.lib.pv_merkle_tree_extend_hashes(self.h, _p(arr), len(hashes))

    def commit(self, count):
        return self.lib.pv_merkle_tree_commit(self.h, count)

    def discard(self, count):
        root = np.zeros(32, np.uint8)
        return self.lib.pv_merkle_tree_discard(self.h, count, _p(root)), root.tobytes()

    def sizes(self):
        c, t = ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert self.lib.pv_merkle_tree_sizes(self.h, ctypes.byref(c), ctypes.byref(t)) == 0
        return c.value, t.value

    def info(self):
        n, depth, root = ctypes.c_uint64(0), ctypes.c_uint32(0), np.zeros(32, np.uint8)
        assert self.lib.pv_merkle_tree_info(self.h, ctypes.byref(n), ctypes.byref(depth), _p(root)) == 0
        return n.value, depth.value, root.tobytes()

    def frontier(self, size):
        out, cnt = np.zeros((64, 32), np.uint8), ctypes.c_uint32(99)
        rc = self.lib.pv_merkle_tree_frontier(self.h, size, _p(out), ctypes.byref(cnt))
        return rc, _rows(out[:cnt.value]) if rc == 0 else None

    def paths(self, pairs):
        """[(m, s)] -> ([path], [MTH(0, s)]) from one pv_merkle_audit_paths call"""
        if not pairs:
            return [], []
        _, depth, _ = self.info()
        index = np.array([m for m, _ in pairs], np.uint64)
        size = np.array([s for _, s in pairs], np.uint64)
        k = len(pairs)
        nodes, lens, roots = np.zeros((k, depth + 1, 32), np.uint8), np.zeros(k, np.uint32), np.zeros((k, 32), np.uint8)
        assert self.lib.pv_merkle_audit_paths(self.h, _p(index), _p(size), k, _p(nodes), _p(lens), _p(roots)) == 0
        return [_rows(nodes[i, :int(lens[i])]) for i in range(k)], _rows(roots)

    def hash_store(self, first, last, cap=None, slack=1):
        """-> (rc, n_nodes, leaf hashes, nodes); the outputs carry `slack` extra rows that must stay untouched"""
        need = lt.nodes_upto(last) - lt.nodes_upto(first) if first <= last else 0
        lo = np.full((max(last - first, 0) + slack, 32), 0xee, np.uint8)
        no = np.full((need + slack, 32), 0xee, np.uint8)
        n_nodes = ctypes.c_uint64(U64_MAX)
        rc = self.lib.pv_merkle_tree_hash_store(self.h, first, last, _p(lo), _p(no), need if cap is None else cap,
                                                ctypes.byref(n_nodes))
        return rc, n_nodes.value, lo, no

    def check_nodes(self, first, last, nodes):
        arr = _dig(nodes)
        bad, at = ctypes.c_uint64(77), ctypes.c_uint64(77)
        rc = self.lib.pv_merkle_tree_check_nodes(self.h, first, last, _p(arr), ctypes.byref(bad), ctypes.byref(at))
        return rc, bad.value, at.value


@pytest.fixture
def new_tree(nat):
    made = []

    def make(hint=16):
        made.append(Tree(nat, hint))
        return made[-1]
    yield make
    for t in made:
        t.free()


# ------------------------------------------------------------------ fixture replay
def test_c_abi_replays_the_fixture_cycle(fx, leaves, lh, tree, new_tree):
    t = new_tree()
    for i, s in enumerate(fx['steps']):
        _, total = t.sizes()
        root = None
        if s['op'] == 'stage':   # leaf data and leaf hashes in turn
            take = slice(total, total + s['count'])
            rc, root = t.stage(leaves[take]) if i % 2 else t.stage_hashes(lh[take])
            if not s['count']:   # an empty stage is PV_OK and writes nothing
                assert root == bytes(32), i
                root = None
        elif s['op'] == 'commit':
            rc = t.commit(s['count'])
        else:
            rc, root = t.discard(s['count'])
        assert rc == 0, i
        assert t.sizes() == (s['committed'], s['total']), i
        want_root = s['unc_root'] or s['committed_root']
        if root is not None:
            assert root == want_root, i
        n, depth, iroot = t.info()
        assert (n, iroot) == (s['total'], want_root), i
        assert depth == (max(s['total'] - 1, 0)).bit_length(), i
        assert t.frontier(s['total']) == (0, s['hashes']), i
        if s['committed']:
            assert t.paths([(0, s['committed'])])[1] == [s['committed_root']], i
            assert t.frontier(s['committed']) == (0, lt.frontier(tree, s['committed'])), i
    assert t.frontier(0) == (0, [])
    assert t.frontier(1031)[0] == PV_EINVAL


def test_python_class_replays_the_fixture_cycle(fx, leaves, nat):
    from plenum_gpu import GpuLedgerTree
    from plenum_gpu.exceptions import LogicError
    t = GpuLedgerTree(capacity_hint=8)
    try:
        assert t.uncommittedRootHash is None and t.size == 0 and t.hashes == ()
        assert t.committed_root_hash == t.uncommitted_root_hash == lt.EMPTY_ROOT
        assert t.appendTxns([]) == (0, 0) and t.uncommittedRootHash is None
        assert t.discardTxns(0) is None
        for i, s in enumerate(fx['steps']):
            total, committed, c = t.uncommitted_size, t.size, s['count']
            if s['op'] == 'stage':
                got = t.appendTxns(leaves[total:total + c])
                assert got == ((total + 1, total + c) if c else (total, total)), i
            elif s['op'] == 'commit':
                got = t.commitTxns(c)
                assert got == ((committed + 1, committed + c) if c else (committed, committed)), i
            else:
                assert t.discardTxns(c) is None
            assert (t.size, t.uncommitted_size, len(t), t.tree_size) == (s['committed'], s['total'], s['total'],
                                                                         s['total']), i
            assert t.sizes() == (s['committed'], s['total']), i
            assert t.uncommittedRootHash == s['unc_root'], i
            assert t.committed_root_hash == s['committed_root'], i
            assert t.uncommitted_root_hash == (s['unc_root'] or s['committed_root']), i
            assert t.root_hash == (s['unc_root'] or s['committed_root']), i
            assert t.hashes == tuple(s['hashes']), i
        with pytest.raises(LogicError) as ei:
            t.discardTxns(1)
        assert str(ei.value) == 'expected to revert 1 txns while there are only 0'
        t.appendTxns(leaves[:3])
        with pytest.raises(LogicError) as ei:
            t.discardTxns(4)
        assert str(ei.value) == 'expected to revert 4 txns while there are only 3'
        assert t.sizes() == (1030, 1033)
        t.reset_uncommitted()
        assert t.sizes() == (1030, 1030) and t.uncommittedRootHash is None
        assert t.root_hash == fx['steps'][-1]['committed_root']
    finally:
        t.close()


# --------------------------------------------------------------------- transitions
def test_every_transition_between_small_sizes(lh, tree, new_tree):
    """stage or discard between every two sizes of S on one tree with nothing committed: the
    root, every audit path at the new size (they read the repaired right edge) and every prefix root"""
    roots = {n: lt.root_of(lh[:n]) for n in S}
    small = {n: mp.LevelTree(lh[:n]) for n in S if n}
    want_paths = {n: [small[n].audit_path(m, n) for m in range(n)] for n in small}
    prefix = [tree.root(s) for s in range(1, max(S) + 1)]
    t = new_tree(hint=4)
    done = 0
    for a in S:
        for b in S:
            _, total = t.sizes()
            if total != a:
                rc, _ = t.stage_hashes(lh[total:a]) if a > total else t.discard(total - a)
                assert rc == 0
            rc, root = t.stage_hashes(lh[a:b]) if b > a else t.discard(a - b)
            assert rc == 0 and root == roots[b], (a, b)
            assert t.sizes() == (0, b), (a, b)
            if b:
                got, rts = t.paths([(m, b) for m in range(b)])
                assert got == want_paths[b], (a, b)
                assert set(rts) == {roots[b]}, (a, b)
                assert t.paths([(0, s) for s in range(1, b + 1)])[1] == prefix[:b], (a, b)
            done += 1
    assert done == len(S) ** 2


# ------------------------------------------------------- the kernel selection boundary
def _synthetic(n):
    return [hashlib.sha256(b'leaf-%d' % i).digest() for i in range(n)]


def _spread(n):
    want = {0, n - 1, n // 2, n // 3}
    p = 1
    while p < n:
        want |= {p - 1, p, p + 1}
        p *= 2
    return sorted(m for m in want if 0 <= m < n)


@pytest.mark.parametrize('n_old', [0, 1, 1000, 1024, 1025])
def test_stage_on_either_side_of_the_one_launch_limit(n_old, new_tree):
    """k up to 1024 leaves takes k_merkle_edge, more the per-level rebuild: both give the tree
    extend_hashes builds, and a discard gives the old one back"""
    hs = _synthetic(n_old + 2049)
    a = new_tree(hint=64)
    assert a.extend_hashes(hs[:n_old]) == 0
    old = (a.info(), a.paths([(m, n_old) for m in _spread(n_old)]))
    for k in (255, 256, 257, 1000, 1023, 1024, 1025, 2049):
        n = n_old + k
        b = new_tree(hint=n)
        assert b.extend_hashes(hs[:n]) == 0
        rc, root = a.stage_hashes(hs[n_old:n])
        assert rc == 0 and a.sizes() == (n_old, n) and b.sizes() == (n, n), k
        assert (n, a.info()[1], root) == b.info() == a.info(), k
        req = [(m, n) for m in _spread(n)] + [(m, s) for s in _spread(n)[1:] for m in (0, s - 1)]
        assert a.paths(req) == b.paths(req), k
        rc, root = a.discard(k)
        assert rc == 0 and a.sizes() == (n_old, n_old), k
        assert root == (old[0][2] if n_old else lt.EMPTY_ROOT), k
        assert (a.info(), a.paths([(m, n_old) for m in _spread(n_old)])) == old, k
        b.free()


# ------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(lh, new_tree):
    t = new_tree()
    assert t.extend_hashes(lh[:10]) == 0 and t.sizes() == (10, 10)
    assert t.stage_hashes(lh[10:15])[0] == 0
    before = (t.sizes(), t.info())
    assert before[0] == (10, 15)
    lib = t.lib
    assert t.discard(6)[0] == PV_EINVAL and b'expected to revert 6 txns' in lib.pv_last_error()
    assert t.commit(6) == PV_EINVAL
    assert t.extend_hashes(lh[15:16]) == PV_EINVAL and b'staged' in lib.pv_last_error()
    off, blob = np.array([0, 3], np.uint64), np.zeros(32, np.uint8)
    assert lib.pv_merkle_tree_extend(t.h, _p(blob), _p(off), 1) == PV_EINVAL
    assert (t.sizes(), t.info()) == before
    assert t.commit(2) == 0 and t.sizes() == (12, 15)
    assert t.discard(4)[0] == PV_EINVAL and t.discard(3) == (0, mp.LevelTree(lh[:12]).lv[-1][0])
    assert t.extend_hashes(lh[12:13]) == 0 and t.sizes() == (13, 13)     # nothing staged: extend commits
    gone = new_tree()
    assert gone.free() == 0
    root = np.zeros(32, np.uint8)
    c = ctypes.c_uint64(0)
    assert gone.stage_hashes(lh[:1])[0] == PV_EINVAL and gone.commit(0) == PV_EINVAL
    assert gone.discard(0)[0] == PV_EINVAL and gone.frontier(0)[0] == PV_EINVAL
    assert lib.pv_merkle_tree_sizes(gone.h, ctypes.byref(c), ctypes.byref(c)) == PV_EINVAL
    assert gone.hash_store(0, 0)[0] == PV_EINVAL and gone.check_nodes(0, 0, [])[0] == PV_EINVAL
    assert lib.pv_merkle_tree_stage(gone.h, _p(blob), _p(off), 1, _p(root)) == PV_EINVAL
    assert gone.free() == PV_EINVAL


# ---------------------------------------------------------------------- hash store
def _store_case(t, n, want_leafs, want_nodes):
    ranges = [(0, n), (0, 1), (n - 1, n), (5, 300), (256, 257), (7, 7)]
    for first, last in ranges:
        if last > n or first > last:
            assert t.hash_store(first, last)[0] == PV_EINVAL, (n, first, last)
            continue
        rc, cnt, lo, no = t.hash_store(first, last)
        lo_w, no_w = want_leafs[first:last], want_nodes[lt.nodes_upto(first):lt.nodes_upto(last)]
        assert (rc, cnt) == (0, len(no_w)), (n, first, last)
        assert _rows(lo[:-1]) == lo_w and _rows(no[:-1]) == no_w, (n, first, last)
        assert (lo[-1] == 0xee).all() and (no[-1] == 0xee).all(), (n, first, last)
        if no_w:   # a short node_cap: the need reported, nothing written
            rc, cnt, lo, no = t.hash_store(first, last, cap=len(no_w) - 1)
            assert (rc, cnt) == (PV_EINVAL, len(no_w)) and (lo == 0xee).all() and (no == 0xee).all()
        assert t.check_nodes(first, last, no_w) == (0, 0, U64_MAX), (n, first, last)
    assert t.check_nodes(0, n, want_nodes) == (0, 0, U64_MAX)
    if not want_nodes:
        return
    for at in (0, len(want_nodes) // 2, len(want_nodes) - 1):
        bad = list(want_nodes)
        bad[at] = bad[at][:9] + bytes([bad[at][9] ^ 0x10]) + bad[at][10:]
        assert t.check_nodes(0, n, bad) == (0, 1, at), (n, at)
    if len(want_nodes) >= 2:
        lo_at, hi_at = len(want_nodes) // 3, len(want_nodes) - 1
        bad = list(want_nodes)
        for at in (hi_at, lo_at):
            bad[at] = bytes([bad[at][0] ^ 1]) + bad[at][1:]
        assert t.check_nodes(0, n, bad) == (0, 1 if lo_at == hi_at else 2, lo_at), n


@pytest.mark.parametrize('n', [1, 2, 3, 1030])
def test_hash_store_in_the_fixture_order(n, fx, lh, new_tree):
    t = new_tree()
    assert t.stage_hashes(lh[:n])[0] == 0     # staged leaves are served like committed ones
    want = [h for e, _, h in fx['store_nodes'] if e <= n]
    assert len(want) == lt.nodes_upto(n)
    _store_case(t, n, lh[:n], want)


def test_hash_store_of_4099_leaves_in_closed_form(new_tree):
    n = 4099
    hs = _synthetic(n)
    t = new_tree(hint=n)
    assert t.extend_hashes(hs) == 0
    _store_case(t, n, hs, [h for _, _, h in lt.store_nodes(mp.LevelTree(hs), 0, n)])


# -------------------------------------------------------------------- device forms
def test_device_forms_give_the_host_forms_bytes(lh, new_tree):
    import torch
    a, b = new_tree(), new_tree()
    dev = torch.device('cuda:0')
    for lo, hi in [(0, 700), (700, 1030)]:
        rc, want_root = a.stage_hashes(lh[lo:hi])
        assert rc == 0
        d = torch.from_numpy(_dig(lh[lo:hi])).to(dev)
        root = np.zeros(32, np.uint8)
        stream = torch.cuda.current_stream().cuda_stream
        torch.cuda.synchronize()
        rc = b.lib.pv_merkle_tree_stage_hashes_device(b.h, ctypes.c_void_p(d.data_ptr()), hi - lo, _p(root),
                                                      ctypes.c_void_p(stream))
        assert rc == 0 and root.tobytes() == want_root
        assert b.lib.pv_merkle_tree_stage_hashes_device(b.h, ctypes.c_void_p(d.data_ptr()), 0, None,
                                                        ctypes.c_void_p(stream)) == 0
        assert a.info() == b.info() and a.sizes() == b.sizes() == (0, hi)
    for first, last in [(0, 1030), (5, 300), (1029, 1030)]:
        rc, need, lo_w, no_w = a.hash_store(first, last, slack=0)
        assert rc == 0
        dl = torch.full((last - first + 1, 32), 0xee, dtype=torch.uint8, device=dev)
        dn = torch.full((need + 1, 32), 0xee, dtype=torch.uint8, device=dev)
        cnt = ctypes.c_uint64(0)
        torch.cuda.synchronize()
        rc = b.lib.pv_merkle_tree_hash_store_device(b.h, first, last, ctypes.c_void_p(dl.data_ptr()),
                                                    ctypes.c_void_p(dn.data_ptr()), need, ctypes.byref(cnt),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and cnt.value == need
        hl, hn = dl.cpu().numpy(), dn.cpu().numpy()
        assert (hl[:-1] == lo_w).all() and (hn[:-1] == no_w).all()
        assert (hl[-1] == 0xee).all() and (hn[-1] == 0xee).all()
        if need:
            rc = b.lib.pv_merkle_tree_hash_store_device(b.h, first, last, None, ctypes.c_void_p(dn.data_ptr()),
                                                        need - 1, ctypes.byref(cnt), None)
            assert rc == PV_EINVAL and cnt.value == need
            assert (dn.cpu().numpy() == hn).all()     # nothing written


# -------------------------------------------------------------------- Python class
def test_python_class_writes_and_recovers_a_hash_store(fx, leaves, lh, nat):
    from plenum_gpu import GpuLedgerTree
    from plenum_gpu.exceptions import ConsistencyVerificationFailed
    store = lt.ListStore()
    t = GpuLedgerTree(hash_store=store)
    try:
        for s in fx['steps']:
            total = t.uncommitted_size
            if s['op'] == 'stage':
                t.appendTxns(leaves[total:total + s['count']])
            elif s['op'] == 'commit':
                t.commitTxns(s['count'])
                assert store.leafCount == s['committed'] and store.nodeCount == lt.nodes_upto(s['committed'])
            else:
                t.discardTxns(s['count'])
        assert store._leafs == lh and store._nodes == fx['store_nodes']
        root = t.root_hash
    finally:
        t.close()
    r = GpuLedgerTree.recover(store, 1030)
    try:
        assert r.sizes() == (1030, 1030) and r.root_hash == root and r.hashStore is store
        assert store.leafCount == 1030 and store.nodeCount == 1027       # recovery writes nothing back
        r.appendTxns([b'one more'])
        r.commitTxns(1)
        assert store.leafCount == 1031 and store._leafs[-1] == mp.leaf(b'one more')
        assert store.nodeCount == lt.nodes_upto(1031)
    finally:
        r.close()
    hash_only = lt.ListStore()     # a persistent store keeps the hashes alone
    hash_only._leafs, hash_only._nodes = list(lh), [h for _, _, h in fx['store_nodes']]
    r = GpuLedgerTree.recover(hash_only, 1030)
    assert r.root_hash == root
    r.close()
    for at in (0, 513, 1026):
        bad = lt.ListStore()
        bad._leafs, bad._nodes = list(lh), [h for _, _, h in fx['store_nodes']]
        bad._nodes[at] = bad._nodes[at][:5] + bytes([bad._nodes[at][5] ^ 2]) + bad._nodes[at][6:]
        with pytest.raises(ConsistencyVerificationFailed):
            GpuLedgerTree.recover(bad, 1030)
    with pytest.raises(ConsistencyVerificationFailed):
        GpuLedgerTree.recover(hash_only, 1029)
    hash_only._nodes.pop()
    with pytest.raises(ConsistencyVerificationFailed):
        GpuLedgerTree.recover(hash_only, 1030)


@pytest.mark.parametrize('gpu_batch', [False, True])
def test_catchup_accepts_the_longest_valid_prefix(gpu_batch, fx, leaves, tree, nat, monkeypatch):
    from plenum_gpu import GpuLedgerTree, merkle_proofs
    if gpu_batch:   # the three proofs through the batch kernel instead of the host walk
        monkeypatch.setattr(merkle_proofs, 'GPU_MIN_ITEMS', 0)
    cu = fx['catchup']
    for v in cu['variants']:
        reps, final_size, final_hash = lt.catchup_case(fx, leaves, v)
        t = GpuLedgerTree()
        try:
            t.extend(leaves[:cu['base']])
            assert t.accept_catchup_replies(reps, final_size, final_hash) == v['accepted'], v['what']
            end = ([cu['base']] + cu['ends'])[v['accepted']]
            assert t.sizes() == (end, end), v['what']
            assert t.root_hash == tree.root(end) and t.uncommittedRootHash is None, v['what']
        finally:
            t.close()
    assert [v['accepted'] for v in cu['variants']] == [3, 1, 2, 0]
