"""The ledger write cycle on the CPU: the hashlib mirror and the routines the
kernels run (csrc/pv_merkle_ledger.h, built for the host) against the
reference fixture tests/golden/ledger_cycle.json."""
import os
import subprocess

import pytest

import _ledger_tree as lt
import _merkle as mk
import _merkle_proofs as mp


@pytest.fixture(scope='module')
def fx():
    return lt.fixture()


@pytest.fixture(scope='module')
def lh():
    return [mp.leaf(d) for d in mk.fixture()['leaves']]


@pytest.fixture(scope='module')
def tree(lh):
    return mp.LevelTree(lh)


def test_fixture_covers_what_the_cycle_must_cross(fx):
    steps = fx['steps']
    assert len(steps) >= 40 and fx['n_leaves'] == 1030
    assert {1, 2, 3, 4, 8, 16, 32, 33, 64, 256, 257, 512, 1024} <= {s['total'] for s in steps}
    assert {s['op'] for s in steps} == {'stage', 'commit', 'discard'}
    assert any(s['op'] == 'discard' and s['unc_root'] is None for s in steps)       # reset_uncommitted
    assert any(s['op'] == 'discard' and s['unc_root'] is not None for s in steps)   # partial revert
    assert steps[-1]['committed'] == steps[-1]['total'] == 1030
    assert [v['accepted'] for v in fx['catchup']['variants']] == [3, 1, 2, 0]


def test_hashlib_mirror_reproduces_the_fixture(fx, lh, tree):
    m = lt.Mirror()
    for i, s in enumerate(fx['steps']):
        if s['op'] == 'stage':
            m.stage(lh[len(m.lh):len(m.lh) + s['count']])
        elif s['op'] == 'commit':
            m.commit(s['count'])
        else:
            m.discard(s['count'])
        assert m.state() == (s['committed'], s['total'], s['committed_root'], s['unc_root'], s['hashes']), i
    # the closed forms of the hash-store order against the reference's store
    assert lt.store_nodes(tree, 0, 1030) == fx['store_nodes']
    for e, h, _ in fx['store_nodes'][:300]:
        pos = [i for i, (e2, h2, _) in enumerate(fx['store_nodes'][:300]) if (e2, h2) == (e, h)]
        assert pos == [lt.nodes_upto(e - 1) + h - 1]
    assert len(fx['store_nodes']) == lt.nodes_upto(1030)


def test_header_routines_reproduce_the_fixture(fx, lh, tree):
    t = lt.HostTree()
    try:
        for i, s in enumerate(fx['steps']):
            _, total = t.sizes()
            if s['op'] == 'stage':
                root = t.stage(lh[total:total + s['count']])
            elif s['op'] == 'commit':
                assert t.commit(s['count']) == 0
                root = None
            else:
                rc, root = t.discard(s['count'])
                assert rc == 0
            assert t.sizes() == (s['committed'], s['total']), i
            if root is not None:
                assert root == (s['unc_root'] or s['committed_root']), i
            assert t.frontier(s['total']) == s['hashes'], i
            if s['committed']:
                assert t.frontier(s['committed']) == lt.frontier(tree, s['committed']), i
        n = 1030
        assert t.frontier(n + 1) is None and t.frontier(0) == []
        assert t.commit(1) == -22 and t.discard(1)[0] == -22 and t.sizes() == (n, n)
        want = [h for _, _, h in fx['store_nodes']]
        leafs, nodes = t.hash_store(0, n)
        assert leafs == lh and nodes == want
        for first, last in [(0, 1), (n - 1, n), (5, 300), (256, 257), (7, 7), (511, 1024)]:
            leafs, nodes = t.hash_store(first, last)
            assert leafs == lh[first:last]
            assert nodes == want[lt.nodes_upto(first):lt.nodes_upto(last)] == \
                [h for _, _, h in lt.store_nodes(tree, first, last)]
        assert t.check_nodes(0, n, want) == (0, None)
        for at in (0, len(want) // 2, len(want) - 1):
            bad = list(want)
            bad[at] = bytes([bad[at][0] ^ 4]) + bad[at][1:]
            assert t.check_nodes(0, n, bad) == (1, at)
        bad = list(want)
        for at in (700, 41):
            bad[at] = bad[at][:31] + bytes([bad[at][31] ^ 0x80])
        assert t.check_nodes(0, n, bad) == (2, 41)
    finally:
        t.close()


def test_header_routines_on_every_small_transition(lh):
    """stage or discard between every two sizes of S on one host tree: root and frontier"""
    sizes = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    roots = {n: lt.root_of(lh[:n]) for n in sizes}
    t = lt.HostTree()
    try:
        for a in sizes:
            for b in sizes:
                _, total = t.sizes()
                if total != a:
                    t.stage(lh[total:a]) if a > total else t.discard(total - a)
                root = t.stage(lh[a:b]) if b >= a else t.discard(a - b)[1]
                assert root == roots[b], (a, b)
                assert t.sizes() == (0, b)
    finally:
        t.close()


def test_python_names_exist():
    import plenum_gpu
    from plenum_gpu import exceptions
    assert plenum_gpu.GpuLedgerTree.__name__ == 'GpuLedgerTree'
    assert issubclass(plenum_gpu.GpuLedgerTree, plenum_gpu.GpuMerkleTree)
    assert issubclass(exceptions.LogicError, RuntimeError)
    assert issubclass(exceptions.ConsistencyVerificationFailed, Exception)
    for name in ('appendTxns', 'commitTxns', 'discardTxns', 'reset_uncommitted', 'frontier', 'recover',
                 'accept_catchup_replies'):
        assert callable(getattr(plenum_gpu.GpuLedgerTree, name))


def test_header_self_check_under_sanitizers():
    """tools/hostcheck/ledgercheck_main.cpp: its own process, built with
    AddressSanitizer + UBSan; every transition between 0..130 leaves into
    exactly-sized levels, every hash-store range and frontier up to 130"""
    subprocess.run(['make', '-s', '-C', lt.HC_DIR, 'ledgercheck_asan'], check=True)
    r = subprocess.run([os.path.join(lt.HC_DIR, 'ledgercheck_asan')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout
