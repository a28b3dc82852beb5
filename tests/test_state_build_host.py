"""Batch trie build on the CPU: the Python mirror (plenum_gpu.state_store.build_host), the host
build of csrc/pv_trie_build.h (tools/hostcheck/statebuildcheck.cpp) and the fixture recorded
from the reference (tests/golden/state_build.json) agree on the root and on the set of node
digests; the stand-alone sanitizer program runs the same cases with exact-size buffers."""
import os
import subprocess

import pytest

import _state_build as sb
import _state_store as ss
from plenum_gpu.state_proofs import BLANK_ROOT
from plenum_gpu.state_store import build_encoded_host, build_host, walk_host

CASES = [c.name for c in sb.fixture()]


def case(name):
    return next(c for c in sb.fixture() if c.name == name)


def test_fixture_covers_the_cases_of_the_issue():
    assert len(CASES) == 18 and len(set(CASES)) == 18
    assert case('empty').root == BLANK_ROOT and case('empty').digests == []
    assert len(case('mixed300').items) == 300
    keys = [k for k, _ in case('overwritten').items]
    assert len(keys) > len(set(keys))
    assert any(k == b'' for k, _ in case('empty_key').items)


@pytest.mark.parametrize('name', CASES)
def test_mirror_matches_reference(name):
    c = case(name)
    root, db = build_host(c.items)
    assert root == c.root
    assert sorted(db) == c.digests
    assert all(sb.sha3(n) == h for h, n in db.items())
    if c.items:
        assert all(len(n) >= 32 for h, n in db.items() if h != root)


@pytest.mark.parametrize('name', CASES)
def test_host_build_matches_reference_and_mirror(name):
    c = case(name)
    b = sb.host_build_cached('fx/' + name, sb.pairs(c.items))
    assert b.rc == sb.OK
    assert b.root == c.root
    assert sorted(set(b.db())) == c.digests
    assert b.db() == build_host(c.items)[1]
    assert int(b.off[0]) == 0 and int(b.off[b.n_nodes]) == b.n_bytes == len(b.blob)


def test_identical_sibling_leaves_are_both_emitted():
    b = sb.host_build_cached('fx/identical_leaves', sb.pairs(case('identical_leaves').items))
    nodes = b.nodes()
    assert len(nodes) == len(set(nodes)) + 1


def test_short_root_is_emitted():
    b = sb.host_build_cached('fx/short_root', sb.pairs(case('short_root').items))
    assert b.n_nodes == 1 and b.n_bytes < 32 and sb.sha3(b.nodes()[0]) == b.root


def test_proof_fixture_tries():
    """the five tries of tests/golden/state_proofs.json: root and exactly their node set"""
    tries = sb.proof_fixture_tries()
    assert len(tries) == 5
    for name, prs, root, db in tries:
        m_root, m_db = build_encoded_host(prs)
        assert m_root == root and m_db == db, name
        b = sb.host_build_cached('pf/' + name, prs)
        assert b.rc == sb.OK and b.root == root and b.db() == db, name


def test_mirror_matches_the_recursive_builder():
    prs = sb.mixed_pairs(500, 7)
    assert build_encoded_host(prs) == ss.build_trie(prs)


@pytest.mark.parametrize('name', [n for n, _ in sb.boundary_pairs()])
def test_list_header_boundaries(name):
    prs = dict(sb.boundary_pairs())[name]
    b = sb.host_build_cached('bd/' + name, prs)
    root, db = build_encoded_host(prs)
    assert b.rc == sb.OK and b.root == root and b.db() == db
    if name.startswith('leaf'):
        assert b.n_bytes == int(name[4:])


def test_chain_is_the_deepest_trie():
    prs = sb.chain_pairs()
    b = sb.host_build_cached('chain', prs)
    root, db = build_encoded_host(prs)
    assert b.rc == sb.OK and b.root == root and b.db() == db
    assert b.max_level == 63
    assert sum(1 for n in db.values() if len(ss_decode(n)) == 17) == 63


def ss_decode(node):
    from plenum_gpu.state_store import rlp_decode
    return rlp_decode(node)


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 66, 4095, 4096, 4097, 5000])
def test_sizes_around_the_tree_blocks(n):
    """n + 1 h-values fill 64-entry blocks of the min tree: one short, exact, one over"""
    prs = sb.random_pairs(n, 100 + n, klen=3 if n > 300 else 2)
    b = sb.host_build(prs)
    root, db = build_encoded_host(prs)
    assert b.rc == sb.OK and b.root == root and b.db() == db


def test_proofs_from_the_built_nodes():
    """every key walks to its value over the nodes the host build emitted"""
    prs = sb.mixed_pairs(200, 3)
    b = sb.host_build(prs)
    db = b.db()
    for k, v in prs:
        st, nodes, value, proof, _ = walk_host(db, b.root, k)
        assert st == 0 and value == v


def test_repeated_runs_are_byte_identical():
    prs = sb.mixed_pairs(300, 5)
    a, b = sb.host_build(prs), sb.host_build(prs)
    assert a.same(b) is None and a.n_nodes > 300


def test_refusals_name_the_first_index():
    prs = sb.mixed_pairs(100, 9)
    swapped = list(prs)
    swapped[40], swapped[41] = swapped[41], swapped[40]
    b = sb.host_build(swapped)
    assert (b.rc, b.bad_index, b.n_nodes) == (sb.BAD_ORDER, 41, 0)
    dup = prs[:70] + [prs[69]] + prs[70:]
    b = sb.host_build(dup)
    assert (b.rc, b.bad_index) == (sb.BAD_ORDER, 70)
    b = sb.host_build([(b'ab', b'\x01'), (b'a', b'\x01')])          # a proper prefix must come first
    assert (b.rc, b.bad_index) == (sb.BAD_ORDER, 1)
    empty = prs[:10] + [(prs[10][0], b'')] + prs[11:]
    b = sb.host_build(empty)
    assert (b.rc, b.bad_index) == (sb.BAD_VALUE, 10)


def test_too_small_capacity_reports_sizes_and_writes_nothing():
    prs = sb.mixed_pairs(100, 11)
    full = sb.host_build(prs)
    for kw in ({'blob_cap': full.n_bytes - 1}, {'node_cap': full.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
        b = sb.host_build(prs, **kw)
        assert b.rc == sb.TOO_SMALL and (b.n_nodes, b.n_bytes) == (full.n_nodes, full.n_bytes)
        assert b.untouched and b.root == full.root


def test_each_capacity_counts_for_its_own_outputs():
    """the digests alone need no blob capacity, the blob alone no node capacity"""
    import ctypes
    import numpy as np
    import _state_proofs as sp
    prs = sb.mixed_pairs(60, 12)
    full = sb.host_build(prs)
    kb, ko = sb.pack([k for k, _ in prs])
    vb, vo = sb.pack([v for _, v in prs])
    root, nn, nb = np.zeros(32, np.uint8), ctypes.c_uint64(0), ctypes.c_uint64(0)
    args = [sp.ptr(kb), sp.ptr(ko), sp.ptr(vb), sp.ptr(vo), len(prs), sp.ptr(root), ctypes.byref(nn), ctypes.byref(nb)]
    dig, blob = np.zeros((full.n_nodes, 32), np.uint8), np.zeros(full.n_bytes, np.uint8)
    so = sb.host_lib()
    assert so.sb_build(*args, None, 0, None, full.n_nodes, sp.ptr(dig), None, None) == sb.OK and (dig == full.dig).all()
    assert so.sb_build(*args, sp.ptr(blob), full.n_bytes, None, 0, None, None, None) == sb.OK
    assert (blob == full.blob).all()
    assert so.sb_build(*args, None, 1 << 40, None, full.n_nodes - 1, sp.ptr(dig), None, None) == sb.TOO_SMALL


def test_mirror_restores_the_recursion_limit():
    import sys
    before = sys.getrecursionlimit()
    levels = before + 200                       # a chain of branches deeper than the interpreter's limit
    keys = []
    for i in range(levels):
        nib = [7] * levels
        nib[i] = 3
        keys.append(bytes(16 * nib[2 * j] + nib[2 * j + 1] for j in range(levels // 2)))
    prs = sorted((k, b'\xc2\x81\x99') for k in set(keys))
    root, db = build_encoded_host(prs)
    assert sb.host_build(prs).root == root and sys.getrecursionlimit() == before


def test_last_of_equal_keys_wins():
    items = case('overwritten').items
    final = dict(items)
    assert build_host(items) == build_host(list(final.items()))
    assert build_host(items)[0] != build_host(list(dict(reversed(items)).items()))[0]


def test_dispatch_threshold_is_named():
    from plenum_gpu import state_store
    assert isinstance(state_store.BUILD_GPU_MIN_ITEMS, int) and state_store.BUILD_GPU_MIN_ITEMS >= 1
    small = case('dogs').items
    assert len(small) < state_store.BUILD_GPU_MIN_ITEMS
    assert state_store.state_root_batch(small) == case('dogs').root    # the mirror: no GPU here


def test_asan_program(tmp_path):
    """statebuildcheck_asan: every fixture case, the boundaries, the chain, the tree-block sizes
    and the refusals, each buffer at its exact size, plus the too-small-capacity path"""
    subprocess.run(['make', '-s', '-C', sb.HC_DIR, 'statebuildcheck_asan'], check=True)
    cases = [sb.pairs(c.items) for c in sb.fixture()]
    cases += [prs for _, prs in sb.boundary_pairs()]
    cases += [sb.chain_pairs(), sb.random_pairs(63, 1), sb.random_pairs(64, 2), sb.random_pairs(65, 3),
              sb.random_pairs(4096, 4, klen=3), sb.mixed_pairs(300, 5)]
    bad = sb.mixed_pairs(50, 6)
    bad[20], bad[21] = bad[21], bad[20]
    cases += [bad, [(b'a', b'\x01'), (b'a', b'\x02')], [(b'a', b'\x01'), (b'b', b'')]]
    path = os.path.join(str(tmp_path), 'cases.bin')
    sb.write_cases(path, [(prs, sb.host_build(prs)) for prs in cases])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(sb.HC_DIR, 'statebuildcheck_asan'), path], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors='replace')
    assert r.returncode == 0, out[-4000:]
    assert '{} cases ok'.format(len(cases)) in out
