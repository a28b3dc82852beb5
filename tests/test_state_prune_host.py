"""Pruning the resident trie store on the CPU: the Python mirror of the mark
(plenum_gpu.state_store.reachable_host) reproduces the set the reference keeps reachable from
headHash at every batch of both fixtures (tests/golden/state_update.json, state_remove.json); the
host build of csrc/pv_trie_prune.h (tools/hostcheck/stateprunecheck.cpp) agrees with the mirror
byte for byte on the kept digests and their order, the counts and the compacted store; the
stand-alone sanitizer program runs the same cases with exact-size buffers."""
import os
import subprocess

import pytest

import _state_prune as pr
import _trie_hostile as th
from plenum_gpu.state_proofs import BLANK_ROOT, PV_SP_MALFORMED, PV_SP_NODE_MISSING, PV_SP_OK
from plenum_gpu.state_store import apply_host, build_host, reachable_host, update_host, walk_host

FIXTURE = [n for n, _, _ in pr.fixture_cases()]
SHAPES = pr.shape_names()


@pytest.mark.parametrize('name', FIXTURE)
def test_mirror_matches_reference(name):
    """reachable_host from each batch's root over base + emitted == what the reference reaches"""
    mod, c = next((m, c) for n, m, c in pr.fixture_cases() if n == name)
    step = update_host if name.startswith('up/') else apply_host
    root, db = build_host(c.base)
    db = dict(db)
    assert root == c.base_root
    kept, missing, status, _ = reachable_host(db, [root])
    assert (kept, missing, status) == (c.base_reachable, 0, [PV_SP_OK])
    deepest = 0
    for b in c.batches:
        root, emitted = step(db, root, b.items)
        db.update(emitted)
        assert root == b.root
        kept, missing, status, d = reachable_host(db, [root])
        assert kept == b.reachable and missing == 0 and status == [PV_SP_OK]
        deepest = max(deepest, d)
    assert deepest <= 3                                 # extension -> branch -> leaf


def test_fixture_cases_carry_garbage():
    for name in ('rm/mixed300', 'up/mixed300'):
        nodes, roots = pr.filled(name)
        assert len(roots) == 6
        last, two = pr.Want(nodes, roots[-1:]), pr.Want(nodes, roots[-2:])
        assert last.n_kept < two.n_kept < len(set(nodes)) <= len(nodes)
        assert last.kept < two.kept


@pytest.mark.parametrize('name', SHAPES)
def test_host_twin_matches_mirror(name):
    nodes, roots = pr.filled(name)
    want = pr.check_host_equals_want(nodes, roots[-1:])
    assert want.n_missing == 0 and want.root_status == [PV_SP_OK]
    two = pr.check_host_equals_want(nodes, roots[-2:])
    assert want.kept <= two.kept
    if name[:3] in ('up/', 'rm/'):
        c = next(c for n, _, c in pr.fixture_cases() if n == name)
        assert want.kept == c.batches[-1].reachable
        before = c.batches[-2].reachable if len(c.batches) > 1 else c.base_reachable
        assert two.kept == want.kept | before
    # every root at once keeps every node some root reaches; the blank root adds nothing
    every = pr.check_host_equals_want(nodes, roots + [BLANK_ROOT])
    assert every.n_kept <= len(set(nodes)) and every.root_status == [PV_SP_OK] * (len(roots) + 1)


def test_walks_at_a_kept_root_are_unchanged_by_the_mirror_prune():
    nodes, roots = pr.filled('rm/mixed300')
    want = pr.Want(nodes, [roots[-1], roots[2]])
    full = {pr.sha3(n): n for n in nodes}
    part = dict(zip(want.digests, want.nodes))
    c = next(c for n, _, c in pr.fixture_cases() if n == 'rm/mixed300')
    keys = [k for k, _ in c.base] + [k for b in c.batches for k, _ in b.items]
    for root in (roots[-1], roots[2]):
        for k in keys:
            assert walk_host(part, root, k) == walk_host(full, root, k)
    assert walk_host(part, roots[0], keys[0])[0] in (PV_SP_NODE_MISSING, PV_SP_OK)
    assert roots[0] not in part


def test_chain_sizes_and_table_edges():
    junk, _ = pr.ext_chain(40, b'junk')
    for n in (1, 31, 32, 33, 63, 64, 65):
        chain, root = pr.ext_chain(n, b'kept')
        nodes = junk[:20] + chain + junk[20:] + chain      # the chain a second time: flagged duplicates
        want = pr.check_host_equals_want(nodes, [root])
        assert want.n_kept == n and want.n_slots == (64 if n <= 32 else 128 if n <= 64 else 256)
        assert want.digests == [pr.sha3(x) for x in chain]


def test_blank_root_alone_empties_the_store_and_a_missing_root_is_refused():
    nodes, roots = pr.filled('rm/mixed300')
    want = pr.check_host_equals_want(nodes, [BLANK_ROOT])
    assert (want.n_kept, want.bytes_kept, want.n_slots) == (0, 0, 64)
    wrong = pr.sha3(b'no such root')
    with pr.HostStore(nodes) as st:
        before = st.info()
        r = st.prune([roots[-1], wrong, roots[0]])
        assert (r['rc'], r['bad_root'], r['root_status']) == (pr.PR_ROOT_MISSING, 1, [PV_SP_OK, PV_SP_NODE_MISSING, PV_SP_OK])
        assert st.info() == before
        rep = st.prune([roots[-1], wrong, roots[0]], apply=False)
        assert rep['rc'] == pr.PR_OK and rep['n_kept'] == pr.Want(nodes, [roots[-1], roots[0]]).n_kept
        assert st.prune([], want_digests=False)['rc'] == pr.PR_NO_ROOTS
        need = st.prune(roots[-1:], apply=False)['n_kept']
        r = st.prune(roots[-1:], digest_cap=need - 1)
        assert (r['rc'], r['n_kept']) == (pr.PR_DIGEST_CAP, need) and st.info() == before


def test_a_value_that_looks_like_a_reference_is_not_followed():
    nodes, root, dropped = pr.value_trap()
    want = pr.check_host_equals_want(nodes, [root])
    assert want.n_kept == 2 and not (want.kept & dropped) and want.n_missing == 0


def test_a_malformed_inline_child_keeps_its_parent_and_hides_what_it_names():
    nodes, root, hidden, leaf = pr.malformed_parent()
    want = pr.check_host_equals_want(nodes, [root])
    assert want.kept == {root, leaf} and hidden not in want.kept
    full = {pr.sha3(n): n for n in nodes}
    part = dict(zip(want.digests, want.nodes))
    for db in (full, part):
        assert walk_host(db, root, b'\x00')[0] == PV_SP_MALFORMED
        assert walk_host(db, root, b'\x10\x08')[0] == PV_SP_OK
    # a stored node that is no trie node at all: kept when referenced, no children
    nodes2 = nodes + [b'\xc3\x01\x02\x03' + b'\x00' * 40]
    want = pr.check_host_equals_want(nodes2, [root, pr.sha3(nodes2[-1])])
    assert want.n_kept == 3


def test_partial_store_counts_missing_references():
    nodes, roots = pr.filled('rm/mixed300')
    full = {pr.sha3(n): n for n in nodes}
    c = next(c for n, _, c in pr.fixture_cases() if n == 'rm/mixed300')
    keys = [k for k, _ in c.base][:5]
    proof_nodes = [n for k in keys for n in walk_host(full, roots[-1], k)[1]]
    want = pr.check_host_equals_want(proof_nodes, roots[-1:])
    assert want.n_missing > 0 and want.kept == {pr.sha3(n) for n in proof_nodes}
    part = dict(zip(want.digests, want.nodes))
    for k in keys:
        assert walk_host(part, roots[-1], k) == walk_host(full, roots[-1], k)


def test_inline_nesting_up_to_the_limit_and_the_refusal_past_it():
    nodes, root, leaf = pr.nested(pr.MAX_INLINE)
    want = pr.check_host_equals_want(nodes, [root])
    assert want.kept == {root, leaf} and want.deepest == pr.MAX_INLINE
    nodes, root, leaf = pr.nested(pr.MAX_INLINE + 1)
    assert pr.Want(nodes, [root]).deepest == pr.MAX_INLINE + 1
    with pr.HostStore(nodes) as st:
        before, dump = st.info(), st.dump()
        for apply in (False, True):
            r = st.prune([root], apply=apply)
            assert r['rc'] == pr.PR_NESTING and r['root_status'] == [PV_SP_OK]
            assert st.info() == before and st.dump()[0] == dump[0]
        assert st.prune([leaf])['rc'] == pr.PR_OK          # the junk node is not reached: no refusal


def test_asan_program(tmp_path):
    """stateprunecheck_asan over every shape (last root, last two roots, all roots and the blank one)
    and the hand-encoded stores, each buffer at its exact size"""
    subprocess.run(['make', '-s', '-C', pr.HC_DIR, 'stateprunecheck_asan'], check=True)
    cases = []
    for name in SHAPES:
        nodes, roots = pr.filled(name)
        for keep in (roots[-1:], roots[-2:], roots + [BLANK_ROOT]):
            cases.append((nodes, keep, pr.Want(nodes, keep)))
    nodes, roots = pr.filled('rm/mixed300')
    keep = [roots[-1], pr.sha3(b'no such root'), BLANK_ROOT]
    cases.append((nodes, keep, pr.Want(nodes, keep)))
    cases.append((nodes, [BLANK_ROOT], pr.Want(nodes, [BLANK_ROOT])))
    cases.append(([], [BLANK_ROOT, pr.sha3(b'?')], pr.Want([], [BLANK_ROOT, pr.sha3(b'?')])))
    junk, _ = pr.ext_chain(40, b'junk')
    for n in (32, 33, 63, 64, 65):
        chain, root = pr.ext_chain(n, b'kept')
        nodes = junk[:20] + chain + junk[20:] + chain
        cases.append((nodes, [root], pr.Want(nodes, [root])))
    for nodes, root in (pr.value_trap()[:2], pr.malformed_parent()[:2], pr.nested(pr.MAX_INLINE)[:2]):
        cases.append((nodes, [root], pr.Want(nodes, [root])))
    nodes, root, _ = pr.nested(pr.MAX_INLINE + 1)
    cases.append((nodes, [root], None))
    full = {pr.sha3(n): n for n in pr.filled('rm/mixed300')[0]}
    proof = walk_host(full, roots[-1], next(iter(full.values()))[:3])[1]
    cases.append((proof, roots[-1:], pr.Want(proof, roots[-1:])))
    cases += [(row.nodes, [row.root], th.prune_want(row)) for row in th.ROWS]      # the hostile-node table
    assert any(w is not None and w.n_missing for _, _, w in cases)
    assert any(w is not None and PV_SP_NODE_MISSING in w.root_status for _, _, w in cases)
    path = os.path.join(str(tmp_path), 'cases.bin')
    pr.write_cases(path, cases)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(pr.HC_DIR, 'stateprunecheck_asan'), path], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors='replace')
    assert r.returncode == 0, out[-4000:]
    assert 'stateprunecheck ok: {} cases'.format(len(cases)) in out
