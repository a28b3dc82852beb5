"""Sets and removals onto a committed root on the CPU: the Python mirror
(plenum_gpu.state_store.apply_host), the host build of csrc/pv_trie_update.h in its removal mode +
pv_trie_build.h (tools/hostcheck/stateapplycheck.cpp) and the fixture recorded from the reference
(tests/golden/state_remove.json) agree on the root after every batch and on the nodes; the
stand-alone sanitizer program runs the same cases with exact-size buffers."""
import os
import subprocess

import pytest

import _state_apply as sa
import _state_build as sb
import _state_update as su
import _trie_hostile as th
from plenum_gpu.state_proofs import BLANK_ROOT, PV_SP_MALFORMED, PV_SP_NODE_MISSING, rlp_encode
from plenum_gpu.state_store import (ITEM_SUBTREE, ITEM_VALUE, apply_encoded_host, apply_host, build_encoded_host,
                                    build_host, merge_host, update_encoded_host, update_host, walk_host)

CASES = [c.name for c in sa.fixture()]
SHAPES = [s[0] for s in sa.shapes()]


def shape(name):
    return next(s for s in sa.all_shapes() if s[0] == name)


def test_fixture_covers_the_cases_of_the_issue():
    assert len(CASES) == 29 and len(set(CASES)) == 29
    kinds = ('hashed_leaf', 'inline_leaf', 'extension', 'hashed_branch', 'inline_branch')
    assert all('collapse_%s_%s' % (w, k) in CASES for w in ('root', 'under_extension') for k in kinds)
    for c in sa.fixture():
        assert build_host(c.base)[0] == c.base_root
    assert sa.case('every_key_removed').batches[0].root == BLANK_ROOT
    assert sa.case('only_key_removed').batches[0].root == BLANK_ROOT
    c = sa.case('absent_removals')
    assert len(c.batches) == 7 and all(b.root == c.base_root and not b.added for b in c.batches)
    c = sa.case('empty_key_removed_from_a_state_without_it')
    assert c.batches[0].root == c.base_root
    assert [len(b.items) for b in sa.case('full_branch_loses_14_then_15').batches] == [14, 1]
    assert any(len(v) == 3000 for _, v in sa.case('big_leaf_lengthened_by_a_collapse').base)
    state = dict(sa.case('mixed300').base)
    for b in sa.case('mixed300').batches:
        sets = sum(v is not None for _, v in b.items)
        present = sum(v is None and k in state for k, v in b.items)
        absent = sum(v is None and k not in state for k, v in b.items)
        assert (sets, present, absent) == (30, 20, 10)
        for k, v in b.items:
            state[k] = v
            if v is None:
                del state[k]


@pytest.mark.parametrize('name', CASES)
def test_mirror_matches_reference(name):
    c = sa.case(name)
    root, db = build_host(c.base)
    assert root == c.base_root and set(db) == c.base_reachable
    state, gone = dict(c.base), set()
    for b in c.batches:
        held = set(db)
        new_root, emitted = apply_host(db, root, b.items)
        assert new_root == b.root
        assert all(sb.sha3(n) == h for h, n in emitted.items())
        assert set(emitted) <= b.reachable              # only nodes of the new trie are emitted
        assert b.added <= set(emitted)                  # all that is new to the reference's trie is
        db.update(emitted)
        assert b.reachable <= set(db)                   # base and emitted hold all of it
        if new_root == root:                            # nothing changed: nothing the store lacks
            assert set(emitted) <= held
        for k, v in b.items:
            if v is None:
                state.pop(k, None)
                gone.add(k)
            else:
                state[k] = v
                gone.discard(k)
        assert new_root == (build_host(list(state.items()))[0] if state else BLANK_ROOT)
        root = new_root
        for k, v in state.items():                      # every surviving key reads back
            st, _, value, _, _ = walk_host(db, root, k)
            assert st == 0 and value == rlp_encode([v])
        for k in gone:                                  # every removed key is proven absent
            st, _, value, proof, _ = walk_host(db, root, k)
            assert st == 0 and value == b'' and proof is not None


@pytest.mark.parametrize('name', CASES)
def test_host_twin_matches_reference_and_mirror(name):
    c = sa.case(name)
    _, base, batches = shape('fx/' + name)
    b0, outs, _ = sa.host_run('fx/' + name, base, batches)
    assert b0.root == c.base_root
    db, root = dict(b0.db()), b0.root
    for want, prs, got in zip(c.batches, batches, outs):
        m_root, m_db = apply_encoded_host(db, root, prs)
        assert got.root == want.root == m_root
        assert got.db() == m_db
        assert int(got.off[0]) == 0 and int(got.off[got.n_nodes]) == got.n_bytes == len(got.blob)
        assert set(got.db()) <= want.reachable
        db.update(got.db())
        assert want.reachable <= set(db)
        root = got.root


@pytest.mark.parametrize('name', SHAPES)
def test_shapes_match_mirror_and_rebuild(name):
    _, base, batches = shape(name)
    b0, outs, _ = sa.host_run(name, base, batches)
    db, root, state = dict(b0.db()), b0.root, dict(base)
    for prs, got in zip(batches, outs):
        assert any(not v for _, v in prs)
        m_root, m_db = apply_encoded_host(db, root, prs)
        sa.state_after(state, prs)
        w_root, w_db = build_encoded_host(sorted(state.items()))
        assert got.root == m_root == w_root
        assert got.db() == m_db and set(m_db) <= set(w_db)
        db.update(m_db)
        assert set(w_db) <= set(db)
        root = got.root


def test_chain_fuses_from_the_bottom():
    _, base, batches = shape('chain')
    b0, outs, _ = sa.host_run('chain', base, batches)
    # the deepest branch (depth 62) held two leaves: one is removed, the other hangs, its path one
    # nibble longer, under the branch at depth 61 (embedded there: it stays under 32 bytes); the 62
    # branches at depths 0 .. 61 are re-encoded.  What else is emitted are the opened leaves beside
    # the path, byte for byte what the store holds.
    held = set(b0.db())
    assert len(set(outs[0].db()) - held) == 62
    held |= set(outs[0].db())
    assert len(set(outs[1].db()) - held) == 51          # eleven more levels gone: the branches at 0 .. 50


def test_opened_items_of_the_merged_list():
    """the removal lane's items by kind of the child it opened, at the smallest tries"""
    def items(name):
        c = sa.case(name)
        root, db = build_host(c.base)
        st, _, out = merge_host(db, root, sa.ops(c.batches[0].items))
        assert st == 0
        return out
    (path, kind, payload), = items('collapse_root_hashed_leaf')
    assert (path, kind) == ([2, 2, 3, 4], ITEM_VALUE) and len(payload) == 36
    (path, kind, payload), = items('collapse_root_inline_leaf')
    assert (path, kind, payload) == ([2, 2, 3, 4], ITEM_VALUE, rlp_encode([b'a']))
    (path, kind, payload), = items('collapse_root_extension')
    assert (path, kind) == ([2, 1, 1], ITEM_SUBTREE) and len(payload) == 33         # slot nibble + the extension's path
    (path, kind, payload), = items('collapse_root_hashed_branch')
    assert (path, kind) == ([2], ITEM_SUBTREE) and len(payload) == 33
    (path, kind, payload), = items('collapse_root_inline_branch')
    assert (path, kind) == ([2], ITEM_SUBTREE) and len(payload) < 32 and payload[0] >= 0xc0
    assert items('every_key_removed') == [] and items('only_key_removed') == []
    (path, kind, _), = items('branch_value_child_removed')
    assert (path, kind) == ([6, 11], ITEM_VALUE)                                      # b'k': the branch's value alone
    got = items('survivor_between_removed_keys')
    assert [(p, k) for p, k, _ in got] == [([5, 2, 3, 4], ITEM_VALUE)]


def test_batch_without_removal_equals_update_and_absent_removals_emit_nothing_new():
    prs = sb.mixed_pairs(300, 31)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 64, 164)
    gone = sorted((sb.sha3(b'never set %d' % i)[:i % 33], b'') for i in range(1, 60))
    with sa.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        a = st.apply(b0.root, batch, insert=False)
        u = st.apply(b0.root, batch, insert=False, removals=False)
        assert a.rc == sa.OK and a.same(u) is None and a.n_items == u.n_items
        assert apply_encoded_host(b0.db(), b0.root, batch) == update_encoded_host(b0.db(), b0.root, batch)
        g = st.apply(b0.root, gone)
        assert g.rc == sa.OK and g.root == b0.root and g.n_nodes > 0
        after = st.info()
        assert after['n_unique'] == before['n_unique'] and after['n_nodes'] == before['n_nodes'] + g.n_nodes
        assert set(g.db()) <= set(b0.db())
        # update keeps refusing an empty value
        r = st.apply(b0.root, gone, removals=False)
        assert (r.rc, r.bad_index) == (sa.BAD_VALUE, 0)
    with pytest.raises(ValueError):
        update_host(b0.db(), b0.root, [(b'k1', b'')])
    with pytest.raises(ValueError):
        build_host([(b'k1', b'')])
    with pytest.raises(ValueError):
        apply_host(b0.db(), b0.root, [(b'k1', b'')])    # None removes; an empty value is no value


def test_empty_batch_blank_root_and_compute_only():
    prs = sb.mixed_pairs(100, 41)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 20, 41)
    kept = [p for p in batch if p[1]]
    with sa.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        got = st.apply(b0.root, [])
        assert (got.rc, got.root, got.n_nodes, got.n_bytes) == (sa.OK, b0.root, 0, 0)
        got = st.apply(BLANK_ROOT, batch, insert=False)             # removals of nothing are dropped
        assert got.same(sb.host_build(kept)) is None and got.n_items == 0
        got = st.apply(BLANK_ROOT, [(k, b'') for k, _ in batch], insert=False)
        assert (got.rc, got.root, got.n_nodes, got.n_bytes) == (sa.OK, BLANK_ROOT, 0, 0)
        got = st.apply(b0.root, [(k, b'') for k, _ in prs])          # every key removed: the blank root, no node
        assert (got.rc, got.root, got.n_nodes, got.n_bytes, got.n_items) == (sa.OK, BLANK_ROOT, 0, 0, 0)
        assert st.info() == before
        got = st.apply(b0.root, batch, insert=False)
        assert got.rc == sa.OK and got.n_nodes > 0 and st.info() == before
        again = st.apply(b0.root, batch, insert=True)
        assert again.same(got) is None and st.info()['n_nodes'] == before['n_nodes'] + got.n_nodes
    assert apply_encoded_host({}, b0.root, []) == (b0.root, {})
    assert apply_encoded_host({}, BLANK_ROOT, batch) == build_encoded_host(kept)
    assert apply_encoded_host(b0.db(), b0.root, [(k, b'') for k, _ in prs]) == (BLANK_ROOT, {})


def test_too_small_capacity_reports_sizes_and_inserts_nothing():
    prs = sb.mixed_pairs(100, 42)
    b0 = sb.host_build(prs)
    batch = sa.batch_onto(prs, 30, 42)
    with sa.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        full = st.apply(b0.root, batch, insert=False)
        for kw in ({'blob_cap': full.n_bytes - 1}, {'node_cap': full.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            b = st.apply(b0.root, batch, **kw)
            assert b.rc == sa.TOO_SMALL and (b.n_nodes, b.n_bytes) == (full.n_nodes, full.n_bytes)
            assert b.untouched and b.root == full.root and st.info() == before


def test_refusals_name_the_first_key():
    prs, b0, key, proof = sa.sibling_case()
    db = b0.db()
    batch = sa.batch_onto(prs, 40, 43)
    swapped = list(batch)
    swapped[20], swapped[21] = swapped[21], swapped[20]
    with sa.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        b = st.apply(b0.root, swapped)
        assert (b.rc, b.bad_index, b.n_nodes) == (sa.BAD_ORDER, 21, 0)
        b = st.apply(b0.root, batch[:30] + [batch[29]] + batch[30:])
        assert (b.rc, b.bad_index) == (sa.BAD_ORDER, 30)
        b = st.apply(sb.sha3(b'no such root'), batch)
        assert (b.rc, b.bad_index, b.status, b.n_nodes) == (sa.BAD_WALK, 0, PV_SP_NODE_MISSING, 0)
        assert st.info() == before
    # a store that holds the removed key's proof nodes only: the set of the key is applied, its
    # removal is refused for the sibling the lane has to open
    part = {sb.sha3(n): n for n in proof}
    two = sorted([(key, b''), (b'\x00 a new key below every other', sb._encode(b'v'))])
    at = two.index((key, b''))
    with pytest.raises(KeyError, match='key {}:'.format(at)):
        apply_encoded_host(part, b0.root, two)
    assert update_encoded_host(part, b0.root, [(key, sb._encode(b'set instead'))])[0] != b0.root
    with sa.HostStore() as st:
        st.add_nodes(proof)
        before = st.info()
        b = st.apply(b0.root, two, blob_cap=1 << 16, node_cap=256)
        assert (b.rc, b.bad_index, b.status, b.n_nodes, b.n_bytes) == (sa.BAD_WALK, at, PV_SP_NODE_MISSING, 0, 0)
        assert st.info() == before
        assert st.apply(b0.root, [(key, sb._encode(b'set instead'))], insert=False).rc == sa.OK
    # the opened node is no trie node: a branch whose slot 1 refers to a three-item list
    junk = b'\xc3\x01\x02\x03' + b'\x00' * 40
    leaf = rlp_encode([b'\x20', sb._encode(b'x' * 40)])
    root_node = rlp_encode([b'', sb.sha3(junk), sb.sha3(leaf)] + [b''] * 14)
    bad_db = {sb.sha3(n): n for n in (junk, leaf, root_node)}
    with pytest.raises(ValueError, match='key 0:'):
        apply_encoded_host(bad_db, sb.sha3(root_node), [(b'\x20', b'')])
    with sa.HostStore() as st:
        st.add_nodes([junk, leaf, root_node])
        b = st.apply(sb.sha3(root_node), [(b'\x20', b'')])
        assert (b.rc, b.bad_index, b.status) == (sa.BAD_WALK, 0, PV_SP_MALFORMED)
        b = st.apply(sb.sha3(root_node), [(b'\x20', sb._encode(b'y'))], insert=False)
        assert b.rc == sa.OK                             # a set carries the reference unopened


def test_last_of_equal_keys_wins():
    base = [(b'k1', b'first'), (b'k2', b'v' * 40), (b'k3', b'w' * 40)]
    root, db = build_host(base)
    assert apply_host(db, root, [(b'k1', b'second'), (b'k1', None)])[0] == build_host(base[1:])[0]
    assert apply_host(db, root, [(b'k1', None), (b'k1', b'second')])[0] == build_host(base[1:] + [(b'k1', b'second')])[0]
    assert apply_host(db, root, [(k, None) for k, _ in base])[0] == BLANK_ROOT


def test_asan_program(tmp_path):
    """stateapplycheck_asan: every batch of every fixture case and of the other shapes and the
    refusals, each buffer at its exact size"""
    subprocess.run(['make', '-s', '-C', sa.HC_DIR, 'stateapplycheck_asan'], check=True)
    cases = []
    for name, base, batches in sa.all_shapes():
        b0, outs, stores = sa.host_run(name, base, batches)
        root = b0.root
        for prs, want, nodes in zip(batches, outs, stores):
            cases.append((nodes, root, prs, want))
            root = want.root
    prs, b0, key, proof = sa.sibling_case()
    batch = sa.batch_onto(prs, 20, 44)
    swapped = list(batch)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    with sa.HostStore() as st:
        st.add_nodes(b0.nodes())
        for root, bad in ((b0.root, swapped), (sb.sha3(b'?'), batch), (b0.root, []), (BLANK_ROOT, batch),
                          (b0.root, [(k, b'') for k, _ in prs]), (b0.root, batch[:5] + [batch[4]])):
            cases.append((b0.nodes(), root, bad, st.apply(root, bad, insert=False)))
    with sa.HostStore() as st:
        st.add_nodes(proof)                             # the sibling withheld
        cases.append((proof, b0.root, [(key, b'')], st.apply(b0.root, [(key, b'')], insert=False)))
    junk = b'\xc3\x01\x02\x03' + b'\x00' * 40
    leaf = rlp_encode([b'\x20', sb._encode(b'x' * 40)])
    root_node = rlp_encode([b'', sb.sha3(junk), sb.sha3(leaf)] + [b''] * 14)
    with sa.HostStore() as st:
        st.add_nodes([junk, leaf, root_node])
        cases.append(([junk, leaf, root_node], sb.sha3(root_node), [(b'\x20', b'')],
                      st.apply(sb.sha3(root_node), [(b'\x20', b'')], insert=False)))
    for row in th.ROWS:                                 # the hostile-node table
        cases += [(row.nodes, row.root, batch, th.apply_twin(row, batch))
                  for batch in th.UPDATE_BATCHES + th.REMOVAL_BATCHES]
    assert {c[3].rc for c in cases} >= {sa.OK, sa.BAD_ORDER, sa.BAD_WALK}
    assert {c[3].status for c in cases} >= {0, PV_SP_NODE_MISSING, PV_SP_MALFORMED}
    path = os.path.join(str(tmp_path), 'cases.bin')
    sa.write_cases(path, cases)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(sa.HC_DIR, 'stateapplycheck_asan'), path], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors='replace')
    assert r.returncode == 0, out[-4000:]
    assert '{} cases ok'.format(len(cases)) in out
