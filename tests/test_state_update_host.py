"""Sets onto a committed root on the CPU: the Python mirror (plenum_gpu.state_store.update_host),
the host build of csrc/pv_trie_update.h + pv_trie_build.h (tools/hostcheck/stateupdatecheck.cpp)
and the fixture recorded from the reference (tests/golden/state_update.json) agree on the root
after every batch and on the nodes; the stand-alone sanitizer program runs the same cases with
exact-size buffers."""
import os
import subprocess

import pytest

import _state_build as sb
import _state_update as su
import _trie_hostile as th
from plenum_gpu.state_proofs import BLANK_ROOT, PV_SP_MALFORMED, PV_SP_NODE_MISSING
from plenum_gpu.state_store import (ITEM_SUBTREE, ITEM_VALUE, build_encoded_host, build_host, merge_host,
                                    update_encoded_host, update_host, walk_host)

CASES = [c.name for c in su.fixture()]
SHAPES = [s[0] for s in su.shapes()]


def shape(name):
    return next(s for s in su.all_shapes() if s[0] == name)


def test_fixture_covers_the_cases_of_the_issue():
    assert len(CASES) == 20 and len(set(CASES)) == 20
    assert su.case('blank_base').base == [] and su.case('blank_base').base_root == BLANK_ROOT
    assert len(su.case('short_root').batches) == 3
    assert [len(b.items) for b in su.case('mixed300').batches] == [60] * 5
    base = dict(su.case('mixed300').base)
    assert sum(k in base for k, _ in su.case('mixed300').batches[0].items) == 30
    c = su.case('reset_same_values')
    assert c.batches[0].root == c.base_root
    assert any(len(v) == 3000 for _, v in su.case('big_value_through_a_split').base)
    for c in su.fixture():
        assert build_host(c.base)[0] == c.base_root


@pytest.mark.parametrize('name', CASES)
def test_mirror_matches_reference(name):
    c = su.case(name)
    root, db = build_host(c.base)
    assert root == c.base_root and set(db) == c.base_reachable
    state = dict(c.base)
    for b in c.batches:
        new_root, emitted = update_host(db, root, b.items)
        assert new_root == b.root
        assert all(sb.sha3(n) == h for h, n in emitted.items())
        assert set(emitted) <= b.reachable              # only nodes of the new trie are emitted
        db.update(emitted)
        assert b.reachable <= set(db)                   # and with them all of it is in the store
        state.update(b.items)
        assert new_root == build_host(list(state.items()))[0]
        root = new_root
    for k, v in state.items():                          # every earlier root stays walkable too
        st, _, value, _, _ = walk_host(db, root, k)
        assert st == 0 and value == sb._encode(v)


@pytest.mark.parametrize('name', CASES)
def test_host_twin_matches_reference_and_mirror(name):
    c = su.case(name)
    _, base, batches = shape('fx/' + name)
    b0, outs, _ = su.host_run('fx/' + name, base, batches)
    assert b0.root == c.base_root
    db, root = dict(b0.db()), b0.root
    for want, prs, got in zip(c.batches, batches, outs):
        m_root, m_db = update_encoded_host(db, root, prs)
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
    b0, outs, _ = su.host_run(name, base, batches)
    db, root, state = dict(b0.db()), b0.root, dict(base)
    for prs, got in zip(batches, outs):
        m_root, m_db = update_encoded_host(db, root, prs)
        state.update(prs)
        w_root, w_db = build_encoded_host(sorted(state.items()))
        assert got.root == m_root == w_root
        assert got.db() == m_db and set(m_db) <= set(w_db)
        db.update(m_db)
        assert set(w_db) <= set(db)
        root = got.root


@pytest.mark.parametrize('name', ['fx/dogs', 'fx/inline_branch', 'fx/run_of_five_at_an_extension', 'fx/full_branch',
                                  'fx/ext7_split_nibble6', 'fx/mixed300', 'wave65', 'chain'])
def test_merged_list_equals_the_mirrors(name):
    """the host twin's merged items, item for item, and the list's properties"""
    _, base, batches = shape(name)
    b0 = sb.host_build(base)
    with su.HostStore() as st:
        st.add_nodes(b0.nodes())
        got = st.merged(b0.root, batches[0])
    status, _, want = merge_host(b0.db(), b0.root, batches[0])
    assert status == 0 and got == want
    paths = [p for p, _, _ in got]
    assert all(a < b for a, b in zip(paths, paths[1:]))
    for i, (p, kind, payload) in enumerate(got):
        assert kind in (ITEM_VALUE, ITEM_SUBTREE) and payload
        if kind == ITEM_SUBTREE:                        # a carried reference is a prefix of nothing
            assert len(payload) == 33 and payload[0] == 0xa0 or (len(payload) < 32 and payload[0] >= 0xc0)
            assert all(q[:len(p)] != p for j, q in enumerate(paths) if j != i)


def test_split_at_the_last_extension_nibble_puts_the_reference_in_the_slot():
    _, base, batches = shape('fx/ext7_split_nibble6')
    b0 = sb.host_build(base)
    _, _, items = merge_host(b0.db(), b0.root, batches[0])
    sub = [it for it in items if it[1] == ITEM_SUBTREE]
    assert len(sub) == 1 and len(sub[0][0]) == 7 and len(items) == 2     # no nibble is left below its slot
    _, _, items = merge_host(b0.db(), b0.root, shape('fx/ext7_split_nibble3')[2][0])
    assert [len(it[0]) for it in items if it[1] == ITEM_SUBTREE] == [7]   # three nibbles left: a new extension


def test_resetting_existing_values_changes_nothing():
    _, base, batches = shape('fx/reset_same_values')
    b0 = sb.host_build(base)
    with su.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        got = st.update(b0.root, batches[0])
        assert got.rc == su.OK and got.root == b0.root and got.n_nodes > 0
        after = st.info()
        assert after['n_unique'] == before['n_unique'] and after['n_nodes'] == before['n_nodes'] + got.n_nodes


def test_empty_batch_blank_root_and_compute_only():
    prs = sb.mixed_pairs(100, 41)
    b0 = sb.host_build(prs)
    with su.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        got = st.update(b0.root, [])
        assert (got.rc, got.root, got.n_nodes, got.n_bytes) == (su.OK, b0.root, 0, 0)
        got = st.update(BLANK_ROOT, prs, insert=False)
        assert got.same(b0) is None and got.n_items == 0         # the plain build; no merge ran
        batch = su._batch_onto(prs, 20, 41)
        got = st.update(b0.root, batch, insert=False)
        assert got.rc == su.OK and got.n_nodes > 0 and st.info() == before
        again = st.update(b0.root, batch, insert=True)
        assert again.same(got) is None and st.info()['n_nodes'] == before['n_nodes'] + got.n_nodes
    assert update_encoded_host({}, b0.root, []) == (b0.root, {})
    assert update_encoded_host({}, BLANK_ROOT, prs) == build_encoded_host(prs)


def test_too_small_capacity_reports_sizes_and_inserts_nothing():
    prs = sb.mixed_pairs(100, 42)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 30, 42)
    with su.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        full = st.update(b0.root, batch, insert=False)
        for kw in ({'blob_cap': full.n_bytes - 1}, {'node_cap': full.n_nodes - 1}, {'blob_cap': 0, 'node_cap': 0}):
            b = st.update(b0.root, batch, **kw)
            assert b.rc == su.TOO_SMALL and (b.n_nodes, b.n_bytes) == (full.n_nodes, full.n_bytes)
            assert b.untouched and b.root == full.root and st.info() == before


def test_refusals_name_the_first_key():
    prs = sb.mixed_pairs(200, 43)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 40, 43)
    db = b0.db()
    swapped = list(batch)
    swapped[20], swapped[21] = swapped[21], swapped[20]
    with su.HostStore() as st:
        st.add_nodes(b0.nodes())
        before = st.info()
        b = st.update(b0.root, swapped)
        assert (b.rc, b.bad_index, b.n_nodes) == (su.BAD_ORDER, 21, 0)
        b = st.update(b0.root, batch[:30] + [batch[29]] + batch[30:])
        assert (b.rc, b.bad_index) == (su.BAD_ORDER, 30)
        b = st.update(b0.root, batch[:5] + [(batch[5][0], b'')] + batch[6:])
        assert (b.rc, b.bad_index) == (su.BAD_VALUE, 5)
        b = st.update(sb.sha3(b'no such root'), batch)             # a root the store does not hold
        assert (b.rc, b.bad_index, b.status, b.n_nodes) == (su.BAD_WALK, 0, PV_SP_NODE_MISSING, 0)
        assert st.info() == before
    with pytest.raises(KeyError, match='key 0:'):
        update_encoded_host(db, sb.sha3(b'no such root'), batch)
    # one inner node withheld: the first batch key whose path crosses it is named
    nodes = walk_host(db, b0.root, batch[7][0])[1]
    assert len(nodes) >= 2
    held = nodes[1]
    first = next(j for j, (k, _) in enumerate(batch) if held in walk_host(db, b0.root, k)[1])
    part = {h: n for h, n in db.items() if n != held}
    with pytest.raises(KeyError, match='key {}:'.format(first)):
        update_encoded_host(part, b0.root, batch)
    with su.HostStore() as st:
        st.add_nodes([n for n in b0.nodes() if n != held])
        before = st.info()
        b = st.update(b0.root, batch)
        assert (b.rc, b.bad_index, b.status, b.n_nodes) == (su.BAD_WALK, first, PV_SP_NODE_MISSING, 0)
        assert st.info() == before
    # a node that is no trie node
    junk = b'\xc3\x01\x02\x03' + b'\x00' * 40
    with su.HostStore() as st:
        st.add_nodes([junk])
        b = st.update(sb.sha3(junk), batch)
        assert (b.rc, b.bad_index, b.status) == (su.BAD_WALK, 0, PV_SP_MALFORMED)
    with pytest.raises(ValueError, match='key 0:'):
        update_encoded_host({sb.sha3(junk): junk}, sb.sha3(junk), batch)


def test_last_of_equal_keys_wins():
    base = [(b'k1', b'first'), (b'k2', b'v' * 40)]
    root, db = build_host(base)
    items = [(b'k1', b'second'), (b'k3', b'x' * 33), (b'k1', b'third')]
    assert update_host(db, root, items)[0] == build_host(base + items)[0]
    assert update_host(db, root, items)[0] != update_host(db, root, items[::-1])[0]
    with pytest.raises(ValueError):
        update_host(db, root, [(b'k1', b'')])


def test_asan_program(tmp_path):
    """stateupdatecheck_asan: every batch of every fixture case and of the other shapes and the
    refusals, each buffer at its exact size"""
    subprocess.run(['make', '-s', '-C', su.HC_DIR, 'stateupdatecheck_asan'], check=True)
    cases = []
    for name, base, batches in su.all_shapes():
        b0, outs, stores = su.host_run(name, base, batches)
        root = b0.root
        for prs, want, nodes in zip(batches, outs, stores):
            cases.append((nodes, root, prs, want))
            root = want.root
    prs = sb.mixed_pairs(60, 44)
    b0 = sb.host_build(prs)
    batch = su._batch_onto(prs, 20, 44)
    swapped = list(batch)
    swapped[3], swapped[4] = swapped[4], swapped[3]
    with su.HostStore() as st:
        st.add_nodes(b0.nodes()[1:])                    # one node withheld
        for root, bad in ((b0.root, swapped), (b0.root, batch), (sb.sha3(b'?'), batch), (b0.root, []),
                          (BLANK_ROOT, batch), (b0.root, batch[:2] + [(batch[2][0], b'')])):
            cases.append((b0.nodes()[1:], root, bad, st.update(root, bad, insert=False)))
    for row in th.ROWS:                                 # the hostile-node table
        cases += [(row.nodes, row.root, batch, th.update_twin(row, batch)) for batch in th.UPDATE_BATCHES]
    assert {c[3].rc for c in cases} >= {su.OK, su.BAD_ORDER, su.BAD_VALUE, su.BAD_WALK}
    path = os.path.join(str(tmp_path), 'cases.bin')
    su.write_cases(path, cases)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(su.HC_DIR, 'stateupdatecheck_asan'), path], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors='replace')
    assert r.returncode == 0, out[-4000:]
    assert '{} cases ok'.format(len(cases)) in out
