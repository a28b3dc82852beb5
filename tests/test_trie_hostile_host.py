"""The hostile-node table (tests/_trie_hostile.py) through the five host twins of the state walks
and their Python mirrors: twin == mirror on every row, and the literal statuses of the table, so
that the rows on which the walks differ on purpose stay different."""
import pytest

import _state_prune as pr
import _trie_hostile as th

ROWS = {r.name: r for r in th.ROWS}
NAMES = list(ROWS)


def test_the_table_holds_the_deliberate_differences():
    differ = [r.name for r in th.ROWS if r.differs]
    assert differ == ['leaf_value_is_list', 'leaf_empty_value', 'other_leaf_empty_value', 'other_leaf_value_is_list',
                      'ext_over_blank', 'branch_value_is_list', 'slot_long_form_ref', 'slot_inline_33', 'slot_inline_32']
    assert len(th.ROWS) >= 28


@pytest.mark.parametrize('name', NAMES)
def test_prove_and_verify(name):
    row = ROWS[name]
    got, want = th.prove_twin(row)
    assert got.rc == 0 and got.same(want) is None, got.same(want)
    assert tuple(got.status.tolist()) == row.prv
    proved = [got.value(q) for q in range(len(th.PROVE_KEYS))]
    for q, key, val in th.verify_queries(row, proved):
        st = th.verify_twin(row, key, val)
        assert st == th.verify_mirror(row, key, val), (key, val)
        # with the proved value expected, verification ends where generation does
        if val == proved[q]:
            assert st == row.prv[q], (key, val)
        elif row.prv[q] == th.OK:
            assert st == th.VALUE_MISMATCH, (key, val)
        else:
            assert st == row.prv[q], (key, val)


def test_verify_literals():
    leaf, lst = ROWS['leaf'], ROWS['leaf_value_is_list']
    assert th.verify_twin(leaf, th.K1, b'v') == th.OK and th.verify_twin(leaf, th.K1, b'') == th.VALUE_MISMATCH
    for key in (th.K, th.K1X):                               # a short and a long key: proven absent
        assert th.verify_twin(leaf, key, b'') == th.OK and th.verify_twin(leaf, key, b'v') == th.VALUE_MISMATCH
    assert th.verify_twin(lst, th.K1, b'\xc1\x76') == th.MALFORMED     # refused before it is compared
    assert th.verify_twin(lst, th.K, b'') == th.OK


@pytest.mark.parametrize('name', NAMES)
def test_update_and_apply(name):
    row = ROWS[name]
    for batch in th.UPDATE_BATCHES:
        want = th.merge_mirror(row, batch)
        assert th.built_status(th.update_twin(row, batch)) == want, batch
        assert th.built_status(th.apply_twin(row, batch)) == want, batch
        assert want[0] == row.upd, batch
    for batch in th.REMOVAL_BATCHES:
        assert th.built_status(th.apply_twin(row, batch)) == th.merge_mirror(row, batch), batch


def test_a_removal_beside_the_slot_opens_what_it_names():
    """key 70 removed: the lane carries slot 6 as an opened item, so apply answers for the child
    where a set carries the reference as it is"""
    rm, st = [(b'\x70', b'')], [(b'\x70', th.NEW)]
    for name, removed, set_ in (('slot_ref', th.OK, th.OK), ('slot_ref_missing', th.NODE_MISSING, th.OK),
                                ('slot_long_form_ref', th.NODE_MISSING, th.NODE_MISSING),
                                ('slot_inline_3_items', th.MALFORMED, th.OK),
                                ('slot_inline_32', th.MALFORMED, th.MALFORMED), ('slot_inline_31', th.OK, th.OK)):
        assert th.built_status(th.apply_twin(ROWS[name], rm))[0] == removed, name
        assert th.built_status(th.apply_twin(ROWS[name], st))[0] == set_, name


@pytest.mark.parametrize('name', NAMES)
def test_prune(name):
    """a node that does not parse keeps its place under the root that names it and has no children"""
    row = ROWS[name]
    want = pr.check_host_equals_want(row.nodes, [row.root])
    assert want.kept == ({row.root, th.H} if row.keeps_l else {row.root})
    assert want.n_missing == row.n_missing and want.root_status == [th.OK]


def test_prune_keeps_a_malformed_node_and_hides_what_it_names():
    row = ROWS['slot_inline_names_l']
    want = pr.check_host_equals_want(row.nodes, [row.root, th.H])      # L is kept when a root names it
    assert want.kept == {row.root, th.H} and want.root_status == [th.OK, th.OK]
    want = pr.check_host_equals_want(row.nodes + [ROWS['items3'].node], [row.root, ROWS['items3'].root])
    assert want.kept == {row.root, ROWS['items3'].root} and want.n_missing == 0
