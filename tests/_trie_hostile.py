"""Hostile trie nodes, one table for the five state walks: hand-encoded root nodes, each walked by
proof verification (sp_verify), proof generation (sg_walk), the update and apply merges (tu_walk_t,
tu_open) and the prune (tp_visit).  The walks share the node parser of csrc/pv_trie_node.h, not a
policy: on the same bytes they answer differently on purpose, and the rows whose `upd` and `prv`
columns differ are the contract a change to the shared parser must keep.

Every store holds the row's node and L = rlp([20 6b 31, 'v' * 40]); the root is the hash of the
row's node.  Statuses are PV_SP_*: 0 OK, 1 VALUE_MISMATCH, 2 NODE_MISSING, 3 MALFORMED."""
import _state_apply as sa
import _state_build as sb
import _state_proofs as sp
import _state_prune as pr
import _state_store as ss
import _state_update as su
from plenum_gpu.state_proofs import _length_prefix, rlp_encode

OK, VALUE_MISMATCH, NODE_MISSING, MALFORMED = range(4)
sha3 = sb.sha3

K, K0, K1, K2, K1X = b'k', b'k0', b'k1', b'k2', b'k1x'
L = rlp_encode([b'\x20\x6b\x31', b'v' * 40])
H = sha3(L)
LEAF = bytes.fromhex('c58320 6b31 76'.replace(' ', ''))


def _list(body):
    return _length_prefix(len(body), 192) + body


def branch(slot6=b'\x80', item16=b'\x80'):
    return _list(b'\x80' * 6 + slot6 + b'\x80' * 9 + item16)


def inline_leaf(n):
    """rlp([3b 31, 'w' * n]): n + 5 bytes; under slot 6 it is the leaf of k1"""
    return rlp_encode([b'\x3b\x31', b'w' * n])


class Row:
    """upd: the status of update and apply for each of UPDATE_BATCHES; prv: the status of prove (and,
    with the proved value expected, of verification) for the keys k1, k, k1x; keeps_l / n_missing:
    what a prune to the row's root does with L and how many references it counts as missing.
    differs: the two columns differ for some key."""

    def __init__(self, name, node, upd, prv, keeps_l=False, n_missing=0):
        self.name, self.node, self.upd = name, bytes(node), upd
        self.prv = (prv,) * 3 if isinstance(prv, int) else tuple(prv)
        self.keeps_l, self.n_missing = keeps_l, n_missing
        self.root = sha3(self.node)
        self.nodes = [self.node, L]

    @property
    def differs(self):
        return any(p != self.upd for p in self.prv)


def _h(s):
    return bytes.fromhex(s.replace(' ', ''))


ROWS = [
    Row('leaf', LEAF, 0, 0),
    Row('leaf_long_header', _h('f8 05 83 20 6b 31 76'), 0, 0),        # lenient: a long form for a short length
    Row('bytes_after_list', LEAF + b'\x00', 3, 3),
    Row('list_overruns_node', _h('c6 83 20 6b 31 76'), 3, 3),
    Row('items3', _h('c3 80 80 80'), 3, 3),
    Row('items16', b'\xd0' + b'\x80' * 16, 3, 3),
    Row('items18', b'\xd2' + b'\x80' * 18, 3, 3),
    Row('empty_list', b'\xc0', 3, 3),
    Row('string_node', b'\x83abc', 3, 3),
    Row('empty_path', _h('c2 80 76'), 3, 3),
    Row('path_is_list', _h('c3 c1 20 76'), 3, 3),
    Row('item_overruns_list', _h('c3 83 20 6b'), 3, 3),
    Row('header_alone', b'\xf8', 3, 3),
    Row('leaf_value_is_list', _h('c6 83 20 6b 31 c1 76'), 3, (3, 0, 0)),
    Row('leaf_empty_value', _h('c5 83 20 6b 31 80'), 3, 0),
    Row('other_leaf_empty_value', _h('c5 83 20 6b 32 80'), 3, 0),
    Row('other_leaf_value_is_list', _h('c6 83 20 6b 32 c1 76'), 3, 0),
    Row('ext_no_nibble', _h('e2 00 a0') + H, 3, 3),
    Row('ext_one_byte_child', _h('c3 16 81 99'), 2, 2),
    Row('ext_over_blank', _h('c2 16 80'), 3, 0),
    Row('branch_value_is_list', branch(item16=b'\xc0'), 3, 0),
    Row('slot_long_form_ref', branch(b'\xb8\x20' + H), 2, 0, keeps_l=True),
    Row('slot_31_byte_string', branch(b'\x9f' + b'\x11' * 31), 2, 2),
    Row('slot_inline_33', branch(inline_leaf(28)), 3, 0),
    Row('slot_inline_32', branch(inline_leaf(27)), 3, 0),
    Row('slot_inline_31', branch(inline_leaf(26)), 0, 0),
    Row('slot_inline_3_items', branch(_h('c3 01 02 03')), 3, 3),
    Row('slot_inline_names_l', branch(_list(b'\xa0' + H + b'\x01\x02')), 3, 3),   # malformed: hides L
    Row('slot_ref', branch(b'\xa0' + H), 0, 0, keeps_l=True),
    Row('slot_ref_missing', branch(b'\xa0' + b'\x22' * 32), 2, 2, n_missing=1),
]
assert len(inline_leaf(27)) == 32 and len({r.name for r in ROWS}) == len(ROWS)

PROVE_KEYS = [K1, K, K1X]
NEW = sb._encode(b'new')
UPDATE_BATCHES = [[(K1, NEW)], [(K0, NEW), (K2, NEW)], [(K, NEW)], [(K1X, NEW)]]
# apply alone: the same keys removed, and a removal beside slot 6, whose lane opens what the slot
# names (tu_open); their statuses are the mirror's
REMOVAL_BATCHES = [[(k, b'') for k, _ in b] for b in UPDATE_BATCHES] + [[(b'\x70', b'')], [(K1, b''), (b'\x70', NEW)]]


# ------------------------------------------------------------------ the host twins and their mirrors
def verify_queries(row, proved):
    """[(q, key q, expected encoded value)]: nothing, 'v', the list c1 76 and what the prove walk found"""
    out = []
    for q, (key, value) in enumerate(zip(PROVE_KEYS, proved)):
        out += [(q, key, v) for v in dict.fromkeys([b'', b'v', b'\xc1\x76', value])]
    return out


def verify_twin(row, key, val):
    return int(sp.host_statuses(sp.Packed.single(row.nodes, row.root, key, val))[0])


def verify_mirror(row, key, val):
    from plenum_gpu.state_proofs import walk_status
    ranges, pos = [], 0
    for n in row.nodes:
        ranges.append((pos, pos + len(n)))
        pos += len(n)
    return walk_status(b''.join(row.nodes), ranges, [sha3(n) for n in row.nodes], row.root, key, val)


def prove_scenario(row):
    return [row.nodes], [row.root], [0] * len(PROVE_KEYS), PROVE_KEYS, None


def prove_twin(row):
    """-> (the twin's ss.Result over PROVE_KEYS, the mirror's)"""
    batches, roots, ridx, keys, max_nodes = prove_scenario(row)
    st = ss.HostStore(1)
    st.add(batches[0])
    return st.prove(roots, ridx, keys), ss.mirror_prove(st.db, st.id_of, roots, ridx, keys)


def merge_mirror(row, batch):
    """-> (status, new root or None)"""
    from plenum_gpu.state_store import build_items_host, merge_host
    from plenum_gpu.state_proofs import BLANK_ROOT
    st, _, items = merge_host({sha3(n): n for n in row.nodes}, row.root, batch)
    if st != OK:
        return st, None
    return st, build_items_host(items)[0] if items else BLANK_ROOT


def update_twin(row, batch):
    """-> the twin's sb.Built (rc, status, root, nodes), nothing inserted"""
    with su.HostStore() as st:
        st.add_nodes(row.nodes)
        return st.update(row.root, batch, insert=False)


def apply_twin(row, batch):
    with sa.HostStore() as st:
        st.add_nodes(row.nodes)
        return st.apply(row.root, batch, insert=False)


def built_status(b):
    """(PV_SP_* status, new root or None) of an update / apply twin's answer"""
    assert b.rc in (su.OK, su.BAD_WALK), b.rc
    return (OK, b.root) if b.rc == su.OK else (b.status, None)


def prune_want(row):
    return pr.Want(row.nodes, [row.root])
