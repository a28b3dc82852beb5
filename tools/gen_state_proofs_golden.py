"""Golden state proofs and verifier verdicts of the reference state trie
(state/pruning_state.py PruningState.generate_state_proof /
generate_state_proof_for_keys_with_prefix / verify_state_proof /
verify_state_proof_multi over state/trie/pruning_trie.py).  Test infrastructure
only: it runs where a checkout of the reference is available and writes
tests/golden/state_proofs.json.

    PYTHONHASHSEED=0 REFERENCE_DIR=<reference checkout> python tools/gen_state_proofs_golden.py

(The reference collects proof nodes in a set, so their order follows the hash
seed; with the seed pinned the file is reproduced byte for byte.)

The reference's `state` package needs the `rlp` package; tools/rlp_shim holds a
minimal stand-in, cross-checked below against the reference's own
state.util.fast_rlp._decode_optimized.

Layout of the file: every distinct trie name, kind, root, key, value and node
(its RLP bytes) is stored once and rows hold indices; a row names its proof as a
list of node indices, in order, a node with one flipped bit as [index, bit].  The serialized
proof the reference saw is rlp(list of those nodes) = list header + the nodes'
bytes back to back.  Verdicts are what the reference returned for that
serialized proof (serialized=True).  Where the reference let an exception escape
(deserialize_proof runs outside its try) the row records False and 'raised'.
A row whose serialized proof holds a length that overruns its enclosing item is
marked '/lenient' (strict_ok below): the verdict recorded is still the
reference's, but the project answers False for every such proof by rule.
"""
import base64
import contextlib
import hashlib
import io
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if os.environ.get('PYTHONHASHSEED') != '0':
    sys.exit('run with PYTHONHASHSEED=0: the order of proof nodes follows the hash seed')
if 'REFERENCE_DIR' not in os.environ:
    sys.exit('set REFERENCE_DIR to a checkout of the reference (the directory that holds state/)')
sys.path[:0] = [os.path.join(HERE, 'rlp_shim'), os.path.join(REPO, 'oracle', 'shims'), os.environ['REFERENCE_DIR']]

import rlp  # noqa: E402  (the shim)
from state.pruning_state import PruningState  # noqa: E402
from state.trie.pruning_trie import (BLANK_ROOT, NODE_TYPE_BLANK, NODE_TYPE_BRANCH, NODE_TYPE_LEAF,  # noqa: E402
                                     bin_to_nibbles, key_nibbles_from_key_value_node, starts_with)
from state.util.fast_rlp import _decode_optimized  # noqa: E402
from storage.kv_in_memory import KeyValueStorageInMemory  # noqa: E402

rng = random.Random(20261019)


def check_shim():
    samples = [[b''], [b'a', [b'', b'x' * 60, [b'\x80', b'\x7f']], b'y' * 300], [[b'k' * 33] * 17]]
    for x in samples:
        assert _decode_optimized(rlp.encode(x)) == x
        assert rlp.decode(rlp.encode(x)) == x
        assert rlp.codec.encode_raw(x) == rlp.encode(x)
    assert rlp.sedes.big_endian_int.deserialize(rlp.sedes.big_endian_int.serialize(65537)) == 65537


def list_header(n):
    if n < 56:
        return bytes([192 + n])
    ls = n.to_bytes((n.bit_length() + 7) // 8, 'big')
    return bytes([247 + len(ls)]) + ls


def serialize(nodes):
    body = b''.join(nodes)
    return list_header(len(body)) + body


def split(ser):
    """the nodes' RLP bytes of a serialized proof the reference produced"""
    nodes = [rlp.encode(x) for x in rlp.decode(ser)]
    assert serialize(nodes) == ser
    return nodes


def quiet(fn, *a, **kw):
    """-> (verdict, raised): the reference's print(e) swallowed; an escaping exception is False"""
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            return bool(fn(*a, **kw)), False
        except Exception:   # noqa: BLE001
            return False, True


def strict_ok(ser):
    """False when the reference's own decoder (state/util/fast_rlp.py) does not read `ser`
    back as the bytes it is: it raises, or what it decoded re-encodes to other bytes.  That
    happens when a length overruns its enclosing item or the input: the decoder slices it
    off silently, and the reference re-encodes every node in canonical form before hashing
    it, so it may accept bytes that differ from the ones that were hashed.  Rows with such
    a proof are marked '/lenient'.  (Judged with the reference's decoder, not with a
    strict decoder of this project's own.)"""
    try:
        return rlp.codec.encode_raw(_decode_optimized(ser)) == ser
    except Exception:   # noqa: BLE001
        return False


def absence_kind(trie, node, nibbles):
    """why `nibbles` is absent below `node` ('present' if it is not)"""
    t = trie._get_node_type(node)
    if t == NODE_TYPE_BLANK:
        return 'blank_slot'
    if t == NODE_TYPE_BRANCH:
        if not nibbles:
            return 'present' if node[-1] != b'' else 'branch_no_value'
        return absence_kind(trie, trie._decode_to_node(node[nibbles[0]]), nibbles[1:])
    curr = key_nibbles_from_key_value_node(node)
    if t == NODE_TYPE_LEAF:
        if nibbles == curr:
            return 'present'
        return 'longer_than_leaf' if starts_with(nibbles, curr) and curr else 'leaf_mismatch'
    if starts_with(nibbles, curr):
        return absence_kind(trie, trie._get_inner_node_from_extension(node), nibbles[len(curr):])
    return 'ext_mismatch'


def flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


class Out:
    """Tables of distinct tries, kinds, roots, keys, values and nodes; rows hold indices.
    A node with one flipped bit is written in a proof as [node index, bit]."""

    def __init__(self):
        self.tab = {n: ([], {}) for n in ('tries', 'kinds', 'roots', 'keys', 'values', 'nodes')}
        self.flips, self.where = {}, {}
        self.rows, self.multi = [], []

    def idx(self, table, x):
        lst, pos = self.tab[table]
        if x not in pos:
            pos[x] = len(lst)
            lst.append(x)
        return pos[x]

    def flipped(self, node, bit):
        b = flip(node, bit)
        self.flips[b] = [self.idx('nodes', node), bit]
        return b

    def proof(self, nodes):
        return [self.flips[n] if n in self.flips else self.idx('nodes', n) for n in nodes]

    def kv(self, k, v, nodes=()):
        """a value of 8 bytes or more that lies in one of the row's own nodes (a leaf holds
        its value) is stored as [node index, offset, length] instead of its bytes"""
        if v is not None and v not in self.tab['values'][1]:
            at = [(n, n.find(v)) for n in nodes if n not in self.flips and len(v) >= 8 and v in n]
            self.where[v] = [self.idx('nodes', at[0][0]), at[0][1], len(v)] if at else None
        return [self.idx('keys', k), -1 if v is None else self.idx('values', v)]

    def values(self):
        return [self.where[v] or base64.b64encode(v).decode() for v in self.tab['values'][0]]

    def head(self, trie, kind, root, ser, raised):
        kind += ('' if strict_ok(ser) else '/lenient') + ('/raised' if raised else '')
        return [self.idx('tries', trie), self.idx('kinds', kind), self.idx('roots', root)]

    def row(self, trie, kind, root, key, value, nodes):
        ser = serialize(nodes)
        ok, raised = quiet(PruningState.verify_state_proof, root, key, value, ser, serialized=True)
        self.rows.append(self.head(trie, kind, root, ser, raised) + self.kv(key, value, nodes) + [self.proof(nodes), int(ok)])
        return ok

    def mrow(self, trie, kind, root, kvs, nodes):
        ser = serialize(nodes)
        ok, raised = quiet(PruningState.verify_state_proof_multi, root, dict(kvs), ser, serialized=True)
        self.multi.append(self.head(trie, kind, root, ser, raised) + [[self.kv(k, v, nodes) for k, v in kvs],
                                                                      self.proof(nodes), int(ok)])
        return ok


def value_offset(node):
    """byte offset of the last byte of the node (inside its value or last child)"""
    return len(node) - 1


def hash_offset(node):
    """byte offset inside a 32-byte child hash of the node, or None"""
    i = node.find(b'\xa0')
    while i >= 0:
        if i + 33 <= len(node):
            return i + 7
        i = node.find(b'\xa0', i + 1)
    return None


def do_trie(out, name, data, mutate_keys, absent_candidates, stranger):
    state = PruningState(KeyValueStorageInMemory())
    for k, v in data.items():
        state.set(k, v)
    root = state.headHash
    trie = state._trie
    proofs = {k: split(state.generate_state_proof(k, serialize=True)) for k in data}
    kinds = set()
    for k, v in data.items():
        assert out.row(name, 'own', root, k, v, proofs[k]), (name, k)
    keys = list(data)
    for k in mutate_keys:
        v, pf = data[k], proofs[k]
        assert not out.row(name, 'wrong_value', root, k, v + b'!', pf)
        assert not out.row(name, 'none_for_present', root, k, None, pf)
        other = keys[(keys.index(k) + 1) % len(keys)]
        out.row(name, 'other_proof', root, k, v, proofs[other])
        out.row(name, 'wrong_root', hashlib.sha3_256(root).digest(), k, v, pf)
        sh = pf[:]
        rng.shuffle(sh)
        assert out.row(name, 'shuffled', root, k, v, sh)
        assert out.row(name, 'reversed', root, k, v, pf[::-1])
        assert out.row(name, 'duplicated', root, k, v, pf + pf[:1] + pf)
        assert out.row(name, 'extra_nodes', root, k, v, stranger[:1] + pf + stranger[1:])
        for j, node in enumerate(pf):
            out.row(name, 'dropped', root, k, v, pf[:j] + pf[j + 1:])
            bits = [0, 8 * value_offset(node) + 1]
            if node.endswith(v):      # the node that holds the value: a bit in its middle
                bits.append(8 * (len(node) - len(v) + len(v) // 2) + 2)
            ho = hash_offset(node)
            if ho is not None:
                bits.append(8 * ho + 3)
            for bit in bits:
                out.row(name, 'flipped', root, k, v, pf[:j] + [out.flipped(node, bit)] + pf[j + 1:])
    per_kind = {}
    for k in absent_candidates:
        if k in data:
            continue
        kind = absence_kind(trie, trie.root_node, bin_to_nibbles(k))
        assert kind != 'present'
        if per_kind.get(kind, 0) >= 4:
            continue
        per_kind[kind] = per_kind.get(kind, 0) + 1
        kinds.add(kind)
        pf = split(state.generate_state_proof(k, serialize=True))
        assert out.row(name, 'absent/' + kind, root, k, None, pf)
        assert not out.row(name, 'absent_with_value/' + kind, root, k, b'ghost', pf)
    return state, root, proofs, kinds


def candidates(keys):
    c = []
    for k in keys:
        for cut in range(len(k)):
            c.append(k[:cut])
        c += [k + b'\x00', k + b'x', k + k[-1:], k[:-1] + bytes([k[-1] ^ 1]), k[:-1] + bytes([k[-1] ^ 0x10]),
              bytes([k[0] ^ 0x40]) + k[1:], k[:1] + bytes([k[1] ^ 1]) + k[2:] if len(k) > 1 else k + b'z']
    rng.shuffle(c)
    seen, o = set(), []
    for k in c:
        if k not in seen:
            seen.add(k)
            o.append(k)
    return o


def main():
    check_shim()
    out = Out()
    stranger_state = PruningState(KeyValueStorageInMemory())
    for i in range(40):
        stranger_state.set(hashlib.sha256(b'stranger%d' % i).digest(), b'value%d' % i)
    stranger = split(stranger_state.generate_state_proof(hashlib.sha256(b'stranger7').digest(), serialize=True))
    assert len(stranger) >= 2

    small = {
        'k1_k4': {b'k1': b'v1', b'k2': b'v2', b'k3': b'v3', b'k4': b'v4'},
        'k35_k70': {b'k1': b'v1', b'k2': b'v2', b'k35': b'v55', b'k70': b'v99'},
        'dog': {b'do': b'verb', b'dog': b'puppy', b'doge': b'coin', b'horse': b'stallion', b'k': b'kay',
                b'k1': b'v1', b'k11': b'v11', b'k2': b'v2'},
    }
    prefix = b'abcdefgh'
    pref = {prefix + str(s).encode(): str(rng.randint(3000, 5000)).encode() for s in [1, 4, 10, 11, 24, 99, 100]}
    pref.update({prefix: b'2122', prefix[:4] + b'zzzz': b'1908', b'zyxwvuts': b'1115', b'rqponmlk': b'0989'})
    small['prefix'] = pref
    kinds = set()
    states = {}
    for name, data in small.items():
        st, root, proofs, kd = do_trie(out, name, data, list(data)[::2][:5], candidates(list(data)), stranger)
        kinds |= kd
        states[name] = (st, root, data)

    big = {}
    def vlen(i):      # 2..250 bytes, most of them short, both ends present
        return 2 if i == 0 else 250 if i == 1 else rng.randint(2, 40) if i % 3 else rng.randint(41, 250)
    for i in range(200):
        big[hashlib.sha256(b'did:%d' % i).digest()] = bytes(rng.getrandbits(8) for _ in range(vlen(i)))
    for i in range(100):
        big[b'attr:%d' % i] = bytes(rng.getrandbits(8) for _ in range(vlen(i)))
    long_keys = []
    for i, n in enumerate([300, 410, 1000, 3000]):
        k = hashlib.sha256(b'long:%d' % i).digest() if i % 2 else b'long:%d' % i
        big[k] = bytes(rng.getrandbits(8) for _ in range(n))
        long_keys.append(k)
    bk = list(big)
    mutate = long_keys + rng.sample(bk, 4)
    st, root, proofs, kd = do_trie(out, 'state', big, mutate, candidates(rng.sample(bk, 40)), stranger)
    kinds |= kd
    want = {'blank_slot', 'leaf_mismatch', 'ext_mismatch', 'branch_no_value', 'longer_than_leaf'}
    assert want <= kinds, want - kinds
    max_nodes = max(len(p) for p in proofs.values())

    # an empty proof, the blank root, no value
    assert out.row('empty', 'blank_root', BLANK_ROOT, b'k1', None, [])
    assert not out.row('empty', 'blank_root_with_value', BLANK_ROOT, b'k1', b'v1', [])

    # verify_state_proof_multi over prefix proofs
    st, root, data = states['prefix']
    ser, vals = st.generate_state_proof_for_keys_with_prefix(prefix, serialize=True, get_value=True)
    nodes = split(ser)
    under = [(k, v) for k, v in data.items() if k.startswith(prefix)]
    assert out.mrow('prefix', 'all_right', root, under, nodes)
    assert out.mrow('prefix', 'subset', root, under[:3], nodes)
    wrong = under[:2] + [(under[2][0], under[2][1] + b'0')] + under[3:]
    assert not out.mrow('prefix', 'one_wrong', root, wrong, nodes)
    assert not out.mrow('prefix', 'one_absent_with_value', root, under + [(prefix + b'5', b'4000')], nodes)
    assert out.mrow('prefix', 'one_absent_none', root, under + [(prefix + b'5', None)], nodes)
    assert out.mrow('prefix', 'shuffled', root, under, nodes[::-1])
    out.mrow('prefix', 'dropped_root', root, under, nodes[:-1])
    out.mrow('prefix', 'wrong_root', hashlib.sha3_256(root).digest(), under, nodes)
    st, root, data = states['dog']
    ser = st.generate_state_proof_for_keys_with_prefix(b'k', serialize=True)
    nodes = split(ser)
    under = [(k, v) for k, v in data.items() if k.startswith(b'k')]
    assert out.mrow('dog', 'all_right', root, under, nodes)
    assert not out.mrow('dog', 'one_wrong', root, under[:-1] + [(under[-1][0], b'nope')], nodes)

    all_nodes = out.tab['nodes'][0]
    max_node = max(len(n) for n in all_nodes)
    doc = {
        'about': 'reference verdicts of PruningState.verify_state_proof[_multi](..., serialized=True); '
                 'tools/gen_state_proofs_golden.py',
        'row': ['trie', 'kind', 'root', 'key', 'value or -1 for None', 'proof', 'verdict'],
        'multi_row': ['trie', 'kind', 'root', '[key, value or -1] pairs', 'proof', 'verdict'],
        'proof': 'node indices in order; [node index, bit] is that node with the bit flipped',
        'values_note': 'base64, or [node index, offset, length]: those bytes of that node',
        'max_nodes_per_proof': max_nodes,
        'largest_node': max_node,
        'tries': out.tab['tries'][0],
        'kinds': out.tab['kinds'][0],
        'roots': [r.hex() for r in out.tab['roots'][0]],
        'keys': [base64.b64encode(k).decode() for k in out.tab['keys'][0]],
        'values': out.values(),
        'nodes': [base64.b64encode(n).decode() for n in all_nodes],
        'rows': out.rows,
        'multi': out.multi,
    }
    path = os.path.join(REPO, 'tests', 'golden', 'state_proofs.json')
    with open(path, 'w') as fh:
        fh.write('{\n' + ',\n'.join(' {}: {}'.format(json.dumps(k), json.dumps(v, separators=(',', ':')))
                                    for k, v in doc.items()) + '\n}\n')
    kname = out.tab['kinds'][0]
    lenient = [r for r in out.rows if '/lenient' in kname[r[1]]]
    print('{} lenient rows, {} of them accepted by the reference'.format(len(lenient), sum(r[-1] for r in lenient)))
    print('{}: {} rows ({} True), {} multi rows, {} nodes, max {} nodes/proof, largest node {} B, {} bytes'
          .format(path, len(out.rows), sum(r[-1] for r in out.rows), len(out.multi), len(all_nodes), max_nodes, max_node,
                  os.path.getsize(path)))
    print('kinds:', ', '.join(sorted(kname)))


if __name__ == '__main__':
    main()
