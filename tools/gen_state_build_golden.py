"""Golden state roots and node sets of the reference state trie
(state/pruning_state.py PruningState.set / headHash over state/trie/pruning_trie.py
Trie.update).  Test infrastructure only: it runs where a checkout of the reference
is available and writes tests/golden/state_build.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_state_build_golden.py

The reference's `state` package needs the `rlp` package; tools/rlp_shim holds a
minimal stand-in (cross-checked by tools/gen_state_proofs_golden.py).

Per case the file holds the keys and the raw values in the order they are given to
a build (hex; a key may occur more than once, the last value wins), the reference's
headHash after PruningState.set of every pair -- in a shuffled order, except where
the case is about the order -- and the sorted SHA3-256 digests of the nodes that
are reachable by hash from that root, found by walking the reference's database
from the root.  The reference's database also holds the intermediate nodes of every
update; they are not reachable from the final root and are not recorded.  Digests,
not node bytes, keep the file small.  `empty_key` records whether the reference
accepted the key b''.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if 'REFERENCE_DIR' not in os.environ:
    sys.exit('set REFERENCE_DIR to a checkout of the reference (the directory that holds state/)')
sys.path[:0] = [os.path.join(HERE, 'rlp_shim'), os.path.join(REPO, 'oracle', 'shims'), os.environ['REFERENCE_DIR']]

import rlp  # noqa: E402  (the shim)
from state.pruning_state import PruningState  # noqa: E402
from state.trie.pruning_trie import BLANK_ROOT  # noqa: E402
from storage.kv_in_memory import KeyValueStorageInMemory  # noqa: E402

rng = random.Random(20261020)


def sha3(b):
    return hashlib.sha3_256(b).digest()


def reachable(state, root):
    """sorted digests of the nodes stored under their hash that a walk from `root` reaches"""
    if root == BLANK_ROOT:
        return []
    db = state._trie._db
    out = set()

    def visit_ref(item):
        if isinstance(item, list):
            visit(item)                      # an embedded node
        elif len(item) == 32:
            fetch(bytes(item))
        else:
            assert item == b''

    def visit(node):
        if len(node) == 17:
            for child in node[:16]:
                visit_ref(child)
        else:
            assert len(node) == 2
            if not (node[0][0] >> 4) & 2:    # an extension
                visit_ref(node[1])

    def fetch(h):
        enc = bytes(db.get(h))
        assert sha3(enc) == h
        out.add(h)
        visit(rlp.decode(enc))

    fetch(root)
    return sorted(out)


def run(name, pairs, shuffle=True):
    order = list(pairs)
    if shuffle:
        rng.shuffle(order)
    state = PruningState(KeyValueStorageInMemory())
    for k, v in order:
        state.set(k, v)
    root = bytes(state.headHash)
    final = dict(order)
    for k, v in final.items():
        assert state.get(k, isCommitted=False) == v
    return {'name': name, 'keys': [k.hex() for k, _ in order], 'values': [v.hex() for _, v in order],
            'root': root.hex(), 'digests': [d.hex() for d in reachable(state, root)]}


def mixed(n):
    out = {}
    for i in range(n):
        key = sha3(b'did:%d' % i) if i % 3 else b'attr:%d' % i
        out[key] = bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 250)))
    return list(out.items())


def cases():
    yield run('empty', [])
    yield run('short_root', [(b'k', b'v')])
    for n, vlen in ((31, 24), (32, 25), (33, 26)):
        c = run('leaf%d' % n, [(b'k', b'\x5a' * vlen)])
        assert len(c['digests']) == 1
        yield c
    yield run('children_31_32_33', [(b'a1', b'\x5a' * 24), (b'b1', b'\x5b' * 25), (b'c1', b'\x5c' * 26)])
    yield run('diverge_first_nibble', [(b'\x10abc', b'one value of some length......'), (b'\x20abc', b'another')])
    yield run('diverge_last_nibble', [(b'abc\x10', b'one value of some length......'), (b'abc\x11', b'another')])
    yield run('prefix', [(b'ab', b'the shorter key, a branch value'), (b'abc', b'the longer key')])
    yield run('dogs', [(k, b'value of ' + k * 5) for k in (b'do', b'dog', b'doge', b'horse', b'k', b'k1', b'k11', b'k2')])
    yield run('full_branch', [(b'p' + bytes([16 * s]), b'slot %d ' % s * 4) for s in range(16)] + [(b'p', b'prefix')])
    yield run('inline_branch', [(b'\x12\x30', b'a'), (b'\x12\x31', b'b')])
    yield run('identical_leaves', [(b'\x1a\xbc\xde', b'x' * 30), (b'\x2a\xbc\xde', b'x' * 30)])
    yield run('big_value', [(b'big', bytes(rng.getrandbits(8) for _ in range(3000))), (b'bit', b'small')])
    yield run('overwritten', [(b'k1', b'first'), (b'k2', b'v' * 40), (b'k1', b'second, longer than the first one'),
                              (b'k3', b'x'), (b'k2', b'w'), (b'k1', b'third')], shuffle=False)
    try:
        c = run('empty_key', [(b'', b'the value under the empty key'), (b'a', b'aa'), (b'b', b'bb' * 20)])
        c['empty_key'] = 'accepted'
    except Exception as exc:   # recorded: the entry points then refuse a zero-length key
        c = {'name': 'empty_key', 'empty_key': 'rejected: ' + type(exc).__name__}
    yield c
    yield run('empty_key_alone', [(b'', b'v')]) if c['empty_key'] == 'accepted' else {'name': 'empty_key_alone',
                                                                                      'empty_key': c['empty_key']}
    yield run('mixed300', mixed(300))


def main():
    out = {'source': 'state/pruning_state.py PruningState.set + headHash; nodes reachable from the root',
           'cases': list(cases())}
    path = os.path.join(REPO, 'tests', 'golden', 'state_build.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')
    print('{}: {} cases, {} bytes'.format(path, len(out['cases']), os.path.getsize(path)))


if __name__ == '__main__':
    main()
