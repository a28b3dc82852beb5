"""Golden state roots and node sets of the reference state trie after successive batches of
sets onto a base state (state/pruning_state.py PruningState.set / headHash over
state/trie/pruning_trie.py Trie.update).  Test infrastructure only: it runs where a checkout
of the reference is available and writes tests/golden/state_update.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_state_update_golden.py

The reference's `state` package needs the `rlp` package; tools/rlp_shim holds a minimal
stand-in (cross-checked by tools/gen_state_proofs_golden.py).

Per case the file holds a base state (keys and raw values, hex; or `base_from`, the name of a
case of tests/golden/state_build.json whose pairs are the base), the reference's headHash of
the base, and a list of batches.  Each batch is set into the same PruningState in a shuffled
order, one PruningState.set per pair, and records the headHash afterwards and the SHA3-256
digests of the nodes reachable by hash from it -- as the digests that joined and the digests
that left the reachable set since the step before (the base's set is recorded whole), which
keeps the file small.  Digests, not node bytes.
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

rng = random.Random(20261021)


def sha3(b):
    return hashlib.sha3_256(b).digest()


def reachable(state, root):
    """digests of the nodes stored under their hash that a walk from `root` reaches"""
    if root == BLANK_ROOT:
        return set()
    db = state._trie._db
    out = set()

    def visit_ref(item):
        if isinstance(item, list):
            visit(item)
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
            if not (node[0][0] >> 4) & 2:
                visit_ref(node[1])

    def fetch(h):
        enc = bytes(db.get(h))
        assert sha3(enc) == h
        out.add(h)
        visit(rlp.decode(enc))

    fetch(root)
    return out


def build_fixture_case(name):
    with open(os.path.join(REPO, 'tests', 'golden', 'state_build.json')) as fh:
        for c in json.load(fh)['cases']:
            if c['name'] == name:
                return [(bytes.fromhex(k), bytes.fromhex(v)) for k, v in zip(c['keys'], c['values'])]
    raise KeyError(name)


def run(name, base, batches, base_from=None):
    state = PruningState(KeyValueStorageInMemory())
    final = {}
    for k, v in base:
        state.set(k, v)
        final[k] = v
    root = bytes(state.headHash)
    seen = reachable(state, root)
    out = {'name': name, 'base_root': root.hex(), 'base_digests': sorted(d.hex() for d in seen), 'batches': []}
    if base_from:
        out['base_from'] = base_from
    else:
        out['base_keys'] = [k.hex() for k, _ in base]
        out['base_values'] = [v.hex() for _, v in base]
    for batch in batches:
        order = list(batch)
        rng.shuffle(order)
        assert len(dict(order)) == len(order)
        for k, v in order:
            state.set(k, v)
            final[k] = v
        root = bytes(state.headHash)
        for k, v in final.items():
            assert state.get(k, isCommitted=False) == v
        now = reachable(state, root)
        out['batches'].append({'keys': [k.hex() for k, _ in order], 'values': [v.hex() for _, v in order],
                               'root': root.hex(), 'added': sorted(d.hex() for d in now - seen),
                               'removed': sorted(d.hex() for d in seen - now)})
        seen = now
    return out


def val(tag, n=34):
    return (tag * n)[:n]


def cases():
    dogs = [(k, b'value of ' + k * 5) for k in (b'do', b'dog', b'doge', b'horse', b'k', b'k1', b'k11', b'k2')]
    yield run('blank_base', [], [dogs[:3], [(b'dot', val(b'dot ')), (b'do', b'again')]])
    yield run('short_root', [(b'k', b'v')],
              [[(b'k', b'w')], [(b'j', b'last nibble')], [(b'\x1b', val(b'first nibble '))]])
    yield run('new_key_is_prefix_of_leaf', [(b'abc', val(b'longer '))], [[(b'ab', val(b'shorter '))]])
    yield run('leaf_is_prefix_of_new_key', [(b'ab', val(b'shorter '))], [[(b'abc', val(b'longer '))]])
    ext7 = [(b'\x12\x34\x56\x70', val(b'seven-zero ')), (b'\x12\x34\x56\x71', val(b'seven-one '))]
    yield run('ext7_split_nibble0', ext7, [[(b'\x22\x34\x56\x70', val(b'zero '))]])
    yield run('ext7_split_nibble3', ext7, [[(b'\x12\x35\x56\x70', val(b'three '))]])
    yield run('ext7_split_nibble6', ext7, [[(b'\x12\x34\x56\x80', val(b'six '))]])
    yield run('ext7_key_is_even_prefix', ext7, [[(b'\x12\x34', val(b'prefix '))]])
    yield run('inline_branch', [(b'\x12\x30', b'a'), (b'\x12\x31', b'b')],
              [[(b'\x10\x00', val(b'above '))], [(b'\x12\x32', b'c')]])
    yield run('dogs', dogs, [[(k, b'set ' + k * 9) for k in (b'do', b'd', b'dogs', b'k1', b'k12')]])
    full = [(b'p' + bytes([16 * s]), b'slot %d ' % s * 4) for s in range(16)] + [(b'p', b'prefix')]
    yield run('full_branch', full, [[(b'p\x00', val(b'new 0 ')), (b'p\xf0', val(b'new 15 ')), (b'p', b'new prefix')]])
    leaf = [(b'\x50\x50', val(b'the old leaf '))]
    lo = [(b'\x50' + bytes([x]), val(b'below %d ' % x)) for x in (0x10, 0x30, 0x4f)]
    hi = [(b'\x50' + bytes([x]), val(b'above %d ' % x)) for x in (0x51, 0x70, 0x90)]
    yield run('leaf_between_batch_keys', leaf, [lo[:2] + hi[1:]])
    yield run('leaf_above_batch_keys', leaf, [lo])
    yield run('leaf_below_batch_keys', leaf, [hi])
    ext = [(b'\xab\xcd\xe0\x01', val(b'one ')), (b'\xab\xcd\xe0\x02', val(b'two ')), (b'\x11', b'other')]
    yield run('run_of_five_at_an_extension', ext,
              [[(b'\xab\x1d\xe0\x01', val(b'leaves at 2, before ')), (b'\xab\xcd\x10\x01', val(b'leaves at 4, before ')),
                (b'\xab\xcd\xe0\x01', val(b'through, overwrites ')), (b'\xab\xcd\xe0\x03', val(b'through, new ')),
                (b'\xab\xcd\xe5\x01', val(b'leaves at 5, after '))]])
    small = [(sha3(b'acct:%d' % i)[:6], val(b'balance %d ' % i, 20 + i)) for i in range(24)]
    yield run('reset_same_values', small, [[small[i] for i in (1, 5, 8, 13, 21)]])
    yield run('empty_key_into_a_state_without_it', [(b'a', b'aa'), (b'b', b'bb' * 20)],
              [[(b'', b'the value under the empty key')]])
    yield run('empty_key_into_a_state_with_it', [(b'', b'the value under the empty key'), (b'a', b'aa'), (b'b', b'bb' * 20)],
              [[(b'', b'another value under the empty key'), (b'a', b'aaa')]])
    big = bytes(rng.getrandbits(8) for _ in range(3000))
    yield run('big_value_through_a_split', [(b'big', big)], [[(b'bih', b'small')], [(b'b', val(b'above '))]])
    base = build_fixture_case('mixed300')
    keys = [k for k, _ in base]
    batches = []
    for b in range(5):
        batch = {}
        for k in rng.sample(keys, 30):
            batch[k] = bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 90)))
        for i in range(30):
            k = sha3(b'did:%d:%d' % (b, i)) if i % 3 else b'attr:%d:%d' % (b, i)
            batch[k] = bytes(rng.getrandbits(8) for _ in range(rng.randint(2, 90)))
            keys.append(k)
        batches.append(list(batch.items()))
    yield run('mixed300', base, batches, base_from='mixed300')


def main():
    out = {'source': 'state/pruning_state.py PruningState.set + headHash after each batch; nodes reachable from the root',
           'cases': list(cases())}
    path = os.path.join(REPO, 'tests', 'golden', 'state_update.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')
    print('{}: {} cases, {} bytes'.format(path, len(out['cases']), os.path.getsize(path)))


if __name__ == '__main__':
    main()
