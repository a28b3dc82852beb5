"""Golden state roots and node sets of the reference state trie after successive batches of
sets and removals onto a base state (state/pruning_state.py PruningState.set / remove / headHash
over state/trie/pruning_trie.py Trie.update / Trie.delete).  Test infrastructure only: it runs
where a checkout of the reference is available and writes tests/golden/state_remove.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_state_remove_golden.py

The reference's `state` package needs the `rlp` package; tools/rlp_shim holds a minimal
stand-in (cross-checked by tools/gen_state_proofs_golden.py).

The file has the layout of tests/golden/state_update.json (tools/gen_state_update_golden.py)
with one addition: a value of null in a batch removes its key.  Each batch is applied to the
same PruningState in a shuffled order, one PruningState.set or PruningState.remove per pair, and
records the headHash afterwards and the digests that joined and that left the set of nodes
reachable by hash from it.  Digests and inputs, not node bytes.  After every batch the generator
asserts that every surviving key reads back, that every removed key reads None and that every
node reachable from the new root is in the database.  The values are distinct random bytes, so
that the reference's reference-count pruning never meets two identical subtrees.

The cases are the smallest tries at which each path of the removal rule of
csrc/pv_trie_update.h can go wrong; see cases().
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
dropped = []   # the cases on which the reference itself failed an assertion


def sha3(b):
    return hashlib.sha3_256(b).digest()


def reachable(state, root):
    """digests of the nodes stored under their hash that a walk from `root` reaches; asserts
    that each of them is in the database under its own hash"""
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
    """-> the case, or None (noted in `dropped`) if the reference fails an assertion on it"""
    try:
        return _run(name, base, batches, base_from)
    except (AssertionError, KeyError) as exc:
        dropped.append('{}: {!r}'.format(name, exc))
        return None


def _run(name, base, batches, base_from):
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
        gone = []
        for k, v in order:
            if v is None:
                state.remove(k)
                final.pop(k, None)
                gone.append(k)
            else:
                state.set(k, v)
                final[k] = v
        root = bytes(state.headHash)
        for k, v in final.items():
            assert state.get(k, isCommitted=False) == v
        for k in gone:
            assert state.get(k, isCommitted=False) is None
        now = reachable(state, root)
        assert (root == BLANK_ROOT) == (not final)
        out['batches'].append({'keys': [k.hex() for k, _ in order],
                               'values': [None if v is None else v.hex() for _, v in order],
                               'root': root.hex(), 'added': sorted(d.hex() for d in now - seen),
                               'removed': sorted(d.hex() for d in seen - now)})
        seen = now
    return out


def val(n=34):
    """n distinct random bytes"""
    return bytes(rng.getrandbits(8) for _ in range(n))


def hex_prefix(nibbles, leaf):
    flags = (2 if leaf else 0) + (len(nibbles) & 1)
    nib = ([flags] if len(nibbles) & 1 else [flags, 0]) + list(nibbles)
    return bytes(16 * nib[i] + nib[i + 1] for i in range(0, len(nib), 2))


def leaf_payload(n_nibbles, raw_len):
    """the length of a leaf's list payload: its hex-prefix path item and its value item"""
    enc = rlp.encode([hex_prefix([1] * n_nibbles, True), rlp.encode([b'\xee' * raw_len])])
    full = len(enc)
    for hl in range(1, 10):   # the list header: 1 byte up to 55, else 1 + the length's bytes
        body = full - hl
        if (hl == 1 and body <= 55) or (hl > 1 and body > 55 and (body.bit_length() + 7) // 8 == hl - 1):
            return body
    raise AssertionError


def rm(*keys):
    return [(k, None) for k in keys]


def cases():
    # ---- the collapse of a two-entry branch, by what survives; at the root and under an extension
    gone = b'\x12\x34'
    survivors = {
        'hashed_leaf': [(b'\x22\x34', val())],
        'inline_leaf': [(b'\x22\x34', b'a')],
        'extension': [(b'\x21\x11', val()), (b'\x21\x12', val())],
        'hashed_branch': [(b'\x21\x11', val()), (b'\x22\x11', val())],
        'inline_branch': [(b'\x21', b'a'), (b'\x22', b'b')],
    }
    for kind, rest in survivors.items():
        yield run('collapse_root_' + kind, [(gone, val())] + rest, [rm(gone)])
        pre = b'\xab\xcd'
        under = [(pre + gone, val())] + [(pre + k, v + b'.') for k, v in rest] + [(b'\x77\x77', val())]
        yield run('collapse_under_extension_' + kind, under, [rm(pre + gone)])
    # ---- branch values
    kk = [(b'k', val()), (b'k1', val())]
    yield run('branch_value_child_removed', kk, [rm(b'k1')])
    yield run('branch_value_removed', kk, [rm(b'k')])
    # ---- carrying order
    three = [(b'\x12\x34', val()), (b'\x52\x34', val()), (b'\x92\x34', val())]
    yield run('survivor_below_removed_slot', three[:2], [rm(b'\x52\x34')])
    yield run('survivor_above_removed_slot', three[:2], [rm(b'\x12\x34')])
    yield run('survivor_between_removed_keys', three, [rm(b'\x12\x34', b'\x92\x34')])
    # ---- cascades
    deep = [(k, val()) for k in (b'\x11\x11', b'\x11\x12', b'\x11\x21', b'\x12\x11')]
    yield run('three_level_subtree_removed', deep + [(b'\x2f\xff', val())], [rm(*[k for k, _ in deep])])
    yield run('every_key_removed', deep + [(b'\x2f\xff', val())], [rm(*([k for k, _ in deep] + [b'\x2f\xff']))])
    yield run('only_key_removed', [(b'only', val())], [rm(b'only')])
    # ---- absent removals: the root stays, nothing new
    absent = [(b'\xab\xcd\x10\x01', val()), (b'\xab\xcd\x20\x02', val()), (b'\x11\x22\x33', val())]
    yield run('absent_removals', absent,
              [rm(b'\xab\xc1'),                # diverges inside the extension [b, c, d]
               rm(b'\x11\x23\x33'),            # diverges inside the leaf of 11 22 33
               rm(b'\x11\x22'),                # a proper prefix of that leaf's key
               rm(b'\x11\x22\x33\x44'),        # extends that leaf's key
               rm(b'\xab\xcd'),                # ends at a branch without a value
               rm(b'\xab\xcd\x30'),            # a blank slot
               rm(b'\xab\xc1', b'\x11\x22', b'\xab\xcd', b'\xab\xcd\x30', b'\xff')])
    # ---- the same batch removes and sets
    two = [(b'\x12\x34', val()), (b'\x22\x34', val())]
    yield run('remove_and_set_in_the_same_slot', two, [rm(b'\x12\x34') + [(b'\x15\x55', val())]])
    yield run('remove_key_set_key_with_suffix', [(b'k', val()), (b'zz', val())], [rm(b'k') + [(b'k1', val())]])
    yield run('remove_and_overwrite_only_sibling', two, [rm(b'\x12\x34') + [(b'\x22\x34', val())]])
    # ---- other shapes
    full = [(b'p' + bytes([16 * s]), val()) for s in range(16)]
    yield run('full_branch_loses_14_then_15', full + [(b'q', val())],
              [rm(*[k for k, _ in full[1:15]]), rm(full[15][0])])
    some = [(b'a', val()), (b'b', val())]
    yield run('empty_key_removed_from_a_state_with_it', [(b'', val())] + some, [rm(b'')])
    yield run('empty_key_removed_from_a_state_without_it', some, [rm(b'')])
    yield run('big_leaf_lengthened_by_a_collapse', [(b'big', val(3000)), (b'bih', b'small')], [rm(b'bih')])
    # a survivor leaf with 5 path nibbles under the root branch: as the root leaf it has 6, one path byte
    # more, and its list payload crosses 55 / 56 or 255 / 256 bytes
    for edge, span in ((55, range(20, 60)), (255, range(200, 260))):
        n = next(n for n in span if leaf_payload(5, n) == edge)
        assert leaf_payload(6, n) == edge + 1
        yield run('survivor_leaf_crosses_%d' % edge, [(b'\x12\x34\x56', val(n)), (b'\x22\x34\x56', val())],
                  [rm(b'\x22\x34\x56')])
    # ---- five mixed batches onto 300 keys: about 30 sets, 20 present and 10 absent removals each
    base = build_fixture_case('mixed300')
    keys = [k for k, _ in base]
    batches = []
    for b in range(5):
        batch = {}
        for k in rng.sample(keys, 35):
            batch[k] = None if len(batch) < 20 else val(rng.randint(2, 90))
        keys = [k for k in keys if batch.get(k, b'') is not None]
        for i in range(15):
            k = sha3(b'did:%d:%d' % (b, i)) if i % 3 else b'attr:%d:%d' % (b, i)
            batch[k] = val(rng.randint(2, 90))
            keys.append(k)
        for i in range(10):   # absent: never set, or removed by an earlier batch
            batch[sha3(b'absent:%d:%d' % (b, i)) if i % 2 else b'attr:%d:%d:x' % (b, i)] = None
        batches.append(list(batch.items()))
    yield run('mixed300', base, batches, base_from='mixed300')


def main():
    out = {'source': 'state/pruning_state.py PruningState.set / remove (a null value) + headHash after each batch; '
                     'nodes reachable from the root',
           'cases': [c for c in cases() if c is not None]}
    path = os.path.join(REPO, 'tests', 'golden', 'state_remove.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')
    print('{}: {} cases, {} bytes'.format(path, len(out['cases']), os.path.getsize(path)))
    for d in dropped:
        print('dropped (the reference failed an assertion):', d)


if __name__ == '__main__':
    main()
