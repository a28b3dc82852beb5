"""Golden answers of the reference's PruningState (state/pruning_state.py) over scripted write
cycles: set / remove / headHash / commit / revertToHead / get / get_for_root_hash.  Test
infrastructure only: it runs where a checkout of the reference is available and writes
tests/golden/state_cycle.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_state_cycle_golden.py

The reference's `state` package needs the `rlp` package; tools/rlp_shim holds a minimal
stand-in (cross-checked by tools/gen_state_proofs_golden.py).

Each script drives one real PruningState over KeyValueStorageInMemory through its steps, in
order, and every step records what the reference answered:

    {"op": "set", "key", "value"}          PruningState.set
    {"op": "remove", "key"}                PruningState.remove
    {"op": "head"}                         headHash is read (for plenum_gpu this is the flush)
    {"op": "get", "key", "committed"}      -> "value" (hex, or null for None)
    {"op": "get_root", "root", "key"}      get_for_root_hash -> "value"
    {"op": "commit", "form", "root"}       form: none | raw | hex_str | hex_bytes | node (the
                                           decoded node of `root` as rootNode)
    {"op": "revert", "root"}               revertToHead

and, for every step, "head_after" and "committed_after": headHash and committedHeadHash once
the step is done.  A replay compares committedHeadHash after every step and headHash at the
"head" steps only: reading it is free in the reference and a flush in plenum_gpu, and the reads
of staged keys between two "head" steps are the point of the first script.  Inputs, digests
and values only; no node bytes.

Beside recording, the generator checks the reference against a plain dict model of the three
views (uncommitted, committed, per recorded root), so that a quirk of the reference would stop
the generation instead of entering the fixture.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if 'REFERENCE_DIR' not in os.environ:
    sys.exit('set REFERENCE_DIR to a checkout of the reference (the directory that holds state/)')
sys.path[:0] = [os.path.join(HERE, 'rlp_shim'), os.path.join(REPO, 'oracle', 'shims'), os.environ['REFERENCE_DIR']]

from state.pruning_state import PruningState  # noqa: E402
from state.trie.pruning_trie import BLANK_ROOT  # noqa: E402
from storage.kv_in_memory import KeyValueStorageInMemory  # noqa: E402

rng = random.Random(20261021)


def val(n=34):
    return bytes(rng.getrandbits(8) for _ in range(n))


def hx(b):
    return None if b is None else bytes(b).hex()


class Recorder:
    """one PruningState, the dict model beside it, and the recorded steps"""

    def __init__(self, name):
        self.name, self.steps = name, []
        self.state = PruningState(KeyValueStorageInMemory())
        self.now = {}                       # the uncommitted view
        self.at = {bytes(BLANK_ROOT): {}}   # root -> the state it stands for

    def _done(self, step):
        step['head_after'] = hx(self.state.headHash)
        step['committed_after'] = hx(self.state.committedHeadHash)
        self.at.setdefault(bytes(self.state.headHash), dict(self.now))
        assert self.at[bytes(self.state.headHash)] == self.now, (self.name, len(self.steps))
        self.steps.append(step)

    def set(self, key, value):
        self.state.set(key, value)
        self.now[key] = value
        self._done({'op': 'set', 'key': hx(key), 'value': hx(value)})

    def remove(self, key):
        self.state.remove(key)
        self.now.pop(key, None)
        self._done({'op': 'remove', 'key': hx(key)})

    def head(self):
        self._done({'op': 'head'})
        return bytes(self.state.headHash)

    def get(self, key, committed):
        got = self.state.get(key, isCommitted=committed)
        want = (self.at[bytes(self.state.committedHeadHash)] if committed else self.now).get(key)
        assert (None if got is None else bytes(got)) == want, (self.name, len(self.steps), key, committed)
        self._done({'op': 'get', 'key': hx(key), 'committed': committed, 'value': hx(got)})

    def get_both(self, *keys):
        for k in keys:
            self.get(k, False)
            self.get(k, True)

    def get_root(self, root, key):
        got = self.state.get_for_root_hash(root, key)
        assert (None if got is None else bytes(got)) == self.at[root].get(key), (self.name, len(self.steps))
        self._done({'op': 'get_root', 'root': hx(root), 'key': hx(key), 'value': hx(got)})

    def commit(self, form, root=None):
        if form == 'none':
            self.state.commit()
            root = bytes(self.state.headHash)
        elif form == 'raw':
            self.state.commit(rootHash=root)
        elif form == 'hex_str':
            self.state.commit(rootHash=root.hex())
        elif form == 'hex_bytes':
            self.state.commit(rootHash=root.hex().encode())
        elif form == 'node':
            self.state.commit(rootNode=self.state.get_head_by_hash(root))
        else:
            raise ValueError(form)
        assert bytes(self.state.committedHeadHash) == root, (self.name, form)
        self._done({'op': 'commit', 'form': form, 'root': hx(root)})

    def revert(self, root):
        self.state.revertToHead(root)
        self.now = dict(self.at[root])
        assert bytes(self.state.headHash) == root
        self._done({'op': 'revert', 'root': hx(root)})

    def out(self):
        return {'name': self.name, 'steps': self.steps}


def read_own_writes():
    """reads of keys set or removed earlier in the same batch, before any headHash"""
    r = Recorder('read_own_writes')
    a, b, c = b'\x12\x34', b'\x12\x35', b'did:absent'
    r.set(a, val())
    r.set(b, val())
    r.get_both(a, b, c)
    r.remove(a)
    r.get_both(a)
    r.set(a, val(50))                 # set again after the removal: the last occurrence wins
    r.set(b, val(3))
    r.get_both(a, b)
    r.head()
    r.get_both(a, b, c)
    r.commit('none')
    r.remove(b)                       # a staged removal over a committed key
    r.set(c, val())
    r.get_both(a, b, c)
    r.head()
    r.get_both(a, b, c)
    return r.out()


def _batches():
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(12)] + [b'k', b'k1', b'k12', b'attr:7']
    b1 = [(k, val()) for k in keys[:8] + [b'k', b'k1']]
    b2 = [(k, val()) for k in keys[8:12] + [b'k12']] + [(keys[0], val(60)), (b'k', None)]
    b3 = [(keys[1], None), (keys[9], None), (b'attr:7', val(120)), (keys[2], val(1))]
    return keys, b1, b2, b3


def _apply(r, batch):
    for k, v in batch:
        if v is None:
            r.remove(k)
        else:
            r.set(k, v)
    return r.head()


def three_batches_and_reverts():
    """three batches, a commit of the first while two are uncommitted, reads at every root, reverts
    from the third head to the first, to the committed head and to BLANK_ROOT, and the same sets
    again after each revert: the roots repeat"""
    r = Recorder('three_batches_and_reverts')
    keys, b1, b2, b3 = _batches()
    probe = [keys[0], keys[1], keys[2], keys[9], b'k', b'k1', b'k12', b'attr:7', b'nothing']
    h1 = _apply(r, b1)
    h2 = _apply(r, b2)
    h3 = _apply(r, b3)
    assert len({h1, h2, h3}) == 3
    r.commit('raw', h1)               # batch 1 ordered; 2 and 3 still uncommitted, the head stays
    r.get_both(*probe)
    for h in (h1, h2, h3, bytes(BLANK_ROOT)):
        for k in probe:
            r.get_root(h, k)
    r.revert(h1)                      # from the third head to the first
    r.get_both(*probe)
    assert _apply(r, b2) == h2 and _apply(r, b3) == h3
    r.revert(h1)                      # to the committed head
    r.set(keys[5], val())             # staged work is dropped by the next revert
    r.revert(bytes(BLANK_ROOT))
    r.get_both(*probe)
    assert _apply(r, b1) == h1
    r.get_both(*probe)
    r.commit('none')
    return r.out()


def commit_forms():
    """each argument form of commit, a batch before each"""
    r = Recorder('commit_forms')
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(10)]
    for i, form in enumerate(('none', 'raw', 'hex_str', 'hex_bytes', 'node')):
        h = _apply(r, [(keys[2 * i], val()), (keys[2 * i + 1], val())])
        r.get(keys[2 * i], True)
        r.commit(form, None if form == 'none' else h)
        r.get(keys[2 * i], True)
    return r.out()


def committed_read_unaffected():
    """a committed read while uncommitted work overwrites, removes and adds"""
    r = Recorder('committed_read_unaffected')
    a, b, c = b'\xab\xcd\x10', b'\xab\xcd\x20', b'\xab\xce'
    _apply(r, [(a, val()), (b, val())])
    r.commit('none')
    h = _apply(r, [(a, val(40)), (b, None), (c, val())])
    r.get_both(a, b, c)
    r.set(a, val(2))
    r.get_both(a)
    r.commit('hex_str', h)
    r.get_both(a, b, c)
    return r.out()


def remove_every_key():
    r = Recorder('remove_every_key')
    keys = [b'\x11\x11', b'\x11\x12', b'\x11\x21', b'\x12\x11', b'\x2f\xff']
    _apply(r, [(k, val()) for k in keys])
    r.commit('none')
    assert _apply(r, [(k, None) for k in keys]) == bytes(BLANK_ROOT)
    r.get_both(*keys)
    r.commit('none')
    r.get_both(keys[0])
    return r.out()


def main():
    scripts = [read_own_writes(), three_batches_and_reverts(), commit_forms(), committed_read_unaffected(),
               remove_every_key()]
    out = {'generator': 'tools/gen_state_cycle_golden.py', 'blank_root': bytes(BLANK_ROOT).hex(), 'scripts': scripts}
    path = os.path.join(REPO, 'tests', 'golden', 'state_cycle.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, separators=(',', ':'))
        fh.write('\n')
    print(path, os.path.getsize(path), 'bytes;', sum(len(s['steps']) for s in scripts), 'steps')


if __name__ == '__main__':
    main()
