"""plenum_gpu.pruning_state.GpuPruningState on the CPU: every script the reference's PruningState
answered (tests/golden/state_cycle.json) replayed through the class over a store made of the Python
mirrors (tests/_state_cycle.py: MirrorStore), and the bookkeeping the scripts do not pin: what is
staged and what runs, the chain of uncommitted heads, the refusals."""
import hashlib

import pytest

import _state_cycle as sc
from plenum_gpu.pruning_state import GpuPruningState
from plenum_gpu.state_proofs import BLANK_NODE, BLANK_ROOT, rlp_encode


def fresh():
    store = sc.MirrorStore()
    return GpuPruningState(store), store


def test_the_fixture_holds_every_script_the_class_is_specified_by():
    fx = sc.fixture()
    assert bytes.fromhex(fx['blank_root']) == BLANK_ROOT
    s = sc.scripts()
    assert sorted(s) == ['commit_forms', 'committed_read_unaffected', 'read_own_writes', 'remove_every_key',
                         'three_batches_and_reverts']
    ops = lambda name: [x['op'] for x in s[name]]                                   # noqa: E731
    first_head = ops('read_own_writes').index('head')
    assert 'get' in ops('read_own_writes')[:first_head] and 'remove' in ops('read_own_writes')[:first_head]
    assert sorted({x['form'] for x in s['commit_forms'] if x['op'] == 'commit'}) == \
        ['hex_bytes', 'hex_str', 'node', 'none', 'raw']
    reverts = [x['root'] for x in s['three_batches_and_reverts'] if x['op'] == 'revert']
    assert len(reverts) == 3 and reverts[-1] == fx['blank_root']
    assert s['remove_every_key'][-1]['head_after'] == fx['blank_root']


@pytest.mark.parametrize('name', sorted(sc.scripts()))
def test_script(name):
    state, store = fresh()
    reads = sc.replay(state, sc.scripts()[name])
    assert reads >= 4
    assert not state.closed


def test_writes_are_staged_and_one_apply_runs_per_head():
    state, store = fresh()
    state.set(b'a', b'1')
    state.set(b'b', b'2')
    state.remove(b'a')
    state.set(b'b', b'3')
    assert store.applies == 0 and store.db == {}
    assert state.get(b'a', isCommitted=False) is None and state.get(b'b', isCommitted=False) == b'3'
    assert store.reads == 0                                 # both answered from the pending map
    assert state.get(b'c', isCommitted=False) is None and store.reads == 1
    assert state.get_batch([b'a', b'b', b'c', b'd'], isCommitted=False) == [None, b'3', None, None]
    assert store.reads == 2                                 # the two remaining keys in one call
    h = state.headHash
    assert store.applies == 1 and state.headHash == h and store.applies == 1      # nothing staged: nothing runs
    from plenum_gpu.state_store import build_host
    assert h == build_host([(b'b', b'3')])[0]
    assert state.uncommittedHeads == [h] and state.committedHeadHash == BLANK_ROOT and state.isEmpty
    with pytest.raises(ValueError):
        state.set(b'k', b'')                                # the reference would store rlp([b''])
    assert state.headHash == h


def test_commit_does_not_move_the_head_and_shortens_the_chain():
    state, store = fresh()
    heads = []
    for i in range(3):
        state.set(b'key%d' % i, b'value%d' % i)
        heads.append(state.headHash)
    state.commit(heads[0])
    assert state.headHash == heads[2] and state.committedHeadHash == heads[0]
    assert state.uncommittedHeads == heads[1:] and not state.isEmpty
    assert state.get(b'key2') is None and state.get(b'key2', isCommitted=False) == b'value2'
    state.revertToHead(heads[1])
    assert state.uncommittedHeads == [heads[1]] and state.headHash == heads[1]
    state.revertToHead(state.committedHeadHash)
    assert state.uncommittedHeads == [] and state.headHash == heads[0]


def test_revert_to_an_unknown_root_changes_nothing():
    state, store = fresh()
    state.set(b'a', b'1')
    h = state.headHash
    state.set(b'b', b'2')
    with pytest.raises(KeyError):
        state.revertToHead(b'\x11' * 32)
    assert state.get(b'b', isCommitted=False) == b'2'       # the staged set is still there
    assert state.headHash != h and state.uncommittedHeads[0] == h
    with pytest.raises(KeyError):
        state.get_for_root_hash(b'\x11' * 32, b'a')


def test_heads_are_decoded_root_nodes():
    state, store = fresh()
    assert state.head == BLANK_NODE and state.committedHead == BLANK_NODE
    state.set(b'a' * 32, b'v' * 40)
    node = state.head
    assert hashlib.sha3_256(rlp_encode(node)).digest() == state.headHash
    assert state.committedHead == BLANK_NODE and state.get_head_by_hash(state.headHash) == node
    state.commit(rootNode=node)
    assert state.committedHead == node


def test_proofs_at_the_head_and_the_traversals_that_are_not_offered():
    state, store = fresh()
    state.set(b'a' * 32, b'v' * 40)
    state.set(b'b' * 32, b'w' * 40)
    proof, value = state.generate_state_proof(b'a' * 32, serialize=True, get_value=True)     # root=None: the head
    assert value == rlp_encode([b'v' * 40])
    assert hashlib.sha3_256(rlp_encode(state.generate_state_proof(b'a' * 32)[-1])).digest() == state.headHash
    for call in (lambda: state.as_dict, lambda: state.get_all_leaves_for_root_hash(state.headHash),
                 lambda: state.generate_state_proof_for_keys_with_prefix(b'a')):
        with pytest.raises(NotImplementedError, match='subtree traversal'):
            call()


def test_prune_keeps_the_committed_head_the_chain_and_the_extras():
    state, store = fresh()
    heads = []
    for i in range(4):
        for j in range(6):
            state.set(hashlib.sha256(b'%d:%d' % (i, j)).digest(), b'value %d %d' % (i, j) * 3)
        heads.append(state.headHash)
    state.commit(heads[1])
    state.revertToHead(heads[2])                            # batch 4 is reverted
    before = len(store.db)
    state.prune(extra_roots=[heads[0]])
    assert len(store.db) < before
    for h in heads[:3]:
        assert state.get_for_root_hash(h, hashlib.sha256(b'0:0').digest()) == b'value 0 0' * 3
    with pytest.raises(KeyError):
        state.get_for_root_hash(heads[3], hashlib.sha256(b'3:0').digest())
    state.prune()                                           # ... and without the extra root
    with pytest.raises(KeyError):
        state.get_for_root_hash(heads[0], hashlib.sha256(b'0:0').digest())
    assert state.get(hashlib.sha256(b'1:5').digest()) == b'value 1 5' * 3


def test_close():
    state, store = fresh()
    state.set(b'a', b'1')
    state.close()
    assert state.closed
    with pytest.raises(ValueError):
        state.headHash
