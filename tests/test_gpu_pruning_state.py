"""plenum_gpu.pruning_state.GpuPruningState over the resident store on the GPU: every script the
reference's PruningState answered (tests/golden/state_cycle.json) through pv_state_apply and
pv_state_store_get, the sha256-keyed reads, and prune() after a revert."""
import hashlib

import pytest

import _state_cycle as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cls():
    import torch
    from plenum_gpu import _native
    from plenum_gpu.pruning_state import GpuPruningState
    assert torch.cuda.is_available()
    _native.ensure_init()
    return GpuPruningState


@pytest.mark.parametrize('name', sorted(sc.scripts()))
def test_script(cls, name):
    state = cls()
    try:
        assert sc.replay(state, sc.scripts()[name]) >= 4
    finally:
        state.close()
    assert state.closed


def test_the_gpu_and_the_mirror_store_walk_the_same_roots(cls):
    """the same writes through the resident store and through the mirrors: equal heads, equal reads"""
    gpu, host = cls(), cls(sc.MirrorStore())
    try:
        for i in range(3):
            for s in (gpu, host):
                for j in range(20):
                    s.set(hashlib.sha256(b'%d:%d' % (i, j)).digest(), b'v%d.%d' % (i, j) * (1 + j))
                if i:
                    s.remove(hashlib.sha256(b'%d:%d' % (i - 1, 3)).digest())
            assert gpu.headHash == host.headHash
        keys = [hashlib.sha256(b'%d:%d' % (i, j)).digest() for i in range(4) for j in range(20)]
        gpu.commit(gpu.uncommittedHeads[0])
        host.commit(host.uncommittedHeads[0])
        for committed in (True, False):
            assert gpu.get_batch(keys, isCommitted=committed) == host.get_batch(keys, isCommitted=committed)
        assert gpu.head == host.head and gpu.committedHead == host.committedHead
    finally:
        gpu.close()


def test_get_batch_sha256_equals_get_batch_of_the_hashed_keys(cls):
    state = cls()
    try:
        pre = [b'did:sov:%d' % i for i in range(70)]
        keys = [hashlib.sha256(p).digest() for p in pre]
        for i, k in enumerate(keys[:50]):
            state.set(k, b'verkey %d' % i * (1 + i % 9))
        state.commit()
        want = state.get_batch(keys)
        assert state.get_batch_sha256(pre) == want and want[49] is not None and want[50] is None
        state.remove(keys[3])                      # staged: matched on the host, the rest on the device
        state.set(keys[60], b'staged')
        assert state.get_batch_sha256(pre, isCommitted=False) == state.get_batch(keys, isCommitted=False)
        assert state.get_batch_sha256(pre, isCommitted=False)[3] is None
        assert state.get_batch_sha256(pre, isCommitted=False)[60] == b'staged'
        assert state.get_batch_sha256(pre) == want                 # the committed view is unaffected
        state.headHash
        assert state.get_batch_sha256(pre, isCommitted=False) == state.get_batch(keys, isCommitted=False)
        assert state.get_batch_sha256([]) == []
    finally:
        state.close()


def test_prune_after_a_revert_drops_the_reverted_batch(cls):
    from plenum_gpu.state_store import GpuStateStore
    with GpuStateStore() as store:
        state = cls(store)
        key = lambda i, j: hashlib.sha256(b'%d:%d' % (i, j)).digest()            # noqa: E731
        heads = []
        for i in range(3):
            for j in range(40):
                state.set(key(i, j), b'value %d %d' % (i, j) * 3)
            heads.append(state.headHash)
        state.commit(heads[0])
        state.revertToHead(heads[1])               # batch 3 is reverted
        before = store.info()
        state.prune()
        after = store.info()
        assert after['n_nodes'] < before['n_nodes'] and after['n_bytes'] < before['n_bytes']
        assert state.get(key(0, 7)) == b'value 0 7' * 3                           # the committed root
        assert state.get(key(1, 7)) is None and state.get(key(1, 7), isCommitted=False) == b'value 1 7' * 3
        with pytest.raises(KeyError):
            state.get_for_root_hash(heads[2], key(2, 0))
        for root in heads[:2]:                     # committed and chain roots still prove
            proof, value = state.generate_state_proof(key(0, 7), root, serialize=True, get_value=True)
            assert cls.verify_state_proof(root, key(0, 7), b'value 0 7' * 3, proof, serialized=True) is True
        for j in range(40):                        # the same batch again: the root repeats
            state.set(key(2, j), b'value %d %d' % (2, j) * 3)
        assert state.headHash == heads[2]
        state.close()
        assert store.info()['n_nodes'] > 0         # a store handed in is not closed with the state
