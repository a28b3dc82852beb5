"""State-cycle test helpers: the scripts the reference's PruningState answered
(tests/golden/state_cycle.json, tools/gen_state_cycle_golden.py), their replay through a
plenum_gpu.pruning_state.GpuPruningState, and a store made of the Python mirrors
(apply_host / get_host / walk_host / reachable_host) so that the CPU suite drives the very class
the GPU suite drives over the resident store."""
import json
import os

from conftest import GOLDEN

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with open(os.path.join(GOLDEN, 'state_cycle.json')) as fh:
            _fixture = json.load(fh)
    return _fixture


def scripts():
    return {s['name']: s['steps'] for s in fixture()['scripts']}


class MirrorStore:
    """the four methods GpuPruningState needs, over {sha3(node RLP): node RLP}"""

    def __init__(self):
        self.db = {}
        self.applies = self.reads = 0      # calls, for the tests that count them

    def apply_batch(self, root, items):
        from plenum_gpu.state_store import apply_host
        self.applies += 1
        new, nodes = apply_host(self.db, root, items)
        self.db.update(nodes)
        return new

    def get_batch(self, items, decode=True):
        from plenum_gpu.state_proofs import PV_SP_NODE_MISSING, PV_SP_OK
        from plenum_gpu.state_store import get_host
        self.reads += 1
        out = []
        for q, (root, key) in enumerate(items):
            st, found, value = get_host(self.db, root, key, decode)
            if st == PV_SP_NODE_MISSING:
                raise KeyError('item {}: the root or a node on the path is not in the store'.format(q))
            if st != PV_SP_OK:
                raise ValueError('item {}: not well formed'.format(q))
            out.append(value if found else None)
        return out

    def generate_state_proof(self, key, root, serialize=False, get_value=False):
        from plenum_gpu.state_proofs import PV_SP_NODE_MISSING, PV_SP_OK
        from plenum_gpu.state_store import rlp_decode, walk_host
        st, _, value, proof, _ = walk_host(self.db, root, key)
        if st == PV_SP_NODE_MISSING:
            raise KeyError('the root or a node on the path is not in the store')
        if st != PV_SP_OK:
            raise ValueError('not well formed')
        if not serialize:
            proof = rlp_decode(proof)
        return (proof, value or None) if get_value else proof

    def prune(self, keep_roots):
        from plenum_gpu.state_store import reachable_host
        kept, n_missing, statuses, _ = reachable_host(self.db, keep_roots)
        if any(statuses):
            raise KeyError('a root to keep is not in the store')
        self.db = {h: n for h, n in self.db.items() if h in kept}
        return {'n_kept': len(kept), 'n_missing': n_missing, 'root_status': statuses}


def unhex(x):
    return None if x is None else bytes.fromhex(x)


def replay(state, steps):
    """every step through `state`, compared with what the reference answered: each read, headHash
    at the "head" steps and at the end, committedHeadHash after every step -> the number of reads"""
    reads = 0
    for i, s in enumerate(steps):
        op = s['op']
        if op == 'set':
            state.set(unhex(s['key']), unhex(s['value']))
        elif op == 'remove':
            state.remove(unhex(s['key']))
        elif op == 'head':
            assert state.headHash == unhex(s['head_after']), (i, s)
        elif op == 'get':
            assert state.get(unhex(s['key']), isCommitted=s['committed']) == unhex(s['value']), (i, s)
            reads += 1
        elif op == 'get_root':
            assert state.get_for_root_hash(unhex(s['root']), unhex(s['key'])) == unhex(s['value']), (i, s)
            reads += 1
        elif op == 'commit':
            root = unhex(s['root'])
            form = s['form']
            if form == 'none':
                state.commit()
            elif form == 'raw':
                state.commit(rootHash=root)
            elif form == 'hex_str':
                state.commit(rootHash=root.hex())
            elif form == 'hex_bytes':
                state.commit(rootHash=root.hex().encode())
            elif form == 'node':
                state.commit(rootNode=state.get_head_by_hash(root))
            else:
                raise AssertionError(form)
        elif op == 'revert':
            state.revertToHead(unhex(s['root']))
            assert state.headHash == unhex(s['head_after']), (i, s)
        else:
            raise AssertionError(op)
        assert state.committedHeadHash == unhex(s['committed_after']), (i, s)
    assert state.headHash == unhex(steps[-1]['head_after'])
    return reads
