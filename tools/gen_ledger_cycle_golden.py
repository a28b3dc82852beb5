"""Golden stage / commit / discard cycle, hash-store contents and catch-up
verdicts of the reference ledger over the 1,030 leaves of
tests/golden/merkle.json.  Test infrastructure only: it runs where a checkout
of the reference is available and writes tests/golden/ledger_cycle.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_ledger_cycle_golden.py

plenum.common.ledger does not import without rlp, so Ledger itself is not
instantiated.  The generator drives the reference's CompactMerkleTree exactly
as Ledger.appendTxns / commitTxns / discardTxns / treeWithAppliedTxns
(plenum/common/ledger.py:38-143) do: the uncommitted tree is a copy of the
current one plus one `append` per leaf, a commit is one `append` per leaf on
the ledger's own tree, a discard rebuilds the uncommitted tree from the
committed one and the txns that remain.  The catch-up case follows
_process_catchup_txns / _has_valid_catchup_replies
(plenum/server/catchup/catchup_rep_service.py:341-426): one temporary tree
per reply, MerkleVerifier.verify_tree_consistency against the final size and
hash, stop at the first reply that fails.

Staging always takes the next leaves of the fixture, so leaf i of any tree in
the script is leaf i of tests/golden/merkle.json.
"""
import base64
import json
import os
import sys
from copy import copy

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if 'REFERENCE_DIR' not in os.environ:
    sys.exit('set REFERENCE_DIR to a checkout of the reference (the directory that holds ledger/)')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'shims'), os.environ['REFERENCE_DIR']]

from ledger.compact_merkle_tree import CompactMerkleTree  # noqa: E402
from ledger.hash_stores.memory_hash_store import MemoryHashStore  # noqa: E402
from ledger.merkle_verifier import MerkleVerifier  # noqa: E402
from ledger.tree_hasher import TreeHasher  # noqa: E402

# (op, count): sizes cross 1, 2, 3, 4, 8, 16, 32, 33, 64, 256, 257, 512 and 1024 in both directions
SCRIPT = [
    ('stage', 1), ('stage', 1), ('discard', 1), ('commit', 1), ('stage', 2), ('stage', 1), ('discard', 3),
    ('stage', 3), ('commit', 2), ('stage', 4), ('discard', 1), ('stage', 9), ('commit', 13), ('stage', 16),
    ('stage', 1), ('discard', 1), ('stage', 1), ('commit', 17), ('stage', 31), ('discard', 31), ('stage', 31),
    ('commit', 0), ('stage', 0), ('stage', 192), ('stage', 1), ('discard', 1), ('commit', 223), ('stage', 1),
    ('stage', 255), ('discard', 255), ('discard', 1), ('stage', 256), ('commit', 256), ('stage', 512),
    ('discard', 512), ('stage', 512), ('stage', 6), ('discard', 6), ('commit', 500), ('stage', 6), ('discard', 10),
    ('stage', 10), ('commit', 18),
]
CATCHUP_BASE, CATCHUP_ENDS = 100, [410, 720, 1000]


class HashOnlyStore(MemoryHashStore):
    def writeNode(self, node):
        self._nodes.append(node[2])


class RefLedger:
    """the tree handling of plenum/common/ledger.py Ledger, txns = serialized leaves"""

    def __init__(self, hasher):
        self.tree = CompactMerkleTree(hasher=hasher, hashStore=MemoryHashStore())
        self.uncommittedTxns = []
        self.uncommittedTree = None
        self.uncommittedRootHash = None

    @property
    def size(self):
        return self.tree.tree_size

    def treeWithAppliedTxns(self, txns, currentTree=None):
        tempTree = copy(currentTree or self.tree)
        for txn in txns:
            tempTree.append(txn)
        return tempTree

    def appendTxns(self, txns):
        self.uncommittedTree = self.treeWithAppliedTxns(txns, self.uncommittedTree)
        self.uncommittedRootHash = self.uncommittedTree.root_hash
        self.uncommittedTxns.extend(txns)

    def commitTxns(self, count):
        for txn in self.uncommittedTxns[:count]:
            self.tree.append(txn)
        self.uncommittedTxns = self.uncommittedTxns[count:]
        if not self.uncommittedTxns:
            self.uncommittedTree = None
            self.uncommittedRootHash = None

    def discardTxns(self, count):
        if count == 0:
            return
        assert count <= len(self.uncommittedTxns)
        self.uncommittedTxns = self.uncommittedTxns[:-count]
        if not self.uncommittedTxns:
            self.uncommittedTree = None
            self.uncommittedRootHash = None
        else:
            self.uncommittedTree = self.treeWithAppliedTxns(self.uncommittedTxns)
            self.uncommittedRootHash = self.uncommittedTree.root_hash


def flip(h, bit):
    b = bytearray(h)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def main():
    with open(os.path.join(REPO, 'tests', 'golden', 'merkle.json')) as fh:
        leaves = [bytes.fromhex(x) for x in json.load(fh)['leaves']]
    n = len(leaves)
    hasher = TreeHasher()
    table = {}

    def ref(h):
        return table.setdefault(bytes(h), len(table))

    # ---- the cycle
    led = RefLedger(hasher)
    steps, seen = [], set()
    for op, count in SCRIPT:
        total = led.size + len(led.uncommittedTxns)
        if op == 'stage':
            assert count or led.uncommittedTxns, 'an empty batch on a clean ledger is not part of the script'
            led.appendTxns(leaves[total:total + count])
        elif op == 'commit':
            led.commitTxns(count)
        else:
            led.discardTxns(count)
        total = led.size + len(led.uncommittedTxns)
        seen.add(total)
        staged = led.uncommittedTree or led.tree
        assert staged.tree_size == total
        steps.append([op, count, led.size, total, ref(led.tree.root_hash),
                      None if led.uncommittedRootHash is None else ref(led.uncommittedRootHash),
                      [ref(h) for h in staged.hashes]])
    assert len(steps) >= 40 and led.size == n == 1030 and not led.uncommittedTxns
    assert {1, 2, 3, 4, 8, 16, 32, 33, 64, 256, 257, 512, 1024} <= seen
    store = led.tree.hashStore
    assert store.leafCount == n and [hasher.hash_leaf(x) for x in leaves] == store._leafs
    store_nodes = [[s, h, ref(d)] for s, h, d in store._nodes]   # MemoryHashStore keeps writeNode's tuples

    # the hash-only form of the same list (what a persistent store holds)
    only = CompactMerkleTree(hasher=hasher, hashStore=HashOnlyStore())
    for leaf in leaves:
        only.append(leaf)
    assert only.hashStore._nodes == [d for _, _, d in store._nodes]
    assert only.root_hash == led.tree.root_hash

    # ---- catch-up: ledger at 100 leaves, seeder at 1,030
    ver = MerkleVerifier(hasher)
    final_hash = only.merkle_tree_hash(0, n)
    bounds = [CATCHUP_BASE] + CATCHUP_ENDS
    proofs = [only.consistency_proof(e, n) for e in CATCHUP_ENDS]
    assert all(len(p) >= 2 for p in proofs)

    def run(reply_leaves, reply_proofs, fhash):
        """_process_catchup_txns over the replies -> how many were added to the ledger"""
        ledger = CompactMerkleTree(hasher=hasher)
        for leaf in leaves[:CATCHUP_BASE]:
            ledger.append(leaf)
        accepted = 0
        for txns, proof in zip(reply_leaves, reply_proofs):
            temp = copy(ledger)
            for t in txns:
                temp.append(t)
            try:
                ok = ver.verify_tree_consistency(temp.tree_size, n, temp.root_hash, fhash, list(proof))
            except Exception:   # noqa: BLE001  (_has_valid_catchup_replies catches everything)
                ok = False
            if not ok:
                break
            for t in txns:
                ledger.append(t)
            accepted += 1
        return accepted

    good_leaves = [leaves[bounds[i]:bounds[i + 1]] for i in range(3)]
    variants = []
    variants.append({'what': 'all valid', 'accepted': run(good_leaves, proofs, final_hash)})
    at, bad_leaf = 17, leaves[bounds[1] + 17] + b'!'
    alt = [list(x) for x in good_leaves]
    alt[1][at] = bad_leaf
    variants.append({'what': 'one leaf of reply 2 altered', 'leaf': [1, at, bad_leaf.hex()],
                     'accepted': run(alt, proofs, final_hash)})
    bad_node = flip(proofs[2][1], 77)
    altp = [list(p) for p in proofs]
    altp[2][1] = bad_node
    variants.append({'what': 'one proof node of reply 3 altered', 'node': [2, 1, ref(bad_node)],
                     'accepted': run(good_leaves, altp, final_hash)})
    wrong = only.merkle_tree_hash(0, n - 1)
    variants.append({'what': 'wrong final hash', 'final_hash': ref(wrong),
                     'accepted': run(good_leaves, proofs, wrong)})
    assert [v['accepted'] for v in variants] == [3, 1, 2, 0]

    doc = {'source': 'reference CompactMerkleTree / MerkleVerifier driven as plenum/common/ledger.py and '
                     'catchup_rep_service.py drive them, over tests/golden/merkle.json, '
                     'tools/gen_ledger_cycle_golden.py',
           'n_leaves': n,
           'steps_format': '[op, count, committed size, uncommitted size, committed root, uncommittedRootHash, '
                           'hashes of the staged tree]',
           'steps': steps,
           'store_nodes': store_nodes,
           'catchup': {'base': CATCHUP_BASE, 'ends': CATCHUP_ENDS, 'final_size': n, 'final_hash': ref(final_hash),
                       'proofs': [[ref(h) for h in p] for p in proofs], 'variants': variants}}
    doc['nodes'] = [base64.b64encode(h).decode() for h in table]
    out = os.path.join(REPO, 'tests', 'golden', 'ledger_cycle.json')
    with open(out, 'w') as fh:
        fh.write('{' + ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                                  for k, v in doc.items()) + '}\n')
    print('wrote', out, os.path.getsize(out), 'bytes:', len(steps), 'steps,', len(store_nodes), 'store nodes,',
          len(variants), 'catch-up variants,', len(table), 'nodes')


if __name__ == '__main__':
    main()
