"""The ledger's write cycle on the device-resident Merkle tree.

`GpuLedgerTree` is a `GpuMerkleTree` that can be a ledger's only tree: it takes
over what plenum/common/ledger.py keeps a host `CompactMerkleTree` (and copies
of it) for.

* The uncommitted cycle of a 3PC batch: `appendTxns` stages leaves and yields
  `uncommittedRootHash` (the txn root of the PRE-PREPARE), `commitTxns` makes a
  prefix permanent, `discardTxns` / `reset_uncommitted` take a reverted batch
  back (plenum/common/ledger.py:38-148).  Leaves are the bytes
  `Ledger.serialize_for_tree` produces; a revert is one kernel launch.
* The hash store: with `hash_store=` every committed leaf hash and completed
  node goes to `writeLeaf` / `writeNode` in `CompactMerkleTree._push_subtree`'s
  order (ledger/compact_merkle_tree.py:95-136); `recover` restarts from a
  store (`Ledger.recoverTreeFromHashStore`, ledger/ledger.py) and, unlike
  `CompactMerkleTree.verify_consistency`, checks every stored node.
* The frontier: `hashes` / `frontier(size)` is `CompactMerkleTree.hashes`.
* Catch-up: `accept_catchup_replies` does what
  plenum/server/catchup/catchup_rep_service.py:341-426 does with one temporary
  tree per reply, in one stage, one root read and one batched proof check.

The inherited reads (`root_hash`, proofs, `merkle_tree_hash`, `audit_proofs`,
`tree_size`, `len`) keep covering all leaves, staged ones included; pass a
size up to `size` for the committed view.  Everything here needs the GPU.
"""
import ctypes
import hashlib

import numpy as np

from . import _native as nat
from .exceptions import ConsistencyVerificationFailed, LogicError
from .merkle_proofs import GpuMerkleTree, GpuMerkleVerifier, _digests, _p

_EMPTY_ROOT = hashlib.sha256(b'').digest()
_U64_MAX = (1 << 64) - 1


def _hash_of(node):
    """MemoryHashStore keeps the (start, height, hash) tuple writeNode gets; file and
    key-value stores keep the hash"""
    return bytes(node[2]) if isinstance(node, tuple) else bytes(node)


class GpuLedgerTree(GpuMerkleTree):

    def __init__(self, hasher=None, capacity_hint=1024, device=0, hash_store=None):
        super().__init__(hasher=hasher, capacity_hint=capacity_hint, device=device)
        self._committed = 0
        self.hashStore = hash_store
        self.uncommittedRootHash = None

    # ------------------------------------------------------------ C ABI forms
    def sizes(self):
        """(committed, total) as the library holds them"""
        c, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
        nat._check('pv_merkle_tree_sizes', nat.load().pv_merkle_tree_sizes(self._h(), ctypes.byref(c),
                                                                           ctypes.byref(t)))
        return c.value, t.value

    def stage(self, leaves):
        """append staged leaves (bytes each, hashed on the GPU) -> MTH(0, n)"""
        leaves = [bytes(x) for x in leaves]
        if not leaves:
            return self.root_hash
        root = np.zeros(32, np.uint8)
        blob, off = nat.pack_messages(leaves)
        blob, off = np.ascontiguousarray(blob, np.uint8), np.ascontiguousarray(off, np.uint64)
        nat._check('pv_merkle_tree_stage', nat.load().pv_merkle_tree_stage(self._h(), _p(blob), _p(off), len(leaves),
                                                                           _p(root)))
        self._n += len(leaves)
        return root.tobytes()

    def stage_hashes(self, leaf_hashes):
        """append staged leaf hashes ((k, 32) uint8 or 32-byte values) -> MTH(0, n)"""
        arr = (np.ascontiguousarray(leaf_hashes, np.uint8) if isinstance(leaf_hashes, np.ndarray)
               else _digests([bytes(h) for h in leaf_hashes]))
        if arr.ndim != 2 or arr.shape[1] != 32:
            raise ValueError('leaf hashes must be (k, 32) bytes')
        if not len(arr):
            return self.root_hash
        root = np.zeros(32, np.uint8)
        nat._check('pv_merkle_tree_stage_hashes', nat.load().pv_merkle_tree_stage_hashes(self._h(), _p(arr), len(arr),
                                                                                        _p(root)))
        self._n += len(arr)
        return root.tobytes()

    def commit(self, count):
        nat._check('pv_merkle_tree_commit', nat.load().pv_merkle_tree_commit(self._h(), int(count)))
        first = self._committed
        self._committed += int(count)
        if self.hashStore is not None and count:
            self._write_store(first, self._committed)

    def discard(self, count):
        """drop the last `count` staged leaves -> the new root"""
        root = np.zeros(32, np.uint8)
        nat._check('pv_merkle_tree_discard', nat.load().pv_merkle_tree_discard(self._h(), int(count), _p(root)))
        self._n -= int(count)
        return root.tobytes()

    def frontier(self, size=None):
        """CompactMerkleTree.hashes of the prefix of `size` leaves (default: all)"""
        size = self._n if size is None else int(size)
        out, cnt = np.zeros((64, 32), np.uint8), ctypes.c_uint32(0)
        nat._check('pv_merkle_tree_frontier', nat.load().pv_merkle_tree_frontier(self._h(), size, _p(out),
                                                                                 ctypes.byref(cnt)))
        return tuple(out[i].tobytes() for i in range(cnt.value))

    def hash_store_arrays(self, first, last):
        """what the hash store receives for leaves first + 1 .. last ->
        (leaf hashes (last - first, 32) uint8, nodes (n_nodes, 32) uint8 in writeNode order)"""
        first, last = int(first), int(last)
        need = ctypes.c_uint64(0)
        nat._check('pv_merkle_tree_hash_store', nat.load().pv_merkle_tree_hash_store(
            self._h(), first, last, _p(None), _p(None), 0, ctypes.byref(need)))
        leafs = np.zeros((last - first, 32), np.uint8)
        nodes = np.zeros((need.value, 32), np.uint8)
        nat._check('pv_merkle_tree_hash_store', nat.load().pv_merkle_tree_hash_store(
            self._h(), first, last, _p(leafs), _p(nodes), need.value, ctypes.byref(need)))
        return leafs, nodes

    def check_nodes(self, first, last, nodes):
        """compare the stored nodes of leaves first + 1 .. last -> (differing, first differing index or None)"""
        arr = nodes if isinstance(nodes, np.ndarray) else _digests([bytes(h) for h in nodes])
        arr = np.ascontiguousarray(arr, np.uint8)
        need = (int(last) - bin(int(last)).count('1')) - (int(first) - bin(int(first)).count('1'))
        if arr.shape != (need, 32):
            raise ValueError('leaves ({}, {}] have {} nodes, {} given'.format(first, last, need, len(arr)))
        bad, at = ctypes.c_uint64(0), ctypes.c_uint64(0)
        nat._check('pv_merkle_tree_check_nodes', nat.load().pv_merkle_tree_check_nodes(
            self._h(), int(first), int(last), _p(arr), ctypes.byref(bad), ctypes.byref(at)))
        return bad.value, (None if at.value == _U64_MAX else at.value)

    # ------------------------------------------------------- the inherited writes
    def _extended(self, before):
        self._committed = self._n
        if self.hashStore is not None and self._n > before:
            self._write_store(before, self._n)

    def extend(self, leaves):
        before = self._n
        super().extend(leaves)
        self._extended(before)

    def extend_hashes(self, leaf_hashes):
        before = self._n
        super().extend_hashes(leaf_hashes)
        self._extended(before)

    # ------------------------------------------------------- plenum/common/ledger.py
    @property
    def size(self):
        """committed leaves (Ledger.size)"""
        return self._committed

    @property
    def uncommitted_size(self):
        return self._n

    @property
    def committed_root_hash(self):
        """Ledger.tree.root_hash"""
        if self._committed == 0:
            return _EMPTY_ROOT
        return self.merkle_tree_hash(0, self._committed)

    @property
    def uncommitted_root_hash(self):
        return self.uncommittedRootHash if self.uncommittedRootHash else self.committed_root_hash

    @property
    def hashes(self):
        """CompactMerkleTree.hashes of the staged tree (all leaves)"""
        return self.frontier(self._n)

    def appendTxns(self, leaves):
        """Ledger.appendTxns over serialized txns -> (start, end) sequence numbers.
        uncommittedRootHash stays None while nothing is staged (the reference sets
        it to the committed root after an empty batch on a clean ledger)."""
        leaves = list(leaves)
        before = self._n
        if leaves:
            self.uncommittedRootHash = self.stage(leaves)
            return before + 1, before + len(leaves)
        return before, before

    def commitTxns(self, count):
        """Ledger.commitTxns -> (start, end) sequence numbers of the committed txns"""
        count = int(count)
        before = self._committed
        self.commit(count)
        if self._committed == self._n:
            self.uncommittedRootHash = None
        if count:
            return before + 1, before + count
        return before, before

    def discardTxns(self, count):
        count = int(count)
        if count == 0:
            return
        staged = self._n - self._committed
        if count > staged:
            raise LogicError("expected to revert {} txns while there are only {}".
                             format(count, staged))
        root = self.discard(count)
        self.uncommittedRootHash = root if self._n > self._committed else None

    def reset_uncommitted(self):
        self.discardTxns(self._n - self._committed)
        self.uncommittedRootHash = None

    # ------------------------------------------------------------- hash store
    def _write_store(self, first, last):
        leafs, nodes = self.hash_store_arrays(first, last)
        at = 0
        for j, e in enumerate(range(first + 1, last + 1)):
            self.hashStore.writeLeaf(leafs[j].tobytes())
            for h in range(1, (e & -e).bit_length()):   # ctz(e) completed nodes, as _push_subtree names them
                self.hashStore.writeNode((e, h, nodes[at].tobytes()))
                at += 1

    @staticmethod
    def get_expected_node_count(leaf_count):
        count = 0
        while leaf_count > 1:
            leaf_count //= 2
            count += leaf_count
        return count

    @classmethod
    def recover(cls, hash_store, expected_leaf_count, **kwargs):
        """A tree rebuilt from a hash store (Ledger.recoverTreeFromHashStore): one
        extend of the stored leaf hashes, the count checks of
        CompactMerkleTree.verify_consistency, then every stored node compared with
        the rebuilt tree.  ConsistencyVerificationFailed tells the caller to fall
        back to the transaction log."""
        leaf_count, node_count = hash_store.leafCount, hash_store.nodeCount
        if expected_leaf_count != leaf_count:
            raise ConsistencyVerificationFailed()
        if cls.get_expected_node_count(leaf_count) != node_count:
            raise ConsistencyVerificationFailed()
        tree = cls(capacity_hint=max(1, leaf_count), **kwargs)
        try:
            if leaf_count:
                leafs = [bytes(h) for h in hash_store.readLeafs(1, leaf_count)]
                if len(leafs) != leaf_count or not all(len(h) == 32 for h in leafs):
                    raise ConsistencyVerificationFailed()
                tree.extend_hashes(leafs)          # hashStore is not attached yet: nothing is written back
                nodes = [_hash_of(x) for x in hash_store.readNodes(1, node_count)] if node_count else []
                if len(nodes) != node_count or not all(len(h) == 32 for h in nodes):
                    raise ConsistencyVerificationFailed()
                if tree.check_nodes(0, leaf_count, nodes)[0]:
                    raise ConsistencyVerificationFailed()
        except Exception:
            tree.close()
            raise
        tree.hashStore = hash_store
        return tree

    # ---------------------------------------------------------------- catch-up
    def accept_catchup_replies(self, reps, final_size, final_hash):
        """reps: [(leaves, consistency proof)] contiguous from size + 1, each proof
        from the tree at the reply's end to (final_size, final_hash).  All leaves
        are staged at once, the roots at every reply's end come from one call and
        the proofs are checked in one batch; the longest valid prefix of replies
        is committed, the rest discarded.  Returns the number of replies accepted
        (_process_catchup_txns stops at the first reply that does not verify)."""
        if self._n != self._committed:
            raise LogicError('catch-up onto a ledger with {} uncommitted txns'.format(self._n - self._committed))
        reps = [([bytes(x) for x in leaves], list(proof)) for leaves, proof in reps]
        if not reps:
            return 0
        base = self._committed
        ends, at = [], base
        for leaves, _ in reps:
            at += len(leaves)
            ends.append(at)
        self.stage([x for leaves, _ in reps for x in leaves])
        try:
            if at == base:
                roots = [self.committed_root_hash] * len(reps)
            else:
                sizes = [max(e, 1) for e in ends]
                _, _, got = self.paths_arrays(self._u64([0] * len(reps)), self._u64(sizes))
                roots = [got[i].tobytes() if ends[i] else _EMPTY_ROOT for i in range(len(reps))]
            items = [(ends[i], int(final_size), roots[i], bytes(final_hash), reps[i][1]) for i in range(len(reps))]
            verdicts = GpuMerkleVerifier(self.hasher).verify_tree_consistency_batch(items)
        except Exception:
            self.discard(self._n - base)
            raise
        accepted = 0
        while accepted < len(reps) and verdicts[accepted] is None:
            accepted += 1
        keep = ends[accepted - 1] - base if accepted else 0
        self.commit(keep)
        self.discard(self._n - self._committed)
        return accepted
