"""Merkle audit paths and consistency proofs, batched on the GPU.

* `GpuMerkleVerifier` mirrors ledger/merkle_verifier.py `MerkleVerifier`
  (verify_tree_consistency, verify_leaf_hash_inclusion, verify_leaf_inclusion,
  audit_path_length, _calculate_root_hash_from_audit_path): the single-item
  methods return True or raise the reference's exception class with the
  reference's text.  The `*_batch` methods check many proofs in one GPU call
  (pv_merkle_verify_inclusion / pv_merkle_verify_consistency, one proof per
  lane) and return, per item, None or the exception instance the single-item
  method would have raised.
* `GpuMerkleTree` is the device-resident tree behind the read side of
  ledger/compact_merkle_tree.py `CompactMerkleTree` (inclusion_proof,
  consistency_proof, merkle_tree_hash(0, s), root_hash) with batch forms and
  the dicts of `Ledger.merkleInfo` / `Ledger.auditProof`
  (ledger/ledger.py:196-217).

Size dispatch as in merkle.py (not a fallback): a lone proof is a chain of a
few dozen SHA-256 compressions, cheaper in hashlib than one launch, so the
single-item methods and batches below `GPU_MIN_ITEMS` run on the host.  Batches
at or above it need the GPU: a missing library or device raises.
"""
import ctypes
from binascii import hexlify
from collections import namedtuple

import numpy as np

from . import _native as nat
from . import base58
from .exceptions import ConsistencyError, ProofError
from .merkle import GPU_MIN_ITEMS, GpuTreeHasher   # noqa: F401  (GPU_MIN_ITEMS: this module's own knob)

# ledger/util.py:64
STH = namedtuple('STH', ['tree_size', 'sha256_root_hash'])

# status codes of include/plenum_verify.h
PV_MP_OK, PV_MP_BAD_RANGE, PV_MP_TOO_SHORT, PV_MP_TOO_LONG, PV_MP_ROOT_MISMATCH, PV_MP_INCONSISTENT = range(6)
PV_MP_LEN_REFUSED = 0xffffffff
_U64 = 1 << 64
_NULL = ctypes.c_void_p(0)


def _p(a):
    return _NULL if a is None else (nat._ptr(a) or _NULL)


def _digests(items):
    """[32-byte values] -> (n, 32) uint8"""
    if not items:
        return np.zeros((0, 32), np.uint8)
    return np.frombuffer(b''.join(items), np.uint8).reshape(len(items), 32).copy()


def _root_table(roots):
    """deduplicate roots -> (table (r, 32) uint8, idx uint32[n])"""
    seen, idx = {}, np.zeros(len(roots), np.uint32)
    for i, r in enumerate(roots):
        idx[i] = seen.setdefault(r, len(seen))
    return _digests(list(seen)), idx


def _pack_proofs(proofs):
    off = np.zeros(len(proofs) + 1, np.uint64)
    if proofs:
        off[1:] = np.cumsum(np.fromiter((len(p) for p in proofs), np.uint64, count=len(proofs)))
    flat = [h for p in proofs for h in p]
    return _digests(flat), off


def _is32(h):
    return isinstance(h, (bytes, bytearray)) and len(h) == 32


def _incl_range_error(leaf_index, tree_size):
    """the two ValueErrors of verify_leaf_hash_inclusion, in its order"""
    if tree_size <= leaf_index:
        return ValueError("Provided STH is for a tree that is smaller "
                          "than the leaf index. Tree size: %d Leaf "
                          "index: %d" % (tree_size, leaf_index))
    if tree_size < 0 or leaf_index < 0:
        return ValueError("Negative tree size or leaf index: "
                          "Tree size: %d Leaf index: %d" %
                          (tree_size, leaf_index))
    return None


def _cons_range_error(old_size, new_size):
    if old_size < 0 or new_size < 0:
        return ValueError("Negative tree size")
    if old_size > new_size:
        return ValueError("Older tree has bigger size (%d vs %d), did "
                          "you supply inputs in the wrong order?" %
                          (old_size, new_size))
    return None


def _root_differs(calculated, expected):
    return ProofError("Constructed root hash differs from provided "
                      "root hash. Constructed: %s Expected: %s" %
                      (hexlify(calculated).strip(),
                       hexlify(expected).strip()))


def _second_differs(new_root, new_hash):
    return ProofError("Bad Merkle proof: second root hash "
                      "does not match. Expected hash: %s "
                      ", computed hash: %s" %
                      (hexlify(new_root).strip(),
                       hexlify(new_hash).strip()))


def _first_differs(old_root, old_hash):
    return ConsistencyError("Inconsistency: first root hash "
                            "does not match. Expected hash: "
                            "%s, computed hash: %s" %
                            (hexlify(old_root).strip(),
                             hexlify(old_hash).strip()))


class GpuMerkleVerifier:
    """ledger/merkle_verifier.py MerkleVerifier with batch entry points."""

    def __init__(self, hasher=None):
        self.hasher = hasher if hasher is not None else GpuTreeHasher()

    def __repr__(self):
        return "%r(hasher: %r)" % (self.__class__.__name__, self.hasher)

    def __str__(self):
        return "%s(hasher: %s)" % (self.__class__.__name__, self.hasher)

    # ------------------------------------------------ single items (host)
    def verify_tree_consistency(self, old_tree_size, new_tree_size, old_root, new_root, proof):
        old_size, new_size = old_tree_size, new_tree_size
        err = _cons_range_error(old_size, new_size)
        if err is not None:
            raise err
        if old_size == new_size:
            if old_root == new_root:
                return True
            raise ConsistencyError("Inconsistency: different root "
                                   "hashes for the same tree size")
        if old_size == 0:
            return True
        node, last_node = old_size - 1, new_size - 1
        while node % 2:
            node //= 2
            last_node //= 2
        p = iter(proof)
        try:
            if node:
                new_hash = old_hash = next(p)
            else:
                new_hash = old_hash = old_root
            while node:
                if node % 2:
                    next_node = next(p)
                    old_hash = self.hasher.hash_children(next_node, old_hash)
                    new_hash = self.hasher.hash_children(next_node, new_hash)
                elif node < last_node:
                    new_hash = self.hasher.hash_children(new_hash, next(p))
                node //= 2
                last_node //= 2
            while last_node:
                new_hash = self.hasher.hash_children(new_hash, next(p))
                last_node //= 2
            if new_hash != new_root:
                raise _second_differs(new_root, new_hash)
            elif old_hash != old_root:
                raise _first_differs(old_root, old_hash)
        except StopIteration:
            raise ProofError("Merkle proof is too short")
        return True   # extra nodes are accepted

    def _calculate_root_hash_from_audit_path(self, leaf_hash, node_index, audit_path, tree_size):
        calculated_hash = leaf_hash
        last_node = tree_size - 1
        while last_node > 0:
            if not audit_path:
                raise ProofError('Proof too short: left with node index '
                                 '%d' % node_index)
            if node_index % 2:
                calculated_hash = self.hasher.hash_children(audit_path.pop(0), calculated_hash)
            elif node_index < last_node:
                calculated_hash = self.hasher.hash_children(calculated_hash, audit_path.pop(0))
            node_index //= 2
            last_node //= 2
        if audit_path:
            raise ProofError('Proof too long: Left with %d hashes.' %
                             len(audit_path))
        return calculated_hash

    @classmethod
    def audit_path_length(cls, index, tree_size):
        length = 0
        last_node = tree_size - 1
        while last_node > 0:
            if index % 2 or index < last_node:
                length += 1
            index //= 2
            last_node //= 2
        return length

    def verify_leaf_hash_inclusion(self, leaf_hash, leaf_index, proof, sth):
        leaf_index = int(leaf_index)
        tree_size = int(sth.tree_size)
        err = _incl_range_error(leaf_index, tree_size)
        if err is not None:
            raise err
        calculated = self._calculate_root_hash_from_audit_path(leaf_hash, leaf_index, list(proof), tree_size)
        if calculated == sth.sha256_root_hash:
            return True
        raise _root_differs(calculated, sth.sha256_root_hash)

    def verify_leaf_inclusion(self, leaf, leaf_index, proof, sth):
        return self.verify_leaf_hash_inclusion(self.hasher.hash_leaf(leaf), leaf_index, proof, sth)

    # ------------------------------------------------------------ batches
    @staticmethod
    def _single(fn, *args):
        try:
            fn(*args)
            return None
        except (ProofError, ConsistencyError, ValueError) as e:
            return e

    def _inclusion_batch(self, leaves, indices, proofs, sths, hashed):
        single = self.verify_leaf_hash_inclusion if hashed else self.verify_leaf_inclusion
        n = len(leaves)
        if not (n == len(indices) == len(proofs) == len(sths)):
            raise ValueError('leaves, indices, proofs and sths differ in length')
        if n < GPU_MIN_ITEMS:
            return [self._single(single, leaves[i], indices[i], proofs[i], sths[i]) for i in range(n)]
        out = [None] * n
        gpu = []   # item numbers that go to the GPU
        for i in range(n):
            idx, size = int(indices[i]), int(sths[i].tree_size)
            err = _incl_range_error(idx, size)
            if err is not None:       # the range checks are made on the host, before packing
                out[i] = err
            elif (size >= _U64 or (hashed and not _is32(leaves[i])) or not _is32(sths[i].sha256_root_hash) or
                  not all(_is32(h) for h in proofs[i])):
                # the reference hashes such operands as they are: same verdict from the same walk
                out[i] = self._single(single, leaves[i], indices[i], proofs[i], sths[i])
            else:
                gpu.append(i)
        if not gpu:
            return out
        nat.ensure_init()
        k = len(gpu)
        index = np.fromiter((int(indices[i]) for i in gpu), np.uint64, count=k)
        size = np.fromiter((int(sths[i].tree_size) for i in gpu), np.uint64, count=k)
        nodes, poff = _pack_proofs([proofs[i] for i in gpu])
        roots, ridx = _root_table([bytes(sths[i].sha256_root_hash) for i in gpu])
        status = np.zeros(k, np.uint8)
        computed = np.zeros((k, 32), np.uint8)
        stop = np.zeros(k, np.uint64)
        if hashed:
            lh, blob, loff = _digests([bytes(leaves[i]) for i in gpu]), None, None
        else:
            lh = None
            blob, loff = nat.pack_messages([bytes(leaves[i]) for i in gpu])
            blob, loff = np.ascontiguousarray(blob, np.uint8), np.ascontiguousarray(loff, np.uint64)
        nat._check('pv_merkle_verify_inclusion', nat.load().pv_merkle_verify_inclusion(
            _p(lh), _p(blob), _p(loff), _p(index), _p(size), _p(nodes), _p(poff), _p(roots), _p(ridx),
            len(roots), k, _p(status), _p(computed), _p(stop)))
        for j, i in enumerate(gpu):
            st = int(status[j])
            if st == PV_MP_OK:
                continue
            if st == PV_MP_TOO_SHORT:
                out[i] = ProofError('Proof too short: left with node index '
                                    '%d' % int(stop[j]))
            elif st == PV_MP_TOO_LONG:
                out[i] = ProofError('Proof too long: Left with %d hashes.' %
                                    (len(proofs[i]) - self.audit_path_length(int(index[j]), int(size[j]))))
            elif st == PV_MP_ROOT_MISMATCH:
                out[i] = _root_differs(computed[j].tobytes(), bytes(sths[i].sha256_root_hash))
            else:
                raise RuntimeError('pv_merkle_verify_inclusion: unexpected status %d for item %d' % (st, i))
        return out

    def verify_leaf_hash_inclusion_batch(self, leaf_hashes, indices, proofs, sths):
        """[None | exception] per (leaf_hash, index, proof, sth)"""
        return self._inclusion_batch(leaf_hashes, indices, proofs, sths, True)

    def verify_leaf_inclusion_batch(self, leaves, indices, proofs, sths):
        """as above from the leaf data: the leaves are hashed on the GPU too"""
        return self._inclusion_batch(leaves, indices, proofs, sths, False)

    def verify_tree_consistency_batch(self, items):
        """items: (old_tree_size, new_tree_size, old_root, new_root, proof) each"""
        n = len(items)
        if n < GPU_MIN_ITEMS:
            return [self._single(self.verify_tree_consistency, *it) for it in items]
        out = [None] * n
        gpu = []
        for i, (old, new, r0, r1, proof) in enumerate(items):
            err = _cons_range_error(old, new)
            if err is not None:
                out[i] = err
            elif new >= _U64 or not _is32(r0) or not _is32(r1) or not all(_is32(h) for h in proof):
                out[i] = self._single(self.verify_tree_consistency, old, new, r0, r1, proof)
            else:
                gpu.append(i)
        if not gpu:
            return out
        nat.ensure_init()
        k = len(gpu)
        old = np.fromiter((int(items[i][0]) for i in gpu), np.uint64, count=k)
        new = np.fromiter((int(items[i][1]) for i in gpu), np.uint64, count=k)
        table, idx = _root_table([bytes(items[i][2]) for i in gpu] + [bytes(items[i][3]) for i in gpu])
        io, inw = np.ascontiguousarray(idx[:k]), np.ascontiguousarray(idx[k:])
        nodes, poff = _pack_proofs([items[i][4] for i in gpu])
        status = np.zeros(k, np.uint8)
        oc, nc = np.zeros((k, 32), np.uint8), np.zeros((k, 32), np.uint8)
        nat._check('pv_merkle_verify_consistency', nat.load().pv_merkle_verify_consistency(
            _p(old), _p(new), _p(table), _p(table), _p(io), _p(inw), len(table), _p(nodes), _p(poff), k,
            _p(status), _p(oc), _p(nc)))
        for j, i in enumerate(gpu):
            st = int(status[j])
            if st == PV_MP_OK:
                continue
            if st == PV_MP_TOO_SHORT:
                out[i] = ProofError("Merkle proof is too short")
            elif st == PV_MP_ROOT_MISMATCH:
                out[i] = _second_differs(bytes(items[i][3]), nc[j].tobytes())
            elif st == PV_MP_INCONSISTENT and old[j] == new[j]:
                out[i] = ConsistencyError("Inconsistency: different root "
                                          "hashes for the same tree size")
            elif st == PV_MP_INCONSISTENT:
                out[i] = _first_differs(bytes(items[i][2]), oc[j].tobytes())
            else:
                raise RuntimeError('pv_merkle_verify_consistency: unexpected status %d for item %d' % (st, i))
        return out


class GpuMerkleTree:
    """A Merkle tree whose every level stays on the GPU: the read side of
    ledger/compact_merkle_tree.py CompactMerkleTree for whole batches of
    requests.  Needs the GPU (no host copy of the tree exists)."""

    def __init__(self, hasher=None, capacity_hint=1024, device=0):
        self.hasher = hasher if hasher is not None else GpuTreeHasher()
        self._handle = None
        nat.ensure_init()
        h = ctypes.c_int32(0)
        nat._check('pv_merkle_tree_create', nat.load().pv_merkle_tree_create(int(capacity_hint), int(device),
                                                                             ctypes.byref(h)))
        self._handle = h.value
        self._n = 0

    def close(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            nat.load().pv_merkle_tree_free(handle)   # already gone after a shutdown: nothing to do

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter teardown
            pass

    def __len__(self):
        return self._n

    def _h(self):
        if self._handle is None:
            raise ValueError('the tree is closed')
        return self._handle

    # ---------------------------------------------------------------- writes
    def extend(self, leaves):
        """append leaves (bytes each), hashed on the GPU as SHA-256(0x00 || leaf)"""
        leaves = [bytes(x) for x in leaves]
        if not leaves:
            return
        blob, off = nat.pack_messages(leaves)
        blob, off = np.ascontiguousarray(blob, np.uint8), np.ascontiguousarray(off, np.uint64)
        nat._check('pv_merkle_tree_extend', nat.load().pv_merkle_tree_extend(self._h(), _p(blob), _p(off),
                                                                             len(leaves)))
        self._n += len(leaves)

    def append(self, leaf):
        self.extend([leaf])

    def extend_hashes(self, leaf_hashes):
        """append leaf hashes: a (k, 32) uint8 array or a sequence of 32-byte values"""
        if isinstance(leaf_hashes, np.ndarray):
            arr = np.ascontiguousarray(leaf_hashes, np.uint8)
            if arr.ndim != 2 or arr.shape[1] != 32:
                raise ValueError('leaf hashes must be (k, 32) bytes')
        else:
            leaf_hashes = [bytes(h) for h in leaf_hashes]
            if not all(len(h) == 32 for h in leaf_hashes):
                raise ValueError('leaf hashes must be 32 bytes each')
            arr = _digests(leaf_hashes)
        if not len(arr):
            return
        nat._check('pv_merkle_tree_extend_hashes', nat.load().pv_merkle_tree_extend_hashes(self._h(), _p(arr),
                                                                                          len(arr)))
        self._n += len(arr)

    # ----------------------------------------------------------------- reads
    @property
    def tree_size(self):
        return self._n

    def _info(self):
        n, depth, root = ctypes.c_uint64(0), ctypes.c_uint32(0), np.zeros(32, np.uint8)
        nat._check('pv_merkle_tree_info', nat.load().pv_merkle_tree_info(self._h(), ctypes.byref(n),
                                                                         ctypes.byref(depth), _p(root)))
        return n.value, depth.value, root.tobytes()

    @property
    def depth(self):
        return self._info()[1]

    @property
    def root_hash(self):
        return self._info()[2]

    def paths_arrays(self, index, tree_size):
        """uint64 arrays -> (nodes (k, depth + 1, 32) uint8, lengths uint32[k], roots (k, 32) uint8)"""
        index = np.ascontiguousarray(index, np.uint64)
        tree_size = np.ascontiguousarray(tree_size, np.uint64)
        k, stride = len(index), self.depth + 1
        nodes = np.zeros((k, stride, 32), np.uint8)
        lens = np.zeros(k, np.uint32)
        roots = np.zeros((k, 32), np.uint8)
        nat._check('pv_merkle_audit_paths', nat.load().pv_merkle_audit_paths(
            self._h(), _p(index), _p(tree_size), k, _p(nodes), _p(lens), _p(roots)))
        return nodes, lens, roots

    def proofs_arrays(self, first, second):
        first = np.ascontiguousarray(first, np.uint64)
        second = np.ascontiguousarray(second, np.uint64)
        k, stride = len(first), self.depth + 1
        nodes = np.zeros((k, stride, 32), np.uint8)
        lens = np.zeros(k, np.uint32)
        nat._check('pv_merkle_consistency_proofs', nat.load().pv_merkle_consistency_proofs(
            self._h(), _p(first), _p(second), k, _p(nodes), _p(lens)))
        return nodes, lens

    @staticmethod
    def _u64(values):
        values = [int(v) for v in values]
        if any(v < 0 or v >= _U64 for v in values):
            raise ValueError('index or size outside 0 .. 2^64 - 1')
        return np.array(values, np.uint64)

    @staticmethod
    def _lists(nodes, lens):
        return [[nodes[i, j].tobytes() for j in range(int(lens[i]))] for i in range(len(lens))]

    def inclusion_proofs(self, pairs):
        """[(m, s)] -> [CompactMerkleTree.inclusion_proof(m, s)], one GPU call"""
        pairs = list(pairs)
        if not pairs:
            return []
        nodes, lens, _ = self.paths_arrays(self._u64(p[0] for p in pairs), self._u64(p[1] for p in pairs))
        return self._lists(nodes, lens)

    def inclusion_proof(self, start, end):
        return self.inclusion_proofs([(start, end)])[0]

    def consistency_proofs(self, pairs):
        """[(first, second)] -> [CompactMerkleTree.consistency_proof(first, second)]"""
        pairs = list(pairs)
        if not pairs:
            return []
        nodes, lens = self.proofs_arrays(self._u64(p[0] for p in pairs), self._u64(p[1] for p in pairs))
        return self._lists(nodes, lens)

    def consistency_proof(self, first, second):
        return self.consistency_proofs([(first, second)])[0]

    def merkle_tree_hash(self, start, end):
        """MTH of leaves [start, end); only start == 0 (what the ledger asks for)"""
        if not end > start:
            raise ValueError("end must be greater than start")
        if start != 0:
            raise NotImplementedError('merkle_tree_hash(start != 0): the proof calls gather those nodes themselves')
        if end == self._n:
            return self.root_hash
        _, _, roots = self.paths_arrays(self._u64([0]), self._u64([end]))
        return roots[0].tobytes()

    # -------------------------------------------------- ledger-shaped helpers
    @staticmethod
    def _seq_nos(seq_nos):
        seq_nos = [int(s) for s in seq_nos]
        for s in seq_nos:
            if s <= 0:   # PlenumValueError('seqNo', seqNo, '> 0'), ledger/ledger.py:198
                raise ValueError("variable '{}', value {}, expected: {}".format('seqNo', s, '> 0'))
        return seq_nos

    @staticmethod
    def hashToStr(h):
        return base58.b58encode(h).decode('utf-8')

    def _dicts(self, seq_nos, sizes, with_size):
        if not seq_nos:
            return []
        nodes, lens, roots = self.paths_arrays(self._u64(s - 1 for s in seq_nos), self._u64(sizes))
        out = []
        for i, path in enumerate(self._lists(nodes, lens)):
            d = {'rootHash': self.hashToStr(roots[i].tobytes()), 'auditPath': [self.hashToStr(h) for h in path]}
            if with_size:
                d['ledgerSize'] = int(sizes[i])
            out.append(d)
        return out

    def merkle_infos(self, seq_nos):
        """[Ledger.merkleInfo(seqNo)]: root and audit path of the tree of size seqNo"""
        seq_nos = self._seq_nos(seq_nos)
        return self._dicts(seq_nos, seq_nos, False)

    def audit_proofs(self, seq_nos):
        """[Ledger.auditProof(seqNo)]: root and audit path in the current tree, and its size"""
        seq_nos = self._seq_nos(seq_nos)
        return self._dicts(seq_nos, [self._n] * len(seq_nos), True)
