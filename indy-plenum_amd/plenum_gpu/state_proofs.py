"""Patricia-trie state proofs and SHA3-256, batched on the GPU.

A read reply is trusted after three checks: the BLS multi-signature over the
state root (bls.py), the Merkle audit path of the transaction
(merkle_proofs.py) and the state proof, the trie nodes that tie (key, value)
to the signed state root.  This module is the third:

* `sha3_256_batch(msgs)`: the trie's hash (state/util/utils.py:7-8,156-157).
* `GpuStateVerifier` has the static methods of state/pruning_state.py:113-128
  `PruningState` (verify_state_proof, verify_state_proof_multi,
  encode_kv_for_verification) with the reference's signatures and verdicts.
* `verify_state_proofs_batch(items)` checks many replies in one GPU call
  (pv_state_proof_verify: every proof node hashed once by k_sha3_256, then one
  lane per (proof, key, value) query walks the trie in k_trie_verify).

Serialized proofs (`Trie.serialize_proof` = rlp(list of nodes),
state/trie/pruning_trie.py:1164-1170) go in as they are: each node's RLP is a
slice of the serialized bytes, found by pv_rlp_split_list; nothing is decoded or
re-encoded.  Unserialized proofs (lists of decoded nodes) are RLP-encoded by
`rlp_encode` below.

Two deliberate differences from the reference:

* A serialized proof that is not one RLP list yields False for its queries.
  The reference lets the decoder's exception escape there (deserialize_proof
  runs outside the try of verify_spv_proof).
* A proof node that is not a well-formed trie node gives False by rule.  Such
  a node is reachable from a trusted root only through a SHA3 preimage, so
  parity with the exact exception pyrlp would raise does not apply; what is
  guaranteed is that no length is trusted before it is checked.

Size dispatch as in merkle.py (not a fallback): below `GPU_MIN_ITEMS` queries
the walk runs here, in a pure-Python mirror of csrc/pv_trie_proof.h with
hashlib; at or above it the GPU is required and a missing library or device
raises.
"""
import ctypes
import hashlib

import numpy as np

from . import _native as nat

# below this many queries (messages, for sha3_256_batch) the host is faster
# than one upload + two launches; tests set it to 0 to push every size through
# the GPU kernels
GPU_MIN_ITEMS = 512

# status codes of include/plenum_verify.h
PV_SP_OK, PV_SP_VALUE_MISMATCH, PV_SP_NODE_MISSING, PV_SP_MALFORMED = range(4)

BLANK_NODE = b''
BLANK_ROOT = hashlib.sha3_256(b'\x80').digest()   # sha3(rlp(b'')), pruning_trie.py:206-207

_NULL = ctypes.c_void_p(0)


def _p(a):
    return _NULL if a is None else (nat._ptr(a) or _NULL)


# ------------------------------------------------------------------ RLP
def _length_prefix(length, offset):
    if length < 56:
        return bytes([offset + length])
    ls = length.to_bytes((length.bit_length() + 7) // 8, 'big')
    return bytes([offset + 55 + len(ls)]) + ls


def rlp_encode(item):
    """RLP of (a nested sequence of) bytes: what rlp.codec.encode_raw gives the trie."""
    if isinstance(item, (bytes, bytearray, memoryview)):
        item = bytes(item)
        if len(item) == 1 and item[0] < 128:
            return item
        return _length_prefix(len(item), 128) + item
    if isinstance(item, (list, tuple)):
        body = b''.join(rlp_encode(x) for x in item)
        return _length_prefix(len(body), 192) + body
    raise TypeError('cannot RLP-encode {!r}'.format(type(item)))


def _rlp_item(b, pos, lim):
    """One item at pos inside [pos, lim) -> (is_list, payload begin, payload end),
    or None when the header or the payload overruns lim (rlp_item of pv_trie_proof.h;
    lengths as state/util/fast_rlp.py:47-71)."""
    if pos >= lim:
        return None
    b0 = b[pos]
    if b0 < 128:
        return False, pos, pos + 1
    ll = 0
    if b0 < 184:
        is_list, length = False, b0 - 128
    elif b0 < 192:
        is_list, length, ll = False, 0, b0 - 183
    elif b0 < 248:
        is_list, length = True, b0 - 192
    else:
        is_list, length, ll = True, 0, b0 - 247
    if ll > lim - pos - 1:
        return None
    if ll:
        length = int.from_bytes(b[pos + 1:pos + 1 + ll], 'big')
    pbeg = pos + 1 + ll
    if length > lim - pbeg:
        return None
    return is_list, pbeg, pbeg + length


def rlp_split_list(data):
    """[(begin, end)] of the top-level items of the RLP list `data`, each with its
    own header, or None when `data` is not one list whose items end exactly at its
    end (rlp_split_list of pv_trie_proof.h)."""
    head = _rlp_item(data, 0, len(data))
    if head is None or not head[0] or head[2] != len(data):
        return None
    out, pos, pe = [], head[1], head[2]
    while pos < pe:
        it = _rlp_item(data, pos, pe)
        if it is None:
            return None
        out.append((pos, it[2]))
        pos = it[2]
    return out


# ------------------------------------------------------ the walk, mirrored
def _nibble(b, base, i):
    v = b[base + (i >> 1)]
    return (v & 15) if (i & 1) else (v >> 4)


def walk_status(blob, ranges, digests, root, key, value):
    """sp_verify of csrc/pv_trie_proof.h in Python: `ranges` are the (begin, end)
    of the proof's nodes in `blob`, `digests` their SHA3-256, `value` the expected
    ENCODED value (b'' = None).  -> PV_SP_*"""
    blank = PV_SP_OK if len(value) == 0 else PV_SP_VALUE_MISMATCH
    if root == BLANK_ROOT:
        return blank
    try:
        cb, ce = ranges[digests.index(root)]
    except ValueError:
        return PV_SP_NODE_MISSING
    total, nib = 2 * len(key), 0
    for _ in range(total + 1):
        head = _rlp_item(blob, cb, ce)
        if head is None or not head[0] or head[2] != ce:
            return PV_SP_MALFORMED
        items, pos = [], head[1]
        while pos < ce:
            if len(items) == 17:
                return PV_SP_MALFORMED
            it = _rlp_item(blob, pos, ce)
            if it is None:
                return PV_SP_MALFORMED
            items.append((pos,) + it)      # (start, is_list, payload begin, payload end)
            pos = it[2]
        done = False
        if len(items) == 17:
            if nib == total:
                ref, done = items[16], True
            else:
                ref = items[_nibble(key, 0, nib)]
                nib += 1
        elif len(items) == 2:
            _, i0l, i0b, i0e = items[0]
            if i0l or i0e == i0b:
                return PV_SP_MALFORMED
            flags = blob[i0b] >> 4
            odd = flags & 1
            pn = 2 * (i0e - i0b - 1) + odd
            skip = 2 - odd
            left = total - nib
            leaf = bool(flags & 2)
            if not leaf and pn == 0:
                return PV_SP_MALFORMED
            match = (pn == left) if leaf else (pn <= left)
            if match:
                match = all(_nibble(blob, i0b, skip + i) == _nibble(key, 0, nib + i) for i in range(pn))
            if not match:
                return blank
            ref = items[1]
            if leaf:
                done = True
            else:
                nib += pn
        else:
            return PV_SP_MALFORMED
        rs, rl, rb, re = ref
        if done:
            if rl:
                return PV_SP_MALFORMED
            return PV_SP_OK if bytes(blob[rb:re]) == value else PV_SP_VALUE_MISMATCH
        if rl:                              # an inline node: its RLP is the item itself
            cb, ce = rs, re
            continue
        if re == rb:
            return blank
        if re - rb != 32:
            return PV_SP_NODE_MISSING
        try:
            cb, ce = ranges[digests.index(bytes(blob[rb:re]))]
        except ValueError:
            return PV_SP_NODE_MISSING
    return PV_SP_MALFORMED


# ------------------------------------------------------------- SHA3-256
def sha3_256_batch(msgs):
    """[bytes] -> [32-byte SHA3-256 digests] (pv_sha3_256_batch, k_sha3_256)."""
    msgs = [bytes(m) for m in msgs]
    n = len(msgs)
    if n == 0:
        return []
    if n < GPU_MIN_ITEMS:
        return [hashlib.sha3_256(m).digest() for m in msgs]
    nat.ensure_init()
    blob, off = nat.pack_messages(msgs)
    out = np.empty((n, 32), np.uint8)
    nat._check('pv_sha3_256_batch', nat.load().pv_sha3_256_batch(_p(blob), _p(off), n, _p(out)))
    return [out[i].tobytes() for i in range(n)]


# ---------------------------------------------------------------- packing
def _native_split(data):
    """rlp_split_list through pv_rlp_split_list (host code of the library, no GPU)"""
    buf = np.frombuffer(data, np.uint8)
    lib = nat.load()
    count = ctypes.c_uint64(0)
    for cap in (64, len(data)):
        beg, end = np.empty(cap, np.uint64), np.empty(cap, np.uint64)
        rc = lib.pv_rlp_split_list(_p(buf), len(data), _p(beg), _p(end), cap, ctypes.byref(count))
        if rc == 0:
            k = count.value
            return list(zip(beg[:k].tolist(), end[:k].tolist()))
        if count.value < cap:      # refused for its form, not for the capacity
            return None
    return None


class _Packed:
    """The arrays of one pv_state_proof_verify call, and per item its queries."""

    def __init__(self):
        self.chunks, self.blob_len = [], 0
        self.node_beg, self.node_end = [], []
        self.proof_first = [0]
        self.roots = []
        self.proof_idx, self.keys, self.vals = [], [], []
        self.item_queries = []      # per item: (first query, count, fixed verdict or None)

    def add_proof(self, root, proof_nodes, serialized, split):
        """-> proof index, or None for a serialized proof that does not split"""
        if serialized:
            data = bytes(proof_nodes)
            ranges = split(data)
            if ranges is None:
                return None
            base = self.blob_len
            self.chunks.append(data)
            self.blob_len += len(data)
            for b, e in ranges:
                self.node_beg.append(base + b)
                self.node_end.append(base + e)
        else:
            for node in proof_nodes:
                enc = rlp_encode(node)
                self.node_beg.append(self.blob_len)
                self.chunks.append(enc)
                self.blob_len += len(enc)
                self.node_end.append(self.blob_len)
        self.proof_first.append(len(self.node_beg))
        self.roots.append(root)
        return len(self.roots) - 1


def _normalise_root(root):
    """-> 32-byte root, or None when the reference's set_root_hash refuses it
    (pruning_trie.py:282-294; b'' is the blank node)"""
    if not isinstance(root, (bytes, bytearray)):
        return None
    root = bytes(root)
    if len(root) == 0:
        return BLANK_ROOT
    return root if len(root) == 32 else None


def _pack(items, split):
    pk = _Packed()
    for it in items:
        serialized = None
        if len(it) == 5:
            root, key, value, proof_nodes, serialized = it
            kvs = [GpuStateVerifier.encode_kv_for_verification(key, value)]
        elif len(it) == 4 and not isinstance(it[1], dict):
            root, key, value, proof_nodes = it
            kvs = [GpuStateVerifier.encode_kv_for_verification(key, value)]
        elif len(it) == 4:
            root, key_values, proof_nodes, serialized = it
            kvs = [GpuStateVerifier.encode_kv_for_verification(k, v) for k, v in key_values.items()]
        elif len(it) == 3:
            root, key_values, proof_nodes = it
            kvs = [GpuStateVerifier.encode_kv_for_verification(k, v) for k, v in key_values.items()]
        else:
            raise ValueError('an item is (root, key, value, proof_nodes) or (root, key_values, proof_nodes)')
        if serialized is None:
            serialized = isinstance(proof_nodes, (bytes, bytearray, memoryview))
        first = len(pk.proof_idx)
        root = _normalise_root(root)
        p = None if root is None else pk.add_proof(root, proof_nodes, serialized, split)
        if p is None:
            pk.item_queries.append((first, 0, False))
            continue
        if not kvs:      # verify_spv_proof_multi with no pairs: True iff the root node is there
            kvs = [(b'', b'')]
            pk.item_queries.append((first, 1, 'root'))
        else:
            pk.item_queries.append((first, len(kvs), None))
        for k, v in kvs:
            pk.proof_idx.append(p)
            pk.keys.append(bytes(k))
            pk.vals.append(bytes(v))
    return pk


def _statuses_host(pk):
    blob = b''.join(pk.chunks)
    digests = [hashlib.sha3_256(blob[b:e]).digest() for b, e in zip(pk.node_beg, pk.node_end)]
    ranges = list(zip(pk.node_beg, pk.node_end))
    out = np.zeros(len(pk.proof_idx), np.uint8)
    for i, p in enumerate(pk.proof_idx):
        f, l = pk.proof_first[p], pk.proof_first[p + 1]
        out[i] = walk_status(blob, ranges[f:l], digests[f:l], pk.roots[p], pk.keys[i], pk.vals[i])
    return out


def _statuses_gpu(pk):
    nat.ensure_init()
    q = len(pk.proof_idx)
    blob = np.frombuffer(b''.join(pk.chunks), np.uint8)
    beg, end = np.array(pk.node_beg, np.uint64), np.array(pk.node_end, np.uint64)
    first = np.array(pk.proof_first, np.uint64)
    roots = np.frombuffer(b''.join(pk.roots), np.uint8)
    pidx = np.array(pk.proof_idx, np.uint32)
    kblob, koff = nat.pack_messages(pk.keys)
    vblob, voff = nat.pack_messages(pk.vals)
    status = np.full(q, PV_SP_MALFORMED, np.uint8)
    nat._check('pv_state_proof_verify', nat.load().pv_state_proof_verify(
        _p(blob), blob.size, _p(beg), _p(end), _p(first), _p(roots), _p(pidx), _p(kblob), _p(koff), _p(vblob),
        _p(voff), beg.size, len(pk.roots), q, _p(status)))
    return status


def state_proof_statuses(items):
    """-> (PV_SP_* per query uint8, [(first query, count, fixed verdict or None)] per item)"""
    gpu = sum(len(it[1]) if isinstance(it[1], dict) else 1 for it in items) >= GPU_MIN_ITEMS
    pk = _pack(items, _native_split if gpu else rlp_split_list)
    if not pk.proof_idx:
        return np.zeros(0, np.uint8), pk.item_queries
    return (_statuses_gpu(pk) if gpu else _statuses_host(pk)), pk.item_queries


def verify_state_proofs_batch(items):
    """Verdicts of many state proofs in one call -> numpy bool array, one per item.

    An item is (root, key, value, proof_nodes) -- PruningState.verify_state_proof --
    or (root, key_values, proof_nodes) -- verify_state_proof_multi; an optional
    last element `serialized` overrides what the type of proof_nodes says (bytes =
    serialized, a list of nodes = not).  Keys and values are as the reference
    takes them (encode_kv_for_verification is applied here)."""
    items = list(items)
    status, queries = state_proof_statuses(items)
    out = np.zeros(len(items), bool)
    for i, (first, count, fixed) in enumerate(queries):
        if fixed is False:
            continue
        st = status[first:first + count]
        if fixed == 'root':
            out[i] = st[0] != PV_SP_NODE_MISSING and st[0] != PV_SP_MALFORMED
        else:
            out[i] = bool((st == PV_SP_OK).all())
    return out


class GpuStateVerifier:
    """state/pruning_state.py:113-128, the verification side of PruningState."""

    @staticmethod
    def verify_state_proof(root, key, value, proof_nodes, serialized=False):
        return bool(verify_state_proofs_batch([(root, key, value, proof_nodes, serialized)])[0])

    @staticmethod
    def verify_state_proof_multi(root, key_values, proof_nodes, serialized=False):
        return bool(verify_state_proofs_batch([(root, key_values, proof_nodes, serialized)])[0])

    @staticmethod
    def encode_kv_for_verification(key, value):
        encoded_key = key.encode() if isinstance(key, str) else key
        encoded_value = rlp_encode([value]) if value is not None else b''
        return encoded_key, encoded_value

    verify_state_proofs_batch = staticmethod(verify_state_proofs_batch)
