"""Resident trie node store: batched state-proof generation on the GPU.

The serving side of state_proofs.py.  A node answers every GET_* with
ReadRequestHandler._get_value_from_state
(plenum/server/request_handlers/handler_interfaces/read_request_handler.py:33-61):
one `generate_state_proof(key, root, serialize=True, get_value=True)` per reply.
The reference's trie database is content-addressed and append-only -- a node is
stored under sha3(rlp(node)) and never changes (state/trie/pruning_trie.py:346-353)
-- and generate_state_proof (:1043-1050, :1075-1098) is Trie._get from a root plus
a record of every node fetched by hash, with the root appended.  So nothing has to
be mutable on the device: `GpuStateStore` grows by "add these node RLPs", which the
host trie hands over on commit, and a proof at any committed root, current or
historical, is a walk over hash lookups.  A batch of replies is one call.

* `GpuStateStore.add_nodes(node RLPs)` -- pv_state_store_add: the nodes are appended
  to a device blob, hashed in place (k_sha3_256) and inserted into a digest-keyed hash
  table (k_trie_store_insert).
* `generate_state_proofs_batch([(root, key), ...])` -- pv_state_store_prove: one lane
  per query walks from its root (k_trie_prove), one wave per proof gathers the
  serialized bytes (k_trie_proof_pack).
* `generate_state_proof(key, root, serialize, get_value)` has PruningState's signature
  (state/pruning_state.py:105-106).
* `walk_host(db, root, key)` is the pure-Python mirror of sg_walk (csrc/pv_trie_store.h)
  plus the serialization: the statement of the algorithm, used by the CPU tests.

There is no CPU path here: the store lives on the device, and a missing library or
GPU raises.

Two deliberate differences from the reference.  Node order: a proof lists the hashed
nodes of the walk in reverse, terminal node first, root last.  Root last is the one
ordering property _generate_state_proof has (pf.append(root), and the NOTE at :1102);
the rest of the reference's order is Python set order.  Blank root: the proof is the
empty list (serialized: the one byte 0xc0), which is what the verifier accepts; the
reference would return [b''].

* `GpuStateStore.build_state(items)` / `state_root_batch(items)` -- pv_state_build: a whole
  trie from a batch of (key, value) pairs (csrc/pv_trie_build.h), the result of one
  PruningState.set per pair (state/pruning_state.py:60-61, Trie.update,
  state/trie/pruning_trie.py:1006-1027); `build_host(items)` is its pure-Python mirror.

* `GpuStateStore.update_state(root, items)` -- pv_state_update: one 3PC batch of sets applied to
  the state at a committed root (csrc/pv_trie_update.h): one lane per batch key walks the old trie in
  the store and carries the children no batch key enters as they are, and the build runs over the
  merged list; `update_host(db, root, items)` is its pure-Python mirror over a {hash: RLP} dict.

* `GpuStateStore.apply_batch(root, items)` / `remove_keys(root, keys)` -- pv_state_apply: a batch
  of sets and removals (a value of None: PruningState.remove, state/pruning_state.py:84-85 ->
  Trie.delete, state/trie/pruning_trie.py:683-848) in one call.  The lane of a removed key emits no
  value and opens the children it carries from the branches on its path (a leaf child as its path and
  value, an extension child as its path and child reference), so a branch left with one entry
  collapses in the build; `apply_host(db, root, items)` is the pure-Python mirror.  A removal needs
  the nodes referenced from the branches on its path in the store, where the reference decodes a
  sibling only on a collapse.  `update_state` and `build_state` keep refusing an empty value.

* `GpuStateStore.prune(keep_roots)` / `reachable(roots)` -- pv_state_store_prune: keep exactly the
  nodes some walk from a kept root can fetch by hash (csrc/pv_trie_prune.h), drop the rest --
  earlier roots, reverted batches, the duplicates apply_batch re-emits -- and shrink the buffers.
  The reference prunes by reference counts, a death row and an epoch ttl
  (state/trie/pruning_trie.py:208-230, 681; state/db/refcount_db.py); here the caller names the
  roots.  `reachable_host(db, roots)` is the pure-Python mirror of the mark.

* `sort_keys_gpu(keys)` -- pv_state_sort_device (csrc/pv_trie_sort.h): the permutation that sorts
  state keys on the device, the last of equal keys kept; `sort_keys_host(keys)` is its mirror.
  `build_state(items, device_sort=True)` and `apply_batch(root, items, device_sort=True)` upload the
  pairs in the caller's order (pv_state_build_unsorted_device, pv_state_apply_unsorted_device), and
  `apply_batch_sha256(root, items)` hashes NYM-style preimages into the key buffer on the device
  first, so no key crosses back to the host.

* `GpuStateStore.get_batch([(root, key), ...], decode=True)` -- pv_state_store_get: reads,
  PruningState.get / get_for_root_hash (state/pruning_state.py:63-77).  One lane per query walks as
  a proof does but records no node (k_trie_get), a scan lays the values out and a lane group per
  value gathers them (k_trie_get_copy): the values alone cross to the host, not the proofs around
  them.  `get_host(db, root, key, decode)` is the pure-Python mirror.  `get_for_root_hash_batch`
  still goes through the proofs.  plenum_gpu.pruning_state.GpuPruningState is the reference's State
  interface (set / remove / headHash / commit / revertToHead / get) over a store.

Out of scope: generate_state_proof_for_keys_with_prefix, as_dict and
get_all_leaves_for_root_hash (subtree traversals).
"""
import ctypes
import hashlib
import sys

import numpy as np

from . import _native as nat
from .state_proofs import (BLANK_NODE, BLANK_ROOT, PV_SP_MALFORMED, PV_SP_NODE_MISSING, PV_SP_OK, _length_prefix,
                           _nibble, _p, _rlp_item, rlp_encode, rlp_split_list)

PV_SP_PATH_TOO_LONG = 4   # include/plenum_verify.h

# Size dispatch of state_root_batch, as state_proofs.GPU_MIN_ITEMS (not a fallback): below this
# many pairs the Python mirror is quicker than one pv_state_build call.
BUILD_GPU_MIN_ITEMS = 160


def rlp_decode(data):
    """one RLP item -> bytes or nested lists (lengths as state/util/fast_rlp.py:47-71,
    each checked against the enclosing end); ValueError when it overruns or bytes are left"""
    data = bytes(data)

    def item(pos, lim):
        it = _rlp_item(data, pos, lim)
        if it is None:
            raise ValueError('RLP item overruns its enclosing item')
        is_list, pb, pe = it
        if not is_list:
            return data[pb:pe], pe
        out = []
        while pb < pe:
            x, pb = item(pb, pe)
            out.append(x)
        return out, pe
    x, end = item(0, len(data))
    if end != len(data):
        raise ValueError('bytes after the RLP item')
    return x


def serialize_nodes(nodes):
    """rlp(list of nodes) from the nodes' own RLP, walk order in, reverse order out"""
    body = b''.join(reversed(nodes))
    return _length_prefix(len(body), 192) + body


def walk_host(db, root, key, max_nodes=None):
    """sg_walk of csrc/pv_trie_store.h in Python over `db` = {sha3(node RLP): node RLP}.

    -> (status, nodes, value, proof, val_rel): the RLP of every node fetched by hash in
    walk order (root first; inline nodes are walked in place and are not among them), the
    value as the trie stores it (b'' = proven absent), the serialized proof (reverse walk
    order; None unless status is PV_SP_OK) and the value's offset in it (the value lies in
    the terminal node, which is serialized first).  With max_nodes, a walk of more hashed
    nodes is PV_SP_PATH_TOO_LONG and `nodes` holds all of them (the true count)."""
    root, key = bytes(root), bytes(key)
    if root == BLANK_ROOT:
        return PV_SP_OK, [], b'', b'\xc0', 0
    blob = db.get(root)
    if blob is None:
        return PV_SP_NODE_MISSING, [], b'', None, 0
    nodes = [blob]

    def end(status, value=b'', at=0):
        if status == PV_SP_OK and max_nodes is not None and len(nodes) > max_nodes:
            status = PV_SP_PATH_TOO_LONG
        if status != PV_SP_OK:
            return status, nodes, b'', None, 0
        proof = serialize_nodes(nodes)
        head = len(proof) - sum(len(n) for n in nodes)
        return status, nodes, value, proof, (head + at if value else 0)

    cb, ce = 0, len(blob)
    total, nib = 2 * len(key), 0
    for _ in range(total + 1):
        head = _rlp_item(blob, cb, ce)
        if head is None or not head[0] or head[2] != ce:
            return end(PV_SP_MALFORMED)
        items, pos = [], head[1]
        while pos < ce:
            if len(items) == 17:
                return end(PV_SP_MALFORMED)
            it = _rlp_item(blob, pos, ce)
            if it is None:
                return end(PV_SP_MALFORMED)
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
                return end(PV_SP_MALFORMED)
            flags = blob[i0b] >> 4
            odd = flags & 1
            pn = 2 * (i0e - i0b - 1) + odd
            skip = 2 - odd
            left = total - nib
            leaf = bool(flags & 2)
            if not leaf and pn == 0:
                return end(PV_SP_MALFORMED)
            match = (pn == left) if leaf else (pn <= left)
            if match:
                match = all(_nibble(blob, i0b, skip + i) == _nibble(key, 0, nib + i) for i in range(pn))
            if not match:
                return end(PV_SP_OK)       # blank: proven absent
            ref = items[1]
            if leaf:
                done = True
            else:
                nib += pn
        else:
            return end(PV_SP_MALFORMED)
        rs, rl, rb, re = ref
        if done:
            if rl:
                return end(PV_SP_MALFORMED)
            return end(PV_SP_OK, bytes(blob[rb:re]), rb)
        if rl:                              # an inline node: its RLP is the item itself
            cb, ce = rs, re
            continue
        if re == rb:
            return end(PV_SP_OK)           # blank: proven absent
        if re - rb != 32:
            return end(PV_SP_NODE_MISSING)
        nxt = db.get(bytes(blob[rb:re]))
        if nxt is None:
            return end(PV_SP_NODE_MISSING)
        blob = nxt
        nodes.append(blob)
        cb, ce = 0, len(blob)
    return end(PV_SP_MALFORMED)


def decode_value_host(value):
    """tg_decode of csrc/pv_trie_get.h: the stored value -> the payload of its first item, or None
    unless the value is one RLP list that fills it and whose first item is a string"""
    head = _rlp_item(value, 0, len(value))
    if head is None or not head[0] or head[2] != len(value):
        return None
    first = _rlp_item(value, head[1], head[2])
    if first is None or first[0]:
        return None
    return bytes(value[first[1]:first[2]])


def get_host(db, root, key, decode=True):
    """tg_get of csrc/pv_trie_get.h in Python over `db` = {sha3(node RLP): node RLP} -> (status,
    found, value): the walk of walk_host without a bound on the nodes; found is False for an
    absent key, a blank root and every status but PV_SP_OK; with decode the value is the payload
    PruningState.get_decoded returns, and a stored value of another form is PV_SP_MALFORMED."""
    st, _, value, _, _ = walk_host(db, root, key)
    if st != PV_SP_OK or not value:
        return st, False, b''
    if not decode:
        return PV_SP_OK, True, value
    payload = decode_value_host(value)
    if payload is None:
        return PV_SP_MALFORMED, False, b''
    return PV_SP_OK, True, payload


def _node_children(blob, cb, ce, depth=0):
    """The mark rule of csrc/pv_trie_prune.h for the node RLP blob[cb:ce] -> (the 32-byte child
    references in item order, through inline nodes; the deepest inline nesting met).  A node that
    does not parse at its own level has no children."""
    head = _rlp_item(blob, cb, ce)
    if head is None or not head[0] or head[2] != ce:
        return [], depth
    items, pos = [], head[1]
    while pos < ce:
        if len(items) == 17:
            return [], depth
        it = _rlp_item(blob, pos, ce)
        if it is None:
            return [], depth
        items.append((pos,) + it)          # (start, is_list, payload begin, payload end)
        pos = it[2]
    if len(items) == 2:
        _, i0l, i0b, i0e = items[0]
        if i0l or i0e == i0b:
            return [], depth
        flags = blob[i0b] >> 4
        if flags & 2 or 2 * (i0e - i0b - 1) + (flags & 1) == 0:
            return [], depth               # a leaf's item 1 is its value; an extension over no nibble
        children = [items[1]]
    elif len(items) == 17:
        children = items[:16]              # item 16 is a value, never a reference
    else:
        return [], depth
    refs, deepest = [], depth
    for start, is_list, pb, pe in children:
        if is_list:                        # an inline node, visited in place
            r, d = _node_children(blob, start, pe, depth + 1)
            refs += r
            deepest = max(deepest, d)
        elif pe - pb == 32:
            refs.append(bytes(blob[pb:pe]))
    return refs, deepest


def reachable_host(db, roots):
    """The mark of csrc/pv_trie_prune.h in Python over `db` = {sha3(node RLP): node RLP}: the nodes
    some walk_host from one of `roots` can fetch by hash -> (set of their digests, n_missing: the
    child references of those nodes that db does not hold, each occurrence counted, [status per
    root]: PV_SP_OK, or PV_SP_NODE_MISSING for a non-blank root db does not hold, the deepest inline
    nesting met).  The blank root reaches nothing.  A 32-byte value is never followed."""
    kept, queue, statuses = set(), [], []
    for root in roots:
        root = bytes(root)
        if root == BLANK_ROOT or root in db:
            statuses.append(PV_SP_OK)
            if root != BLANK_ROOT and root not in kept:
                kept.add(root)
                queue.append(root)
        else:
            statuses.append(PV_SP_NODE_MISSING)
    n_missing, deepest, at = 0, 0, 0
    while at < len(queue):
        blob = db[queue[at]]
        at += 1
        refs, d = _node_children(blob, 0, len(blob))
        deepest = max(deepest, d)
        for h in refs:
            if h not in db:
                n_missing += 1
            elif h not in kept:
                kept.add(h)
                queue.append(h)
    return kept, n_missing, statuses, deepest


def _hex_prefix(nibbles, leaf):
    """pack_nibbles (state/trie/pruning_trie.py): flag nibble 2 = leaf, 1 = odd length"""
    flags = (2 if leaf else 0) + (len(nibbles) & 1)
    nib = ([flags] if len(nibbles) & 1 else [flags, 0]) + list(nibbles)
    return bytes(16 * nib[i] + nib[i + 1] for i in range(0, len(nib), 2))


def _pairs(items):
    """(key, raw value) pairs -> sorted [(key, rlp([value]))], the last of equal keys kept"""
    last = {}
    for key, value in items:
        key = key.encode() if isinstance(key, str) else bytes(key)
        value = value.encode() if isinstance(value, str) else bytes(value)
        if not value:
            raise ValueError('an empty value removes a key; a build takes values only')
        last[key] = rlp_encode([value])
    return sorted(last.items())


def build_encoded_host(pairs):
    """The build of csrc/pv_trie_build.h in Python over sorted distinct (key, encoded value)
    pairs -> (root, {sha3(node RLP): node RLP}): the nodes of >= 32 bytes and the root node.
    A run of keys that share `depth` nibbles is one node: a leaf for one key, else the branch
    at the depth where the run splits, under an extension if that is deeper than `depth`."""
    db = {}
    keys = [[n for b in k for n in (b >> 4, b & 15)] for k, _ in pairs]

    def ref(node, root=False):
        enc = rlp_encode(node)
        if len(enc) < 32 and not root:
            return node
        h = hashlib.sha3_256(enc).digest()
        db[h] = enc
        return h

    def node_of(lo, hi, depth):
        if hi - lo == 1:
            return [_hex_prefix(keys[lo][depth:], True), pairs[lo][1]]
        first, last = keys[lo], keys[hi - 1]     # sorted: the run's common prefix is theirs
        d = depth
        while d < len(first) and d < len(last) and first[d] == last[d]:
            d += 1
        if d > depth:
            return [_hex_prefix(first[depth:d], False), ref(node_of(lo, hi, d))]
        slots, value = [b''] * 16, b''
        if len(first) == depth:                  # the key that is the run's prefix: the value slot
            value = pairs[lo][1]
            lo += 1
        while lo < hi:
            nib, end = keys[lo][depth], lo
            while end < hi and keys[end][depth] == nib:
                end += 1
            slots[nib] = ref(node_of(lo, end, depth + 1))
            lo = end
        return slots + [value]

    if not pairs:
        return BLANK_ROOT, db
    # node_of recurses once per trie level, at most 2 * key length + 1 deep: raise the
    # interpreter's limit for this call only when keys of hundreds of bytes need it
    limit, need = sys.getrecursionlimit(), 2 * max(len(k) for k in keys) + 100
    if limit < need:
        sys.setrecursionlimit(need)
    try:
        return ref(node_of(0, len(pairs), 0), root=True), db
    finally:
        if limit < need:
            sys.setrecursionlimit(limit)


def build_host(items):
    """(key, raw value) pairs in any order, the last of equal keys wins -> (root, {hash: node
    RLP}): what PruningState.set of every pair leaves reachable from headHash.  The mirror of
    pv_state_build, used by the CPU tests and below BUILD_GPU_MIN_ITEMS."""
    return build_encoded_host(_pairs(items))


# ------------------------------------------------------------------ sets onto a committed root
ITEM_VALUE, ITEM_SUBTREE = 0, 1   # csrc/pv_trie_update.h: TU_VALUE, TU_SUBTREE


class _Raw(bytes):
    """RLP that is already encoded: a child reference carried as it is"""


def _rlp_raw(item):
    if isinstance(item, _Raw):
        return bytes(item)
    if isinstance(item, (list, tuple)):
        body = b''.join(_rlp_raw(x) for x in item)
        return _length_prefix(len(body), 192) + body
    return rlp_encode(item)


def _node_fields(blob, cb, ce):
    """the 2 or 17 items of the node RLP blob[cb:ce] -> [(start, is_list, payload begin, payload
    end)], or None for anything else (tu_fields of csrc/pv_trie_update.h)"""
    head = _rlp_item(blob, cb, ce)
    if head is None or not head[0] or head[2] != ce:
        return None
    items, pos = [], head[1]
    while pos < ce:
        if len(items) == 17:
            return None
        it = _rlp_item(blob, pos, ce)
        if it is None:
            return None
        items.append((pos,) + it)
        pos = it[2]
    return items if len(items) in (2, 17) else None


def _child_ref(blob, it):
    """a child reference -> (status, b'' for blank or the reference's bytes as they are): 0xa0 and
    32 hash bytes, or the RLP of an inline node under 32 bytes"""
    start, is_list, pb, pe = it
    if is_list:
        return (PV_SP_OK, bytes(blob[start:pe])) if pe - start < 32 else (PV_SP_MALFORMED, b'')
    if pe == pb:
        return PV_SP_OK, b''
    if pe - pb != 32 or pb != start + 1:
        return PV_SP_NODE_MISSING, b''
    return PV_SP_OK, bytes(blob[start:pe])


def _cmp_path(path, rest):
    """Q = prefix + path against X = prefix + rest -> 0: equal, 1: Q a proper prefix of X, 2: X a
    proper prefix of Q, 3: Q < X at a nibble, 4: X < Q at a nibble"""
    m = 0
    while m < len(path) and m < len(rest) and path[m] == rest[m]:
        m += 1
    if m == len(path):
        return 0 if m == len(rest) else 1
    if m == len(rest):
        return 2
    return 3 if path[m] < rest[m] else 4


def _lcp(a, b):
    m = 0
    while m < len(a) and m < len(b) and a[m] == b[m]:
        m += 1
    return m


def _open_ref(db, blob, it, ref):
    """tu_open of csrc/pv_trie_update.h: the non-blank child reference `ref` (item `it` of the node
    in `blob`) -> (status, path nibbles, kind, payload) of the item it stands for once its node is
    opened.  A branch: no nibbles and the reference as it is.  A leaf: its path and value.  An
    extension: its path and its child reference."""
    if it[1]:                                           # an inline node, read in place
        node, cb, ce = blob, it[0], it[3]
    else:
        node = db.get(ref[1:])
        if node is None:
            return PV_SP_NODE_MISSING, [], 0, b''
        cb, ce = 0, len(node)
    f = _node_fields(node, cb, ce)
    if f is None:
        return PV_SP_MALFORMED, [], 0, b''
    if len(f) == 17:
        return PV_SP_OK, [], ITEM_SUBTREE, ref
    _, pl, pb, pe = f[0]
    if pl or pe == pb:
        return PV_SP_MALFORMED, [], 0, b''
    flags = node[pb] >> 4
    odd = flags & 1
    path = [_nibble(node, pb, 2 - odd + i) for i in range(2 * (pe - pb - 1) + odd)]
    if flags & 2:
        _, vl, vb, ve = f[1]
        if vl or ve == vb:
            return PV_SP_MALFORMED, [], 0, b''
        return PV_SP_OK, path, ITEM_VALUE, bytes(node[vb:ve])
    if not path:
        return PV_SP_MALFORMED, [], 0, b''
    st, child = _child_ref(node, f[1])
    if st != PV_SP_OK or not child:
        return st or PV_SP_MALFORMED, [], 0, b''
    return PV_SP_OK, path, ITEM_SUBTREE, child


def _merge_key(db, root, keys, j, value):
    """The walk of batch key j (tu_walk of csrc/pv_trie_update.h) -> (status, its items in order):
    the old trie's values and subtrees it carries before itself, its own VALUE, those after.
    An empty `value` removes the key (apply_encoded_host only): no VALUE of its own, and every
    child reference carried from a branch slot is opened (_open_ref)."""
    remove = not value
    k = keys[j]
    kp = keys[j - 1] if j else None
    lp = _lcp(kp, k) if j else -1
    ln = _lcp(keys[j + 1], k) if j + 1 < len(keys) else -1
    before, after = [], []
    blob = db.get(root)
    if blob is None:
        return PV_SP_NODE_MISSING, []
    cb, ce, depth = 0, len(blob), 0
    for _ in range(len(k) + 1):
        f = _node_fields(blob, cb, ce)
        if f is None:
            return PV_SP_MALFORMED, []
        first, last = lp < depth, ln < depth
        if len(f) == 17:
            _, vl, vb, ve = f[16]
            if vl:
                return PV_SP_MALFORMED, []
            if ve > vb and first and len(k) != depth:
                before.append((k[:depth], ITEM_VALUE, bytes(blob[vb:ve])))
            s = k[depth] if len(k) > depth else -1
            s_prev = kp[depth] if not first and len(kp) > depth else -1
            group = []
            for t in list(range(s_prev + 1, s)) + (list(range(s + 1, 16)) if last else []):
                st, ref = _child_ref(blob, f[t])
                if st != PV_SP_OK:
                    return st, []
                if ref:
                    item = (k[:depth] + [t], ITEM_SUBTREE, ref)
                    if remove:
                        st, path, kind, payload = _open_ref(db, blob, f[t], ref)
                        if st != PV_SP_OK:
                            return st, []
                        item = (item[0] + path, kind, payload)
                    (before if t < s else group).append(item)
            if group:
                after.append(group)
            if s < 0:
                break
            nxt = f[s]
            depth += 1
        else:
            _, pl, pb, pe = f[0]
            if pl or pe == pb:
                return PV_SP_MALFORMED, []
            flags = blob[pb] >> 4
            odd, leaf = flags & 1, bool(flags & 2)
            pn = 2 * (pe - pb - 1) + odd
            if not leaf and pn == 0:
                return PV_SP_MALFORMED, []
            path = [_nibble(blob, pb, 2 - odd + i) for i in range(pn)]
            c = _cmp_path(path, k[depth:])
            if leaf:
                _, vl, vb, ve = f[1]
                if vl or ve == vb:
                    return PV_SP_MALFORMED, []
            if leaf and c == 0:
                break                                   # overwritten
            if not leaf and c in (0, 1):                # dissolved: its nibbles are the key's
                nxt = f[1]
                depth += pn
            else:
                if leaf:
                    item = (k[:depth] + path, ITEM_VALUE, bytes(blob[vb:ve]))
                else:
                    st, ref = _child_ref(blob, f[1])
                    if st != PV_SP_OK or not ref:
                        return st or PV_SP_MALFORMED, []
                    item = (k[:depth] + path, ITEM_SUBTREE, ref)
                if c in (1, 3):
                    if first or _cmp_path(path, kp[depth:]) in (2, 4):
                        before.append(item)
                elif last:
                    after.append([item])
                break
        st, ref = _child_ref(blob, nxt)
        if st != PV_SP_OK:
            return st, []
        if not ref:
            if len(f) == 2:
                return PV_SP_MALFORMED, []              # an extension over nothing
            break
        if nxt[1]:                                      # an inline node, walked in place
            cb, ce = nxt[0], nxt[3]
        else:
            blob = db.get(ref[1:])
            if blob is None:
                return PV_SP_NODE_MISSING, []
            cb, ce = 0, len(blob)
    else:
        return PV_SP_MALFORMED, []                      # the step bound ran out
    own = [] if remove else [(k, ITEM_VALUE, value)]
    return PV_SP_OK, before + own + [it for g in reversed(after) for it in g]


def merge_host(db, root, pairs):
    """The merge of csrc/pv_trie_update.h over `db` = {hash: node RLP}: the trie at `root` and
    sorted distinct (key, encoded value) pairs -> (status, index of the first refused key,
    [(nibbles, kind, payload)]), one strictly increasing list that holds every new value, every
    old value outside the batch and, as a SUBTREE, the reference of every child no batch key
    enters.  No sort: key j's items follow key j - 1's."""
    keys = [[n for b in k for n in (b >> 4, b & 15)] for k, _ in pairs]
    out = []
    for j in range(len(pairs)):
        st, items = _merge_key(db, root, keys, j, pairs[j][1])
        if st != PV_SP_OK:
            return st, j, []
        out += items
    return PV_SP_OK, 0, out


def build_items_host(items):
    """build_encoded_host over merged items [(nibbles, kind, payload)]: a SUBTREE item with no
    nibble left below its slot is its payload, the reference itself; with nibbles left it is an
    extension over them.  It is never a branch value.  -> (root, {hash: node RLP})"""
    db = {}
    keys = [it[0] for it in items]

    def ref(node, root=False):
        if isinstance(node, _Raw):
            return node
        enc = _rlp_raw(node)
        if len(enc) < 32 and not root:
            return _Raw(enc)
        h = hashlib.sha3_256(enc).digest()
        db[h] = enc
        return h

    def node_of(lo, hi, depth):
        if hi - lo == 1:
            _, kind, payload = items[lo]
            if kind == ITEM_VALUE:
                return [_hex_prefix(keys[lo][depth:], True), payload]
            if len(keys[lo]) == depth:
                return _Raw(payload)
            return [_hex_prefix(keys[lo][depth:], False), _Raw(payload)]
        first, last = keys[lo], keys[hi - 1]
        d = depth
        while d < len(first) and d < len(last) and first[d] == last[d]:
            d += 1
        if d > depth:
            return [_hex_prefix(first[depth:d], False), ref(node_of(lo, hi, d))]
        slots, value = [b''] * 16, b''
        if len(first) == depth:
            value = items[lo][2]
            lo += 1
        while lo < hi:
            nib, end = keys[lo][depth], lo
            while end < hi and keys[end][depth] == nib:
                end += 1
            slots[nib] = ref(node_of(lo, end, depth + 1))
            lo = end
        return slots + [value]

    limit, need = sys.getrecursionlimit(), max(len(k) for k in keys) + 100
    if limit < need:
        sys.setrecursionlimit(need)
    try:
        return ref(node_of(0, len(items), 0), root=True), db
    finally:
        if limit < need:
            sys.setrecursionlimit(limit)


def update_encoded_host(db, root, pairs):
    """pv_state_update in Python: sorted distinct (key, encoded value) pairs set into the trie at
    `root`, whose nodes are in `db` = {hash: node RLP} -> (new root, {hash: node RLP} of the nodes
    the update emits: every re-encoded node, none from inside an untouched subtree).  KeyError
    when the root or a node on a batch key's path is not in db, ValueError for a malformed one."""
    root = bytes(root)
    if not pairs:
        return root, {}
    if root == BLANK_ROOT:
        return build_encoded_host(pairs)
    st, j, items = merge_host(db, root, pairs)
    if st == PV_SP_NODE_MISSING:
        raise KeyError('key {}: the root or a node on its path is not in the store'.format(j))
    if st != PV_SP_OK:
        raise ValueError('key {}: a node on its path is not a well-formed trie node'.format(j))
    return build_items_host(items)


def update_host(db, root, items):
    """(key, raw value) pairs in any order, the last of equal keys wins, set into the trie at
    `root` as PruningState.set does -> (new root, emitted nodes)"""
    return update_encoded_host(db, root, _pairs(items))


# ------------------------------------------------------------------ sets and removals
def _ops(items):
    """(key, raw value or None) pairs -> sorted [(key, rlp([value]) or b'' for a removal)], the last
    of equal keys kept: a later removal beats an earlier set and the other way round"""
    last = {}
    for key, value in items:
        key = key.encode() if isinstance(key, str) else bytes(key)
        if value is None:
            last[key] = b''
            continue
        value = value.encode() if isinstance(value, str) else bytes(value)
        if not value:
            raise ValueError('an empty value is no value; None removes a key')
        last[key] = rlp_encode([value])
    return sorted(last.items())


def apply_encoded_host(db, root, pairs):
    """pv_state_apply in Python: sorted distinct (key, encoded value) pairs, an empty encoded value
    a removal, applied to the trie at `root` whose nodes are in `db` -> (new root, {hash: node RLP}
    of the emitted nodes).  The merge of update_encoded_host with one rule added: the walk of a
    removed key emits no value and opens the children it carries (_merge_key).  KeyError when the
    root, a node on a key's path or a child referenced from a branch on a removed key's path is not
    in db, ValueError for a malformed one."""
    root = bytes(root)
    if not pairs:
        return root, {}
    if root == BLANK_ROOT:                              # removals of nothing are dropped
        return build_encoded_host([p for p in pairs if p[1]])
    st, j, items = merge_host(db, root, pairs)
    if st == PV_SP_NODE_MISSING:
        raise KeyError('key {}: the root or a node on its path is not in the store'.format(j))
    if st != PV_SP_OK:
        raise ValueError('key {}: a node on its path is not a well-formed trie node'.format(j))
    if not items:
        return BLANK_ROOT, {}
    return build_items_host(items)


def apply_host(db, root, items):
    """(key, raw value or None) pairs in any order, the last of equal keys wins, applied to the trie
    at `root` as PruningState.set and PruningState.remove (None) do -> (new root, emitted nodes)"""
    return apply_encoded_host(db, root, _ops(items))


def _root_ptr(root):
    return root.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _build_gpu(pairs, store_id, want_nodes=False):
    """pv_state_build over (key, encoded value) pairs -> (root, n_nodes, n_bytes[, blob, off, digests])"""
    nat.ensure_init()
    lib = nat.load()
    n = len(pairs)
    kblob, koff = nat.pack_messages([k for k, _ in pairs])
    vblob, voff = nat.pack_messages([v for _, v in pairs])
    root = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(blob, bcap, off, ncap, dig):
        return lib.pv_state_build(_p(kblob), _p(koff), _p(vblob), _p(voff), n, store_id, _root_ptr(root), ctypes.byref(nn),
                                  ctypes.byref(nb), _p(blob), bcap, _p(off), ncap, _p(dig))
    if not want_nodes:
        nat._check('pv_state_build', call(None, 0, None, 0, None))
        return root.tobytes(), nn.value, nb.value
    if store_id != -1:
        raise ValueError('the sizing call and the retry would insert twice')
    nat._check('pv_state_build', call(None, 0, None, 0, None))   # sizes
    blob = np.zeros(max(nb.value, 1), np.uint8)
    off = np.zeros(nn.value + 1, np.uint64)
    dig = np.zeros((max(nn.value, 1), 32), np.uint8)
    nat._check('pv_state_build', call(blob, nb.value, off, nn.value, dig))
    return root.tobytes(), nn.value, nb.value, blob[:nb.value], off, dig[:nn.value]


def _update_gpu(store_id, root, pairs, insert=True, want_nodes=False, entry='pv_state_update'):
    """pv_state_update (or, with entry, pv_state_apply: an empty encoded value removes its key) over (key,
    encoded value) pairs -> (new root, n_nodes, n_bytes[, blob, off, digests]).
    With want_nodes the sizing call computes only and the retry inserts, so nothing is inserted twice."""
    nat.ensure_init()
    lib = nat.load()
    fn = getattr(lib, entry)
    n = len(pairs)
    kblob, koff = nat.pack_messages([k for k, _ in pairs])
    vblob, voff = nat.pack_messages([v for _, v in pairs])
    old = np.frombuffer(bytes(root), np.uint8).copy()
    new = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(ins, blob, bcap, off, ncap, dig):
        return fn(store_id, _root_ptr(old), _p(kblob), _p(koff), _p(vblob), _p(voff), n, int(ins), _root_ptr(new),
                  ctypes.byref(nn), ctypes.byref(nb), _p(blob), bcap, _p(off), ncap, _p(dig))
    if not want_nodes:
        nat._check(entry, call(insert, None, 0, None, 0, None))
        return new.tobytes(), nn.value, nb.value
    nat._check(entry, call(False, None, 0, None, 0, None))   # sizes
    blob = np.zeros(max(nb.value, 1), np.uint8)
    off = np.zeros(nn.value + 1, np.uint64)
    dig = np.zeros((max(nn.value, 1), 32), np.uint8)
    nat._check(entry, call(insert, blob, nb.value, off, nn.value, dig))
    return new.tobytes(), nn.value, nb.value, blob[:nb.value], off, dig[:nn.value]


def _apply_gpu(store_id, root, pairs, insert=True, want_nodes=False):
    """pv_state_apply over (key, encoded value) pairs, an empty encoded value a removal"""
    return _update_gpu(store_id, root, pairs, insert, want_nodes, entry='pv_state_apply')


# ------------------------------------------------------------------ keys sorted on the device
SORT_TILE = 2048            # csrc/pv_trie_sort.h: TS_TILE, the scatter kernel's items per block
SORT_MAX_KEY_BYTES = 1024   # TS_MAX_KEY_BYTES: longer keys are refused by the device sort


def sort_keys_host(keys):
    """The mirror of pv_state_sort_device: perm (uint32) with perm[k] = the index of the k-th key in
    bytewise order, a proper prefix first; of equal keys the last occurrence stays."""
    last = {}
    for i, key in enumerate(keys):
        last[bytes(key)] = i
    return np.array([last[k] for k in sorted(last)], np.uint32)


def _encoded_in_order(items, removals):
    """(key, raw value or None) pairs -> [(key, rlp([value]) or b'' for a removal)] in the caller's
    order, every occurrence kept: what the fused forms sort and deduplicate on the device"""
    out = []
    for key, value in items:
        key = key.encode() if isinstance(key, str) else bytes(key)
        if value is None and removals:
            out.append((key, b''))
            continue
        value = value.encode() if isinstance(value, str) else bytes(value)
        if not value:
            raise ValueError('an empty value is no value; None removes a key' if removals else
                             'an empty value removes a key; a build takes values only')
        out.append((key, rlp_encode([value])))
    return out


def _upload(arr, device):
    """a numpy array as a device tensor of its bytes plus the 16 spare bytes the kernels may read"""
    import torch
    raw = np.concatenate([np.ascontiguousarray(arr).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])
    return torch.from_numpy(raw).to(torch.device('cuda', device))


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


def sort_keys_gpu(keys, device=0):
    """pv_state_sort_device over `keys` (uploaded as they are) -> perm as sort_keys_host gives it"""
    nat.ensure_init()
    keys = [bytes(k) for k in keys]
    n = len(keys)
    if n == 0:
        return np.zeros(0, np.uint32)
    import torch
    kblob, koff = nat.pack_messages(keys)
    d_kb, d_ko = _upload(kblob, device), _upload(koff, device)
    perm = torch.zeros(4 * n, dtype=torch.uint8, device=d_kb.device)
    kept = ctypes.c_uint64(0)
    torch.cuda.synchronize(d_kb.device)   # the library runs on its own stream
    nat._check('pv_state_sort_device',
               nat.load().pv_state_sort_device(_dp(d_kb), _dp(d_ko), n, _dp(perm), ctypes.byref(kept), device, None))
    return perm.cpu().numpy().view(np.uint32)[:kept.value].copy()


def _build_unsorted_gpu(pairs, store_id, device=0):
    """pv_state_build_unsorted_device over (key, encoded value) pairs in any order -> (root, n_nodes, n_bytes)"""
    nat.ensure_init()
    n = len(pairs)
    kblob, koff = nat.pack_messages([k for k, _ in pairs])
    vblob, voff = nat.pack_messages([v for _, v in pairs])
    bufs = [_upload(a, device) for a in (kblob, koff, vblob, voff)] if n else [None] * 4
    root = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    nat._check('pv_state_build_unsorted_device', nat.load().pv_state_build_unsorted_device(
        *[_dp(b) if n else None for b in bufs], n, store_id, _root_ptr(root), ctypes.byref(nn), ctypes.byref(nb),
        None, 0, None, 0, None, device, None))
    return root.tobytes(), nn.value, nb.value


def _apply_unsorted_device(store_id, root, n, d_kb, d_ko, d_vb, d_vo, insert=True):
    """pv_state_apply_unsorted_device over device tensors -> (new root, n_nodes, n_bytes)"""
    old = np.frombuffer(bytes(root), np.uint8).copy()
    new = np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    nat._check('pv_state_apply_unsorted_device', nat.load().pv_state_apply_unsorted_device(
        store_id, _root_ptr(old), _dp(d_kb), _dp(d_ko), _dp(d_vb), _dp(d_vo), n, int(insert), _root_ptr(new),
        ctypes.byref(nn), ctypes.byref(nb), None, 0, None, 0, None, None))
    return new.tobytes(), nn.value, nb.value


def _apply_unsorted_gpu(store_id, root, pairs, device=0, insert=True):
    """pv_state_apply_unsorted_device over (key, encoded value or b'') pairs in any order"""
    nat.ensure_init()
    if not pairs:
        return bytes(root), 0, 0
    kblob, koff = nat.pack_messages([k for k, _ in pairs])
    vblob, voff = nat.pack_messages([v for _, v in pairs])
    bufs = [_upload(a, device) for a in (kblob, koff, vblob, voff)]
    return _apply_unsorted_device(store_id, root, len(pairs), *bufs, insert=insert)


def state_root_batch(items):
    """The state root after PruningState.set of every (key, raw value) pair (state/pruning_state.py
    :60-61), the last of equal keys winning; no node is kept.  One pv_state_build call from
    BUILD_GPU_MIN_ITEMS pairs on, the mirror below."""
    pairs = _pairs(items)
    if len(pairs) < BUILD_GPU_MIN_ITEMS:
        return build_encoded_host(pairs)[0]
    return _build_gpu(pairs, -1)[0]


def root_hash_of(root):
    """a 32-byte root hash as it is; a decoded root node (what get_head_by_hash returns)
    RLP-encoded and hashed; the blank node -> BLANK_ROOT"""
    if isinstance(root, (bytes, bytearray, memoryview)):
        root = bytes(root)
        if root == BLANK_NODE:
            return BLANK_ROOT
        if len(root) != 32:
            raise ValueError('a root hash has 32 bytes')
        return root
    if isinstance(root, (list, tuple)):
        return hashlib.sha3_256(rlp_encode(root)).digest()
    raise TypeError('root is a 32-byte hash or a decoded root node')


class Proved:
    """The arrays of one pv_state_store_prove call."""
    __slots__ = ('status', 'node_count', 'proof_off', 'val_rel', 'val_len', 'blob')

    def proof(self, q):
        return self.blob[self.proof_off[q]:self.proof_off[q + 1]].tobytes()

    def value(self, q):
        o = int(self.proof_off[q] + self.val_rel[q])
        return self.blob[o:o + int(self.val_len[q])].tobytes()


class Got:
    """The arrays of one pv_state_store_get call."""
    __slots__ = ('status', 'found', 'val_off', 'blob')

    def value(self, q):
        """the value of query q (b'' for a present key with an empty payload), None unless found"""
        if not self.found[q]:
            return None
        return self.blob[int(self.val_off[q]):int(self.val_off[q + 1])].tobytes()

    def values(self):
        """every query's value; KeyError where the reference raises it (the root or a node on the
        path is not in the store), ValueError for a node or a stored value that is not well formed"""
        out = []
        for q in range(len(self.status)):
            st = int(self.status[q])
            if st == PV_SP_NODE_MISSING:
                raise KeyError('item {}: the root or a node on the path is not in the store'.format(q))
            if st != PV_SP_OK:
                raise ValueError('item {}: a node on the path or the stored value is not well formed'.format(q))
            out.append(self.value(q))
        return out


def group_roots(items):
    """[(root, key), ...] -> (distinct root hashes, root index per item, keys as bytes)"""
    index, roots, ridx, keys = {}, [], [], []
    for root, key in items:
        rh = root_hash_of(root)
        ridx.append(index.setdefault(rh, len(index)))
        if ridx[-1] == len(roots):
            roots.append(rh)
        keys.append(key.encode() if isinstance(key, str) else bytes(key))
    return roots, ridx, keys


class GpuStateStore:
    """A device-resident store of trie nodes keyed by their SHA3-256: append-only between two
    prune() calls, each of which keeps the nodes reachable from the roots it is given."""

    def __init__(self, device=0, node_hint=1 << 16, byte_hint=0):
        nat.ensure_init()
        self._lib = nat.load()
        self.device = device
        h = ctypes.c_int32(0)
        nat._check('pv_state_store_create', self._lib.pv_state_store_create(node_hint, byte_hint, device,
                                                                            ctypes.byref(h)))
        self._id = h.value

    def close(self):
        if self._id:
            sid, self._id = self._id, 0
            nat._check('pv_state_store_free', self._lib.pv_state_store_free(sid))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """{'n_nodes': added, 'n_unique': with a table slot, 'n_bytes', 'n_slots'}"""
        v = [ctypes.c_uint64(0) for _ in range(4)]
        nat._check('pv_state_store_info', self._lib.pv_state_store_info(self._id, *[ctypes.byref(x) for x in v]))
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes', 'n_slots'), (x.value for x in v)))

    def add_nodes(self, nodes, want_digests=False):
        """Add node RLPs (what the host trie stores under their hash on commit) -> the
        number new to the store; with want_digests -> (that, [32-byte digests])."""
        nodes = [bytes(n) for n in nodes]
        if not nodes:
            return (0, []) if want_digests else 0
        blob, off = nat.pack_messages(nodes)
        dig = np.empty((len(nodes), 32), np.uint8) if want_digests else None
        added = ctypes.c_uint64(0)
        nat._check('pv_state_store_add', self._lib.pv_state_store_add(self._id, _p(blob), _p(off), len(nodes), _p(dig),
                                                                      ctypes.byref(added)))
        if want_digests:
            return added.value, [dig[i].tobytes() for i in range(len(nodes))]
        return added.value

    def _prune(self, roots, apply, want_digests):
        roots = [root_hash_of(r) for r in roots]
        if not roots:
            raise ValueError('no root to keep: close the store instead')
        rts = np.frombuffer(b''.join(roots), np.uint8)
        status = np.zeros(len(roots), np.uint8)
        kept, nbytes, missing = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

        def call(ap, dig, cap):
            rc = self._lib.pv_state_store_prune(self._id, _p(rts), len(roots), ap, _p(status), ctypes.byref(kept),
                                                ctypes.byref(nbytes), ctypes.byref(missing), _p(dig), cap)
            if rc != 0 and (status == PV_SP_NODE_MISSING).any():
                text = self._lib.pv_last_error().decode(errors='replace')
                if 'is not in the store' in text:
                    raise KeyError(text)
            nat._check('pv_state_store_prune', rc)
        dig = None
        if want_digests or not apply:
            call(0, None, 0)                           # the sizing call
        if want_digests:
            dig = np.zeros((max(kept.value, 1), 32), np.uint8)
        if apply or want_digests:
            call(apply, dig, kept.value if want_digests else 0)
        out = {'n_kept': kept.value, 'bytes_kept': nbytes.value, 'n_missing': missing.value,
               'root_status': [int(x) for x in status]}
        if want_digests:
            out['digests'] = [dig[i].tobytes() for i in range(kept.value)]
        return out

    def reachable(self, roots, want_digests=False):
        """What a prune to `roots` (32-byte hashes or decoded root nodes, as root_hash_of takes them)
        would keep; the store is untouched (pv_state_store_prune with apply == 0) -> {'n_kept',
        'bytes_kept', 'n_missing': child references of kept nodes the store does not hold,
        'root_status': PV_SP_OK or PV_SP_NODE_MISSING per root[, 'digests': the kept nodes' in new-id
        order]}.  A root that is not in the store is reported, not refused."""
        return self._prune(roots, 0, want_digests)

    def prune(self, keep_roots, want_digests=False):
        """Keep exactly the nodes reachable from `keep_roots`, drop the rest and give the memory back
        (pv_state_store_prune) -> the dict of reachable(), after the compaction.  What the
        reference's pruning state does with reference counts on commit and revertToHead
        (state/pruning_state.py:87-102).  Keep committedHeadHash, the heads of uncommitted batches
        and every root still served to readers: proofs and updates at a kept root are unchanged,
        every other root is gone.  KeyError for a root that is not in the store (nothing is
        dropped)."""
        return self._prune(keep_roots, 1, want_digests)

    def build_state(self, items, device_sort=False):
        """Build the trie of (key, raw value) pairs on the device (pv_state_build) and insert its
        nodes -> the root hash.  Afterwards generate_state_proof(key, root, ...) and
        get_for_root_hash_batch work at that root; no host trie is involved.  With device_sort the
        pairs are uploaded in the caller's order and sorted there (pv_state_build_unsorted_device)."""
        if device_sort:
            return _build_unsorted_gpu(_encoded_in_order(items, False), self._id, self.device)[0]
        return _build_gpu(_pairs(items), self._id)[0]

    def update_state(self, root, items):
        """Set (key, raw value) pairs into the state at the committed `root` on the device
        (pv_state_update) and insert the nodes the update emits -> the new root hash: one 3PC batch
        of PruningState.set (state/pruning_state.py:60-61) and the new headHash, with rlp([v]) applied
        to each value as set does.  `root` and every earlier root stay provable.  Always on the GPU:
        the old trie's nodes live there.  KeyError when the root or a node on a key's path is not in
        the store, ValueError for a node that is no trie node."""
        try:
            return _update_gpu(self._id, root_hash_of(root), _pairs(items))[0]
        except nat.PlenumGpuError as exc:
            text = str(exc)
            if 'state update: key ' in text:
                raise (KeyError if 'is not in the store' in text else ValueError)(text) from None
            raise

    def apply_batch(self, root, items, device_sort=False):
        """Apply (key, raw value or None) pairs to the state at the committed `root` on the device
        (pv_state_apply) and insert the nodes it emits -> the new root hash: one 3PC batch of
        PruningState.set and, for a value of None, PruningState.remove (state/pruning_state.py:60-61,
        84-85), the last of equal keys winning.  Removing a key the state does not hold changes
        nothing; removing every key gives BLANK_ROOT.  `root` and every earlier root stay provable.
        KeyError when the root, a node on a key's path or a node referenced from a branch on a
        removed key's path is not in the store, ValueError for a node that is no trie node.  With
        device_sort the pairs are uploaded in the caller's order and sorted there
        (pv_state_apply_unsorted_device)."""
        try:
            if device_sort:
                return _apply_unsorted_gpu(self._id, root_hash_of(root), _encoded_in_order(items, True),
                                           self.device)[0]
            return _apply_gpu(self._id, root_hash_of(root), _ops(items))[0]
        except nat.PlenumGpuError as exc:
            text = str(exc)
            if 'state apply: key ' in text:
                raise (KeyError if 'is not in the store' in text else ValueError)(text) from None
            raise

    def apply_batch_sha256(self, root, items):
        """apply_batch for (preimage, raw value or None) pairs whose state key is sha256(preimage),
        as the domain state keys a NYM (nym_to_state_key, plenum/server/request_handlers/utils.py
        :38-39; nym_handler.py:112).  pv_sha256_batch_device hashes the preimages into a device
        buffer in request order and pv_state_apply_unsorted_device sorts and applies them there: no
        key crosses back to the host."""
        import torch
        nat.ensure_init()
        enc = _encoded_in_order(items, True)
        n = len(enc)
        if n == 0:
            return root_hash_of(root)
        pblob, poff = nat.pack_messages([k for k, _ in enc])
        vblob, voff = nat.pack_messages([v for _, v in enc])
        d_pb, d_po, d_vb, d_vo = (_upload(a, self.device) for a in (pblob, poff, vblob, voff))
        d_keys = torch.zeros(32 * n + 16, dtype=torch.uint8, device=d_pb.device)
        d_ko = _upload(32 * np.arange(n + 1, dtype=np.uint64), self.device)
        torch.cuda.synchronize(d_pb.device)   # the library runs on its own stream
        nat._check('pv_sha256_batch_device', self._lib.pv_sha256_batch_device(_dp(d_pb), _dp(d_po), n, -1, _dp(d_keys),
                                                                            self.device, None))
        try:
            return _apply_unsorted_device(self._id, root_hash_of(root), n, d_keys, d_ko, d_vb, d_vo)[0]
        except nat.PlenumGpuError as exc:
            text = str(exc)
            if 'state apply: key ' in text:
                raise (KeyError if 'is not in the store' in text else ValueError)(text) from None
            raise

    def remove_keys(self, root, keys):
        """PruningState.remove of every key (state/pruning_state.py:84-85) at the committed `root`
        -> the new root hash"""
        return self.apply_batch(root, [(k, None) for k in keys])

    def add_serialized_proof(self, data):
        """Add the nodes of a serialized proof (rlp(list of nodes)) -> the number new to the store"""
        data = bytes(data)
        ranges = rlp_split_list(data)
        if ranges is None:
            raise ValueError('not a serialized proof: not one RLP list')
        return self.add_nodes([data[b:e] for b, e in ranges if e - b > 1])   # 0x80, the blank node, is no node

    def prove(self, roots, root_idx, keys, max_nodes=None, proof_cap=None):
        """pv_state_store_prove: `roots` 32-byte hashes, root_idx per key (None: root q for
        key q) -> Proved.  max_nodes defaults to 2 * max key length + 1, the bound of any
        walk, so PV_SP_PATH_TOO_LONG cannot occur."""
        keys = [bytes(k) for k in keys]
        n = len(keys)
        out = Proved()
        out.status, out.node_count = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        out.proof_off = np.zeros(n + 1, np.uint64)
        out.val_rel, out.val_len = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        out.blob = np.zeros(0, np.uint8)
        if n == 0:
            return out
        if max_nodes is None:
            max_nodes = 2 * max(len(k) for k in keys) + 1
        rts = np.frombuffer(b''.join(bytes(r) for r in roots), np.uint8)
        ridx = None if root_idx is None else np.ascontiguousarray(root_idx, np.uint32)
        kblob, koff = nat.pack_messages(keys)
        cap = max(1 << 16, 1024 * n) if proof_cap is None else proof_cap
        for _ in range(2):
            blob = np.empty(max(cap, 1), np.uint8)
            rc = self._lib.pv_state_store_prove(self._id, _p(rts), _p(ridx), len(roots), _p(kblob), _p(koff), n,
                                                max_nodes, _p(out.status), _p(out.node_count), _p(out.proof_off),
                                                _p(out.val_rel), _p(out.val_len), _p(blob), cap)
            total = int(out.proof_off[n])
            # a capacity guessed too small: the offsets are written, the bytes are not
            if rc == 0 or proof_cap is not None or total <= cap or \
                    not self._lib.pv_last_error().startswith(b'proof_cap '):
                break
            cap = total
        nat._check('pv_state_store_prove', rc)
        out.blob = blob[:total]
        return out

    def generate_state_proofs_batch(self, items):
        """[(root, key), ...] -> per item (serialized proof, value or None), or None for an
        item whose root or a node on its path is not in the store (the read handler's
        (None, None)); one GPU call.  The value is decoded as PruningState.get_decoded does
        (state/pruning_state.py:162-163)."""
        items = list(items)
        index, roots, ridx, keys = {}, [], [], []
        for root, key in items:
            rh = root_hash_of(root)
            ridx.append(index.setdefault(rh, len(index)))
            if ridx[-1] == len(roots):
                roots.append(rh)
            keys.append(key.encode() if isinstance(key, str) else bytes(key))
        pr = self.prove(roots, ridx, keys)
        out = []
        for q in range(len(items)):
            st = int(pr.status[q])
            if st == PV_SP_NODE_MISSING:
                out.append(None)
            elif st != PV_SP_OK:
                raise ValueError('item {}: a node on the path is not a well-formed trie node'.format(q))
            else:
                out.append((pr.proof(q), rlp_decode(pr.value(q))[0] if pr.val_len[q] else None))
        return out

    def get(self, roots, root_idx, keys, decode=True, val_cap=None):
        """pv_state_store_get: `roots` 32-byte hashes, root_idx per key (None: root q for key q)
        -> Got.  The values' bytes are sized by a first call unless val_cap is given."""
        keys = [bytes(k) for k in keys]
        n = len(keys)
        out = Got()
        out.status, out.found = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        out.val_off = np.zeros(n + 1, np.uint64)
        out.blob = np.zeros(0, np.uint8)
        if n == 0:
            return out
        rts = np.frombuffer(b''.join(bytes(r) for r in roots), np.uint8)
        ridx = None if root_idx is None else np.ascontiguousarray(root_idx, np.uint32)
        kblob, koff = nat.pack_messages(keys)
        cap = max(1 << 12, 160 * n) if val_cap is None else val_cap
        for _ in range(2):
            blob = np.empty(max(cap, 1), np.uint8)
            rc = self._lib.pv_state_store_get(self._id, _p(rts), _p(ridx), len(roots), _p(kblob), _p(koff), n,
                                              int(decode), _p(out.status), _p(out.found), _p(out.val_off), _p(blob),
                                              cap)
            total = int(out.val_off[n])
            # a capacity guessed too small: the offsets are written, the bytes are not
            if rc == 0 or val_cap is not None or total <= cap or \
                    not self._lib.pv_last_error().startswith(b'val_cap '):
                break
            cap = total
        nat._check('pv_state_store_get', rc)
        out.blob = blob[:total]
        return out

    def get_batch(self, items, decode=True):
        """PruningState.get_for_root_hash (state/pruning_state.py:72-77) for [(root, key), ...] in one
        pv_state_store_get call -> the values (decoded as get_decoded does, :162-163, or with
        decode=False as the trie stores them), None for an absent key; b'' is a present key with an
        empty payload.  KeyError where the reference raises it: the root or a node on the path is
        not in the store; ValueError for a node or a stored value that is not well formed."""
        items = list(items)
        roots, ridx, keys = group_roots(items)
        got = self.get(roots, ridx, keys, decode)
        return got.values()

    def get_batch_sha256(self, root, preimages, decode=True):
        """get_batch at one root for keys that are sha256(preimage) (nym_to_state_key,
        plenum/server/request_handlers/utils.py:38-39): pv_sha256_batch_device hashes the preimages
        into the device key buffer pv_state_store_get_device walks, so no key crosses back to the
        host and only the values do."""
        import torch
        nat.ensure_init()
        preimages = [p.encode() if isinstance(p, str) else bytes(p) for p in preimages]
        n = len(preimages)
        if n == 0:
            return []
        pblob, poff = nat.pack_messages(preimages)
        d_pb, d_po = _upload(pblob, self.device), _upload(poff, self.device)
        dev = d_pb.device
        d_keys = torch.zeros(32 * n + 16, dtype=torch.uint8, device=dev)
        d_ko = _upload(32 * np.arange(n + 1, dtype=np.uint64), self.device)
        d_root = _upload(np.frombuffer(root_hash_of(root), np.uint8), self.device)
        d_ridx = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
        d_status, d_found = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
        d_voff = torch.zeros(8 * (n + 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)   # the library runs on its own stream
        nat._check('pv_sha256_batch_device', self._lib.pv_sha256_batch_device(_dp(d_pb), _dp(d_po), n, -1, _dp(d_keys),
                                                                            self.device, None))
        cap = max(1 << 12, 160 * n)
        for _ in range(2):
            d_vals = torch.zeros(cap, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            rc = self._lib.pv_state_store_get_device(self._id, _dp(d_root), _dp(d_ridx), 1, _dp(d_keys), _dp(d_ko), n,
                                                     int(decode), _dp(d_status), _dp(d_found), _dp(d_voff),
                                                     _dp(d_vals), cap, None)
            if rc == 0 or not self._lib.pv_last_error().startswith(b'val_cap '):
                break
            cap = int(d_voff.cpu().numpy().view(np.uint64)[n])
        nat._check('pv_state_store_get_device', rc)
        got = Got()
        got.status, got.found = d_status.cpu().numpy(), d_found.cpu().numpy()
        got.val_off = d_voff.cpu().numpy().view(np.uint64)
        got.blob = d_vals.cpu().numpy()[:int(got.val_off[n])]
        return got.values()

    def get_for_root_hash_batch(self, items):
        """PruningState.get_for_root_hash (state/pruning_state.py:72-77) for [(root, key), ...]:
        the decoded values, None for an absent key; KeyError for a missing root or node"""
        out = []
        for q, r in enumerate(self.generate_state_proofs_batch(items)):
            if r is None:
                raise KeyError('item {}: the root or a node on the path is not in the store'.format(q))
            out.append(r[1])
        return out

    def generate_state_proof(self, key, root, serialize=False, get_value=False):
        """PruningState.generate_state_proof for one key.  `root` is a 32-byte root hash or a
        decoded root node.  -> the proof (serialized bytes, or the list of decoded nodes,
        root last), with get_value (proof, value as the trie stores it or None).  KeyError
        where the reference raises it: the root or a node on the path is not in the store."""
        key = key.encode() if isinstance(key, str) else bytes(key)
        pr = self.prove([root_hash_of(root)], None, [key])
        st = int(pr.status[0])
        if st == PV_SP_NODE_MISSING:
            raise KeyError('the root or a node on the path is not in the store')
        if st != PV_SP_OK:
            raise ValueError('a node on the path is not a well-formed trie node')
        proof = pr.proof(0)
        if not serialize:
            proof = rlp_decode(proof)
        if not get_value:
            return proof
        return proof, (pr.value(0) if pr.val_len[0] else None)
