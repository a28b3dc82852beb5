"""Builders for the device-buffer Merkle / SHA-256 tests (tests only, no GPU
needed): the SHA-256 length x misalignment grid, request batches for a resident
tree with refused requests woven in, and the small class tables the
second-trip test expands on the device.  Expectations come from hashlib,
LevelTree (tests/_merkle_proofs.py) and a restatement of the reference
verifier's two walks; tests/test_merkle_host.py and
tests/test_merkle_proofs_host.py check all of them on the CPU."""
import hashlib

import numpy as np

import _merkle_proofs as mp

TAIL = b'\xff' * 16          # the documented minimum after the last message, and not zero
REFUSED = 0xffffffff         # PV_MP_LEN_REFUSED

# both sides of every terminator and length-field boundary of blocks 1 to 4,
# with and without the prefix byte
SHA_LENGTHS = (list(range(0, 10)) + list(range(51, 70)) + list(range(115, 134)) + list(range(179, 198)) +
               list(range(247, 262)))


def sha_grid(seed=256):
    """-> (msgs, placed): every length of SHA_LENGTHS at a start offset = 0, 1,
    2, 3 (mod 4) of the packed blob, reached by 1..3-byte filler messages;
    placed = [(message index, length, start offset mod 4)], fillers not listed"""
    rng = np.random.default_rng(seed)
    msgs, placed, cur = [], [], 0
    for ln in SHA_LENGTHS:
        for r in range(4):
            fill = (r - cur) % 4
            if fill:
                msgs.append(rng.integers(0, 256, fill, dtype=np.uint8).tobytes())
                cur += fill
            placed.append((len(msgs), ln, r))
            msgs.append(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
            cur += ln
    return msgs, placed


def last_message_batches(seed=257):
    """batches whose last message has each padding shape: the tail bytes sit
    right behind an empty message, one byte, a full first block with and without
    room for the length field, and a block boundary"""
    rng = np.random.default_rng(seed)
    head = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (3, 70, 0, 64, 129)]
    return [head + [rng.integers(0, 256, n, dtype=np.uint8).tobytes()] for n in (0, 1, 55, 56, 63, 64)]


def long_message(seed=258):
    """one message of 65 blocks"""
    return [np.random.default_rng(seed).integers(0, 256, 4097, dtype=np.uint8).tobytes()]


def pack(msgs, tail=TAIL):
    """-> (blob with `tail` behind the last message, n + 1 offsets)"""
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b''.join(msgs) + tail, np.uint8).copy(), off


def at_misalignment(blob, k, fill=0xff):
    """a copy of blob that starts k bytes past a 64-byte boundary; the bytes
    before it (which an aligned-down window reads and masks) are `fill`"""
    raw = np.full(len(blob) + 128, fill, np.uint8)
    start = (-raw.ctypes.data) % 64 + k
    view = raw[start:start + len(blob)]
    view[:] = blob
    assert view.ctypes.data % 64 == k
    return view


def sha_want(msgs, prefix):
    pre = b'' if prefix < 0 else bytes([prefix])
    return [hashlib.sha256(pre + m).digest() for m in msgs]


# ------------------------------------------------ requests for a resident tree
def _pow2_edges(n):
    out, p = set(), 1
    while p <= n + 1:
        out.update(v for v in (p - 1, p, p + 1) if 0 <= v <= n)
        p *= 2
    return sorted(out)


def path_edges(n):
    """valid (index, tree_size) at the edges: s = 1, s = n, powers of two +- 1"""
    out = []
    for s in sorted({v for v in _pow2_edges(n) if v >= 1} | {n}):
        for m in sorted({0, s - 1, s // 2} | set(_pow2_edges(s - 1))):
            out.append((m, s))
    return out


def proof_edges(n):
    """valid (first, second) at the edges: a = 0, a = b, powers of two +- 1"""
    out = []
    for b in sorted(set(_pow2_edges(n)) | {n}):
        for a in sorted({0, b} | set(_pow2_edges(b))):
            out.append((a, b))
    return out


def path_refusals(n):
    """requests pv_merkle_audit_paths_device must refuse.  The last seven are
    the 64-bit traps: four are in range once an operand is cut to 32 bits,
    2^64 - 1 is -1 to a signed compare, 2^63 is the sign bit alone"""
    return [(7, 7), (n, n), (9, 7), (n + 5, n), (0, 0), (3, 0), (0, n + 1), (n, n + 1),
            (2 ** 32, 5), (2 ** 32, n), (3, 2 ** 32 + 9), (0, 2 ** 32 + n), (2 ** 64 - 1, n), (2 ** 64 - 1, 1),
            (0, 2 ** 63)]


def proof_refusals(n):
    return [(8, 7), (1, 0), (n + 1, n), (3, n + 1), (n + 1, n + 1), (0, n + 1),
            (2 ** 32, 5), (2 ** 32, n), (3, 2 ** 32 + 9), (0, 2 ** 32 + n), (2 ** 64 - 1, n), (2 ** 64 - 1, 0),
            (1, 2 ** 63), (2 ** 63, 2 ** 63)]


def _weave(k, phase, valid, refused):
    """k requests, valid and refused alternating (request i is refused when
    i + phase is odd) -> [(a, b, is_valid)]"""
    out, iv, ir = [], 0, 0
    for i in range(k):
        if (i + phase) % 2:
            out.append(refused[ir % len(refused)] + (False,))
            ir += 1
        else:
            out.append(valid[iv % len(valid)] + (True,))
            iv += 1
    return out


def path_requests(n, k, phase, seed=6962):
    """k audit-path requests over a tree of n leaves: the edges, then random
    ones, with refused requests in every other slot"""
    rng = np.random.default_rng(seed + k)
    valid, slots = path_edges(n), (k + 1) // 2
    while len(valid) < max(slots, len(path_edges(n)) + 64):
        s = int(rng.integers(1, n + 1))
        valid.append((int(rng.integers(0, s)), s))
    valid = valid[::len(valid) // slots]     # a short batch still sees edges and random ones
    return _weave(k, phase, valid, path_refusals(n))


def proof_requests(n, k, phase, seed=6963):
    rng = np.random.default_rng(seed + k)
    valid, slots = proof_edges(n), (k + 1) // 2
    while len(valid) < max(slots, len(proof_edges(n)) + 64):
        b = int(rng.integers(1, n + 1))
        valid.append((int(rng.integers(0, b + 1)), b))
    valid = valid[::len(valid) // slots]
    return _weave(k, phase, valid, proof_refusals(n))


# ----------------------- the reference verifier's walks, with what a walk leaves
def ref_inclusion(leaf_hash, index, size, path, root):
    """MerkleVerifier._calculate_root_hash_from_audit_path and the root compare
    (ledger/merkle_verifier.py:155-238) -> (status, hash the walk reached, the
    node index a too-short walk stopped at, else 0)"""
    if index >= size:
        return mp.BAD_RANGE, leaf_hash, 0
    node, last, h, pos = index, size - 1, leaf_hash, 0
    while last:
        if pos == len(path):
            return mp.TOO_SHORT, h, node
        if node & 1:
            h, pos = mp.node(path[pos], h), pos + 1
        elif node < last:
            h, pos = mp.node(h, path[pos]), pos + 1
        node, last = node >> 1, last >> 1
    if pos < len(path):
        return mp.TOO_LONG, h, 0
    return (mp.OK if h == root else mp.ROOT_MISMATCH), h, 0


def ref_consistency(old, new, r0, r1, proof):
    """MerkleVerifier.verify_tree_consistency (:47-153) -> (status, old hash,
    new hash); the given roots when the proof is not walked"""
    if old > new:
        return mp.BAD_RANGE, r0, r1
    if old == new:
        return (mp.OK if r0 == r1 else mp.INCONSISTENT), r0, r1
    if old == 0:
        return mp.OK, r0, r1
    node, last = old - 1, new - 1
    while node & 1:
        node, last = node >> 1, last >> 1
    pos = 0
    if node:
        if not proof:
            return mp.TOO_SHORT, r0, r1
        oh = nh = proof[0]
        pos = 1
    else:
        oh = nh = r0
    while last:
        consumes = bool(node & 1) or node < last
        if consumes:
            if pos == len(proof):
                return mp.TOO_SHORT, oh, nh
            if node & 1:
                oh, nh = mp.node(proof[pos], oh), mp.node(proof[pos], nh)
            else:
                nh = mp.node(nh, proof[pos])
            pos += 1
        node, last = node >> 1, last >> 1
    if nh != r1:
        return mp.ROOT_MISMATCH, oh, nh
    if oh != r0:
        return mp.INCONSISTENT, oh, nh
    return mp.OK, oh, nh


# ------------------------------------------- class tables of the second-trip test
SMALL = 5     # leaves of the small resident tree (depth 3)


def small_tree(leaf_hashes):
    return mp.LevelTree(list(leaf_hashes[:SMALL]))


def path_classes(tree):
    """[(index, tree_size, path or None when refused, root or None)]: the 15
    valid pairs of a 5-leaf tree and 3 refused ones"""
    n = tree.size
    out = [(m, s, tree.audit_path(m, s), tree.root(s)) for s in range(1, n + 1) for m in range(s)]
    return out + [(3, 3, None, None), (0, n + 1, None, None), (2 ** 32, 3, None, None)]


def proof_classes(tree):
    """[(first, second, proof or None when refused)]: all 21 valid pairs and 2 refused"""
    n = tree.size
    out = [(a, b, tree.consistency_proof(a, b)) for b in range(n + 1) for a in range(b + 1)]
    return out + [(3, 2, None), (1, n + 1, None)]


def incl_classes(tree):
    """[((leaf_hash, index, tree_size, path, root), (status, computed, stop))]:
    the valid proofs, then wrong root, too short, too long, bad range"""
    n = tree.size
    lh = tree.lv[0]
    items = [(lh[m], m, s, tree.audit_path(m, s), tree.root(s)) for s in range(1, n + 1) for m in range(s)]
    items.append((lh[1], 1, n, tree.audit_path(1, n), tree.root(n - 1)))
    items.append((lh[3], 3, n, tree.audit_path(3, n)[:1], tree.root(n)))
    items.append((lh[3], 3, 4, tree.audit_path(3, 4) + [lh[0]], tree.root(4)))
    items.append((lh[4], n, n, tree.audit_path(4, n), tree.root(n)))
    return [(it, ref_inclusion(*it)) for it in items]


def cons_classes(tree):
    """[((old, new, old_root, new_root, proof), (status, old computed, new
    computed))]: the valid proofs, then wrong new root, too short, bad range,
    inconsistent old root"""
    n = tree.size
    root = lambda s: tree.root(s) if s else hashlib.sha256(b'').digest()   # noqa: E731
    items = [(a, b, root(a), root(b), tree.consistency_proof(a, b)) for b in range(n + 1) for a in range(b + 1)]
    items.append((3, n, root(3), root(4), tree.consistency_proof(3, n)))
    items.append((3, n, root(3), root(n), tree.consistency_proof(3, n)[:-1]))
    items.append((4, 3, root(4), root(3), tree.consistency_proof(3, 4)))
    items.append((3, n, root(2), root(n), tree.consistency_proof(3, n)))
    return [(it, ref_consistency(*it)) for it in items]
