"""Golden audit paths, consistency proofs and verifier verdicts of the reference
ledger (ledger/compact_merkle_tree.py CompactMerkleTree.inclusion_proof /
consistency_proof / merkle_tree_hash, ledger/merkle_verifier.py MerkleVerifier)
over the 1,030 leaves of tests/golden/merkle.json.  Test infrastructure only:
it runs where a checkout of the reference is available and writes
tests/golden/merkle_proofs.json.

    REFERENCE_DIR=<reference checkout> python tools/gen_merkle_proofs_golden.py

Two properties of the reference are worked around here, not there:
CompactMerkleTree.extend does not write the hash store, so the tree is filled
with append; MemoryHashStore.writeNode keeps the whole (start, height, hash)
tuple, so a subclass keeps the hash alone.
"""
import base64
import hashlib
import json
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if 'REFERENCE_DIR' not in os.environ:
    sys.exit('set REFERENCE_DIR to a checkout of the reference (the directory that holds ledger/)')
sys.path[:0] = [os.path.join(REPO, 'oracle', 'shims'), os.environ['REFERENCE_DIR']]

from ledger.compact_merkle_tree import CompactMerkleTree  # noqa: E402
from ledger.hash_stores.memory_hash_store import MemoryHashStore  # noqa: E402
from ledger.merkle_verifier import MerkleVerifier  # noqa: E402
from ledger.tree_hasher import TreeHasher  # noqa: E402
from ledger.util import STH  # noqa: E402

FULL_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 70]
SPREAD_SIZES = [127, 128, 129, 513, 777, 1000, 1030]


class HashOnlyStore(MemoryHashStore):
    def writeNode(self, node):
        self._nodes.append(node[2])


def spread(s):
    """16 leaf indices of a tree of s leaves: first, last, around each power of two"""
    want = [0, s - 1]
    p = 1
    while p < s:
        want += [p - 1, p, p + 1]
        p *= 2
    seen = []
    for m in want:
        if 0 <= m < s and m not in seen:
            seen.append(m)
    keep = seen[:2] + seen[2:][-14:]
    return sorted(keep)


def outcome(fn, *args):
    try:
        assert fn(*args) is True
        return None, None
    except Exception as e:   # noqa: BLE001  (the class is what is recorded)
        return type(e).__name__, str(e)


def flip(h, bit):
    b = bytearray(h)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def main():
    with open(os.path.join(REPO, 'tests', 'golden', 'merkle.json')) as fh:
        leaves = [bytes.fromhex(x) for x in json.load(fh)['leaves']]
    n = len(leaves)
    hasher = TreeHasher()
    tree = CompactMerkleTree(hasher=hasher, hashStore=HashOnlyStore())
    for leaf in leaves:
        tree.append(leaf)
    assert tree.tree_size == n == 1030
    ver = MerkleVerifier(hasher)
    lh = [hasher.hash_leaf(x) for x in leaves]
    hx = lambda hs: [h.hex() for h in hs]   # noqa: E731

    def root(s):
        return tree.merkle_tree_hash(0, s)

    # ---- explicit audit paths
    paths = []
    for s in FULL_SIZES + SPREAD_SIZES:
        for m in (range(s) if s in FULL_SIZES else spread(s)):
            p = tree.inclusion_proof(m, s)
            assert ver.verify_leaf_hash_inclusion(lh[m], m, p, STH(s, root(s)))
            paths.append({'m': m, 's': s, 'path': hx(p)})
    root_sizes = set(range(1, 71)) | set(SPREAD_SIZES)

    # ---- explicit consistency proofs
    rnd = random.Random(6962)
    pairs = [(a, b) for b in range(1, 18) for a in range(0, b + 1)]
    while len(pairs) < 18 * 19 // 2 - 1 + 64:
        b = rnd.randrange(2, n + 1)
        a = rnd.randrange(1, b)
        if (a, b) not in pairs:
            pairs.append((a, b))
    pairs += [(0, 1030), (1030, 1030), (512, 512), (512, 1030), (1, 1030), (1029, 1030)]
    cons = []
    for a, b in pairs:
        # first == 0: CompactMerkleTree._subproof does not terminate; the row records the verifier's
        # contract instead ("a consistency proof with an empty tree is an empty proof")
        p = tree.consistency_proof(a, b) if a else []
        if a:
            assert ver.verify_tree_consistency(a, b, root(a), root(b), p)
        cons.append({'a': a, 'b': b, 'proof': hx(p)})
        root_sizes |= {s for s in (a, b) if s}
    roots = {str(s): root(s).hex() for s in sorted(root_sizes)}   # MTH(0, s) of every size the rows use

    # ---- digests over everything up to 70 leaves
    h = hashlib.sha256()
    count_p = 0
    for s in range(1, 71):
        for m in range(s):
            h.update(b''.join(tree.inclusion_proof(m, s)))
            count_p += 1
    assert count_p == 2485
    digest_paths = h.hexdigest()
    h = hashlib.sha256()
    for b in range(1, 71):
        for a in range(1, b + 1):
            h.update(b''.join(tree.consistency_proof(a, b)))
    digest_cons = h.hexdigest()

    # ---- negative inclusion rows
    neg_incl = []

    def incl_row(what, leaf_hash, index, size, path, rt):
        exc, msg = outcome(ver.verify_leaf_hash_inclusion, leaf_hash, index, list(path), STH(size, rt))
        neg_incl.append({'what': what, 'leaf_hash': leaf_hash.hex(), 'index': index, 'tree_size': size,
                         'path': hx(path), 'root': rt.hex(), 'exc': exc, 'msg': msg})

    for m, s in [(5, 70), (0, 1), (300, 777)]:
        p, rt = tree.inclusion_proof(m, s), root(s)
        incl_row('valid', lh[m], m, s, p, rt)
        for pos in range(len(p)):
            q = list(p)
            q[pos] = flip(q[pos], (37 * pos + m) % 256)
            incl_row('bit flipped in node %d' % pos, lh[m], m, s, q, rt)
        incl_row('leaf hash bit flipped', flip(lh[m], 3), m, s, p, rt)
        if p:
            incl_row('truncated by one node', lh[m], m, s, p[:-1], rt)
            incl_row('first node dropped', lh[m], m, s, p[1:], rt)
        incl_row('empty path', lh[m], m, s, [], rt)
        incl_row('extended by one node', lh[m], m, s, p + [lh[0]], rt)
        incl_row('extended by three nodes', lh[m], m, s, p + lh[:3], rt)
        if m + 1 < s:
            incl_row('m + 1', lh[m], m + 1, s, p, rt)
        if m:
            incl_row('m - 1', lh[m], m - 1, s, p, rt)
        incl_row('tree_size + 1', lh[m], m, s + 1, p, rt)
        incl_row('tree_size - 1', lh[m], m, s - 1, p, rt)
        incl_row('wrong root', lh[m], m, s, p, root(s % n + 1))
        incl_row('tree_size == index', lh[m], s, s, p, rt)
        incl_row('tree_size < index', lh[m], s + 7, s, p, rt)
    incl_row('negative index', lh[0], -1, 5, tree.inclusion_proof(0, 5), root(5))
    incl_row('negative size and index', lh[0], -3, -2, [], root(5))

    # ---- negative consistency rows
    neg_cons = []

    def cons_row(what, a, b, r0, r1, p):
        exc, msg = outcome(ver.verify_tree_consistency, a, b, r0, r1, list(p))
        neg_cons.append({'what': what, 'old': a, 'new': b, 'old_root': r0.hex(), 'new_root': r1.hex(),
                         'proof': hx(p), 'exc': exc, 'msg': msg})

    for a, b in [(3, 7), (4, 8), (5, 1030), (777, 1000)]:
        p, r0, r1 = tree.consistency_proof(a, b), root(a), root(b)
        cons_row('valid', a, b, r0, r1, p)
        cons_row('swapped roots', a, b, r1, r0, p)
        cons_row('wrong old root only', a, b, root(a + 1), r1, p)
        cons_row('wrong new root', a, b, r0, root(b - 1), p)
        cons_row('both roots wrong', a, b, root(a + 1), root(b - 1), p)
        cons_row('truncated proof', a, b, r0, r1, p[:-1])
        cons_row('empty proof', a, b, r0, r1, [])
        cons_row('extended by one node (accepted)', a, b, r0, r1, p + [lh[0]])
        for pos in range(len(p)):
            q = list(p)
            q[pos] = flip(q[pos], (11 * pos + a) % 256)
            cons_row('bit flipped in node %d' % pos, a, b, r0, r1, q)
        cons_row('old > new', b, a, r1, r0, p)
        cons_row('sizes shifted', a, b - 1 if b - 1 > a else b + 1, r0, r1, p)
    cons_row('equal sizes, equal roots, proof ignored', 9, 9, root(9), root(9), [lh[1]])
    cons_row('equal sizes, different roots', 9, 9, root(9), root(10), [])
    cons_row('old size 0, bogus proof ignored', 0, 9, lh[0], root(9), [lh[1], lh[2]])
    cons_row('negative size', -1, 9, root(9), root(9), [])

    # ---- wide indices: random siblings, the root from the reference's own walk
    wide = []
    for size, index in [(2 ** 40 + 5, 3), (2 ** 40 + 5, 2 ** 40 + 4), (2 ** 63, 2 ** 62), (2 ** 64 - 1, 2 ** 64 - 2)]:
        k = ver.audit_path_length(index, size)
        p = [hashlib.sha256(b'wide-%d-%d-%d' % (size, index, j)).digest() for j in range(k)]
        leaf_hash = hashlib.sha256(b'wide-leaf-%d' % index).digest()
        rt = ver._calculate_root_hash_from_audit_path(leaf_hash, index, list(p), size)
        assert ver.verify_leaf_hash_inclusion(leaf_hash, index, p, STH(size, rt))
        for what, q, r in [('valid', p, rt), ('truncated by one node', p[:-1], rt), ('wrong root', p, lh[0]),
                           ('extended by one node', p + [lh[0]], rt)]:
            exc, msg = outcome(ver.verify_leaf_hash_inclusion, leaf_hash, index, list(q), STH(size, r))
            wide.append({'what': what, 'leaf_hash': leaf_hash.hex(), 'index': index, 'tree_size': size,
                         'path': hx(q), 'root': r.hex(), 'exc': exc, 'msg': msg})

    # ---- compact form: every 32-byte value once, in 'nodes' (base64); rows hold indices into it, and the
    # reference's messages name their hashes as <#index> (tests/_merkle_proofs.py fixture() expands it)
    table = {}

    def ref(hexstr):
        return table.setdefault(hexstr, len(table))

    def pack_row(r):
        r = dict(r)
        for key in ('leaf_hash', 'root', 'old_root', 'new_root'):
            if key in r:
                r[key] = ref(r[key])
        for key in ('path', 'proof'):
            if key in r:
                r[key] = [ref(h) for h in r[key]]
        if r.get('msg'):
            r['msg'] = re.sub('[0-9a-f]{64}', lambda m: '<#%d>' % ref(m.group(0)), r['msg'])
        return r

    doc = {'source': 'reference ledger CompactMerkleTree / MerkleVerifier over tests/golden/merkle.json, '
                     'tools/gen_merkle_proofs_golden.py',
           'n_leaves': n,
           'roots': {s: ref(h) for s, h in roots.items()},
           'audit_paths': [[r['m'], r['s'], [ref(h) for h in r['path']]] for r in paths],
           'consistency': [[r['a'], r['b'], [ref(h) for h in r['proof']]] for r in cons],
           'digest_paths_le70': digest_paths, 'digest_cons_le70': digest_cons,
           'neg_inclusion': [pack_row(r) for r in neg_incl], 'neg_consistency': [pack_row(r) for r in neg_cons],
           'wide': [pack_row(r) for r in wide]}
    doc['nodes'] = [base64.b64encode(bytes.fromhex(h)).decode() for h in table]   # base64: 44 characters each
    out = os.path.join(REPO, 'tests', 'golden', 'merkle_proofs.json')
    with open(out, 'w') as fh:
        fh.write('{' + ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(v, separators=(',', ':')))
                                  for k, v in doc.items()) + '}\n')
    print('wrote', out, os.path.getsize(out), 'bytes:', len(paths), 'paths,', len(cons), 'proofs,',
          len(neg_incl), '+', len(neg_cons), 'verdict rows,', len(wide), 'wide rows,', len(table), 'nodes')


if __name__ == '__main__':
    main()
