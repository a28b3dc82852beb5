"""Ledger write-cycle checker helpers (tests only): the reference fixture
tests/golden/ledger_cycle.json (tools/gen_ledger_cycle_golden.py), a hashlib
mirror of the stage / commit / discard cycle with the hash-store order and the
frontier in closed form over _merkle_proofs.LevelTree, and the host build of
csrc/pv_merkle_ledger.h (tools/hostcheck/ledgercheck.cpp)."""
import base64
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np

import _merkle_proofs as mp
from conftest import GOLDEN

HC_DIR = mp.HC_DIR
EMPTY_ROOT = hashlib.sha256(b'').digest()
_host_lib = None


def fixture():
    """The fixture, expanded: every 32-byte value is stored once (in 'nodes', base64)."""
    with open(os.path.join(GOLDEN, 'ledger_cycle.json')) as fh:
        d = json.load(fh)
    nodes = [base64.b64decode(x) for x in d.pop('nodes')]
    d['steps'] = [{'op': op, 'count': c, 'committed': cs, 'total': ts, 'committed_root': nodes[cr],
                   'unc_root': None if ur is None else nodes[ur], 'hashes': [nodes[i] for i in hs]}
                  for op, c, cs, ts, cr, ur, hs in d['steps']]
    d['store_nodes'] = [(s, h, nodes[i]) for s, h, i in d['store_nodes']]
    cu = d['catchup']
    cu['final_hash'] = nodes[cu['final_hash']]
    cu['proofs'] = [[nodes[i] for i in p] for p in cu['proofs']]
    for v in cu['variants']:
        if 'node' in v:
            v['node'] = (v['node'][0], v['node'][1], nodes[v['node'][2]])
        if 'leaf' in v:
            v['leaf'] = (v['leaf'][0], v['leaf'][1], bytes.fromhex(v['leaf'][2]))
        if 'final_hash' in v:
            v['final_hash'] = nodes[v['final_hash']]
    return d


def catchup_case(fx, leaves, variant):
    """-> (reps [(leaves, proof)], final_size, final_hash) of one fixture variant"""
    cu = fx['catchup']
    bounds = [cu['base']] + cu['ends']
    reps = [[list(leaves[bounds[i]:bounds[i + 1]]), list(cu['proofs'][i])] for i in range(len(cu['ends']))]
    if 'leaf' in variant:
        r, j, value = variant['leaf']
        reps[r][0][j] = value
    if 'node' in variant:
        r, j, value = variant['node']
        reps[r][1][j] = value
    return [tuple(r) for r in reps], cu['final_size'], variant.get('final_hash', cu['final_hash'])


def popcount(x):
    return bin(x).count('1')


def ctz(e):
    return (e & -e).bit_length() - 1


def nodes_upto(e):
    """nodes in the hash store once e leaves were appended one by one"""
    return e - popcount(e)


def store_nodes(tree, first, last):
    """the nodes the hash store receives for leaves first + 1 .. last of a
    _merkle_proofs.LevelTree, in writeNode order, as (e, height, hash)"""
    return [(e, h, tree.lv[h][(e >> h) - 1]) for e in range(first + 1, last + 1) for h in range(1, ctz(e) + 1)]


def frontier(tree, size):
    """CompactMerkleTree.hashes of the prefix of `size` leaves of a LevelTree"""
    return [tree.lv[b][(size >> b) - 1] for b in reversed(range(size.bit_length())) if (size >> b) & 1]


def root_of(leaf_hashes):
    return mp.LevelTree(leaf_hashes).lv[-1][0] if leaf_hashes else EMPTY_ROOT


class Mirror:
    """the cycle over a plain list of leaf hashes: sizes, roots and frontier from scratch after every op"""

    def __init__(self):
        self.lh, self.committed = [], 0

    def stage(self, leaf_hashes):
        self.lh += list(leaf_hashes)

    def commit(self, count):
        assert count <= len(self.lh) - self.committed
        self.committed += count

    def discard(self, count):
        assert count <= len(self.lh) - self.committed
        if count:
            del self.lh[-count:]

    def state(self):
        """(committed, total, committed root, uncommittedRootHash, hashes) as the fixture rows hold them"""
        total = len(self.lh)
        tree = mp.LevelTree(self.lh) if total else None
        unc = tree.root(total) if total > self.committed else None
        com = tree.root(self.committed) if self.committed else EMPTY_ROOT
        return self.committed, total, com, unc, frontier(tree, total) if total else []


def host_lib():
    """csrc/pv_merkle_ledger.h built for the host (tools/hostcheck/ledgercheck.cpp)"""
    global _host_lib
    if _host_lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libledgercheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libledgercheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.lc_tree_new.restype = vp
        so.lc_tree_free.argtypes = [vp]
        so.lc_stage.argtypes = [vp, ctypes.c_char_p, u64, vp]
        so.lc_commit.argtypes = [vp, u64]
        so.lc_discard.argtypes = [vp, u64, vp]
        so.lc_sizes.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        so.lc_frontier.restype = ctypes.c_uint32
        so.lc_frontier.argtypes = [vp, u64, vp]
        so.lc_hash_store.restype = u64
        so.lc_hash_store.argtypes = [vp, u64, u64, vp, vp]
        so.lc_check_nodes.restype = u64
        so.lc_check_nodes.argtypes = [vp, u64, u64, ctypes.c_char_p, ctypes.POINTER(u64)]
        _host_lib = so
    return _host_lib


class HostTree:
    """the header's routines on the host behind the C ABI's shape"""

    def __init__(self):
        self.so = host_lib()
        self.t = self.so.lc_tree_new()

    def close(self):
        self.so.lc_tree_free(self.t)

    def stage(self, leaf_hashes):
        root = np.zeros(32, np.uint8)
        assert self.so.lc_stage(self.t, b''.join(leaf_hashes), len(leaf_hashes), root.ctypes.data) == 0
        return root.tobytes()

    def commit(self, count):
        return self.so.lc_commit(self.t, count)

    def discard(self, count):
        root = np.zeros(32, np.uint8)
        rc = self.so.lc_discard(self.t, count, root.ctypes.data)
        return rc, root.tobytes()

    def sizes(self):
        c, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.so.lc_sizes(self.t, ctypes.byref(c), ctypes.byref(t))
        return c.value, t.value

    def frontier(self, size):
        out = np.zeros((64, 32), np.uint8)
        cnt = self.so.lc_frontier(self.t, size, out.ctypes.data)
        return None if cnt == 0xffffffff else [out[i].tobytes() for i in range(cnt)]

    def hash_store(self, first, last):
        need = nodes_upto(last) - nodes_upto(first)
        lo, no = np.zeros((last - first + 1, 32), np.uint8), np.zeros((need + 1, 32), np.uint8)
        assert self.so.lc_hash_store(self.t, first, last, lo.ctypes.data, no.ctypes.data) == need
        assert not lo[-1].any() and not no[-1].any()
        return [x.tobytes() for x in lo[:-1]], [x.tobytes() for x in no[:-1]]

    def check_nodes(self, first, last, nodes):
        at = ctypes.c_uint64(0)
        bad = self.so.lc_check_nodes(self.t, first, last, b''.join(nodes), ctypes.byref(at))
        return bad, (None if at.value == 2 ** 64 - 1 else at.value)


class ListStore:
    """duck-typed hash store, list-backed: ledger/hash_stores/memory_hash_store.py MemoryHashStore"""

    def __init__(self):
        self._leafs, self._nodes = [], []

    def writeLeaf(self, leafHash):
        self._leafs.append(leafHash)

    def writeNode(self, nodeHash):
        self._nodes.append(nodeHash)

    def readLeafs(self, startpos, endpos):
        return list(self._leafs[startpos - 1:endpos])

    def readNodes(self, startpos, endpos):
        return list(self._nodes[startpos - 1:endpos])

    @property
    def leafCount(self):
        return len(self._leafs)

    @property
    def nodeCount(self):
        return len(self._nodes)
