"""Merkle proof checker helpers (tests only): audit paths, the right-edge chain
and consistency proofs restated with hashlib over a level-wise tree (an odd
last node moves up), for sizes the reference fixture
(tests/golden/merkle_proofs.json, tools/gen_merkle_proofs_golden.py) does not
hold.  The restatement itself is checked against that fixture on the CPU
(tests/test_merkle_proofs_host.py)."""
import base64
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np

from conftest import GOLDEN, REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
_host_lib = None


def host_lib():
    """csrc/pv_merkle_proof.h built for the host (tools/hostcheck/merklecheck.cpp)"""
    global _host_lib
    if _host_lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libmerklecheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libmerklecheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.mc_verify_inclusion.restype = ctypes.c_uint32
        so.mc_verify_inclusion.argtypes = [ctypes.c_char_p, u64, u64, ctypes.c_char_p, u64, ctypes.c_char_p, vp,
                                           ctypes.POINTER(u64)]
        so.mc_verify_consistency.restype = ctypes.c_uint32
        so.mc_verify_consistency.argtypes = [u64, u64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u64, vp, vp]
        so.mc_tree_new.restype = vp
        so.mc_tree_new.argtypes = [ctypes.c_char_p, u64]
        so.mc_tree_free.argtypes = [vp]
        so.mc_tree_depth.restype = ctypes.c_uint32
        so.mc_tree_depth.argtypes = [vp]
        so.mc_audit_path.restype = ctypes.c_uint32
        so.mc_audit_path.argtypes = [vp, u64, u64, vp, vp]
        so.mc_cons_proof.restype = ctypes.c_uint32
        so.mc_cons_proof.argtypes = [vp, u64, u64, vp]
        _host_lib = so
    return _host_lib


def host_inclusion(lib, leaf_hash, index, size, path, root):
    """mp_verify_inclusion on the host -> (status, computed, stop index)"""
    comp, stop = np.zeros(32, np.uint8), ctypes.c_uint64(0)
    st = lib.mc_verify_inclusion(leaf_hash, index, size, b''.join(path), len(path), root, comp.ctypes.data,
                                 ctypes.byref(stop))
    return st, comp.tobytes(), stop.value


def host_consistency(lib, old, new, r0, r1, proof):
    """mp_verify_consistency on the host -> (status, old computed, new computed)"""
    c0, c1 = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    st = lib.mc_verify_consistency(old, new, r0, r1, b''.join(proof), len(proof), c0.ctypes.data, c1.ctypes.data)
    return st, c0.tobytes(), c1.tobytes()


def leaf(d):
    return hashlib.sha256(b'\x00' + d).digest()


def node(l, r):
    return hashlib.sha256(b'\x01' + l + r).digest()


def fixture():
    """The fixture, expanded: it stores every 32-byte value once (in 'nodes', base64);
    rows hold indices into that table and messages name hashes as <#index>."""
    with open(os.path.join(GOLDEN, 'merkle_proofs.json')) as fh:
        d = json.load(fh)
    nodes = [base64.b64decode(x).hex() for x in d.pop('nodes')]
    d['roots'] = {s: nodes[i] for s, i in d['roots'].items()}
    d['audit_paths'] = [{'m': m, 's': s, 'path': [nodes[i] for i in p]} for m, s, p in d['audit_paths']]
    d['consistency'] = [{'a': a, 'b': b, 'proof': [nodes[i] for i in p]} for a, b, p in d['consistency']]
    for r in d['neg_inclusion'] + d['neg_consistency'] + d['wide']:
        for key in ('leaf_hash', 'root', 'old_root', 'new_root'):
            if key in r:
                r[key] = nodes[r[key]]
        for key in ('path', 'proof'):
            if key in r:
                r[key] = [nodes[i] for i in r[key]]
        if r['msg']:
            r['msg'] = re.sub(r'<#(\d+)>', lambda m: nodes[int(m.group(1))], r['msg'])
    return d


def unhex(hs):
    return [bytes.fromhex(h) for h in hs]


OK, BAD_RANGE, TOO_SHORT, TOO_LONG, ROOT_MISMATCH, INCONSISTENT = range(6)   # PV_MP_* of plenum_verify.h


def _hex_in(msg, label):
    """the hash printed after `label` as b'<hex>' in a reference message"""
    tail = msg.split(label, 1)[1]
    return bytes.fromhex(tail.split("b'", 1)[1].split("'", 1)[0])


def expect_inclusion(row):
    """fixture verdict row -> (status, computed root or None, stop index or None)
    as the per-proof routine must report it"""
    exc, msg = row['exc'], row['msg']
    if exc is None:
        return OK, bytes.fromhex(row['root']), 0
    if exc == 'ValueError':
        return BAD_RANGE, None, None
    assert exc == 'ProofError', exc
    if msg.startswith('Proof too short'):
        return TOO_SHORT, None, int(msg.rsplit(' ', 1)[1])
    if msg.startswith('Proof too long'):
        return TOO_LONG, None, 0
    assert msg.startswith('Constructed root hash differs'), msg
    return ROOT_MISMATCH, _hex_in(msg, 'Constructed:'), 0


def expect_consistency(row):
    """-> (status, computed old root or None, computed new root or None)"""
    exc, msg = row['exc'], row['msg']
    if exc is None:
        return OK, None, None
    if exc == 'ValueError':
        return BAD_RANGE, None, None
    if exc == 'ConsistencyError':
        if 'same tree size' in msg:
            return INCONSISTENT, None, None
        return INCONSISTENT, _hex_in(msg, 'computed hash:'), bytes.fromhex(row['new_root'])
    assert exc == 'ProofError', exc
    if msg == 'Merkle proof is too short':
        return TOO_SHORT, None, None
    assert msg.startswith('Bad Merkle proof'), msg
    return ROOT_MISMATCH, None, _hex_in(msg, 'computed hash:')


def negative(row):
    """rows a 64-bit unsigned interface cannot carry (host-side ValueErrors only)"""
    return any(row.get(k, 0) < 0 for k in ('index', 'tree_size', 'old', 'new'))


class LevelTree:
    """lv[l][j] = node j of level l; level 0 = the leaf hashes"""

    def __init__(self, leaf_hashes):
        self.lv = [list(leaf_hashes)]
        self._chains = {}
        while len(self.lv[-1]) > 1:
            cur = self.lv[-1]
            nxt = [node(cur[i], cur[i + 1]) for i in range(0, len(cur) - 1, 2)]
            if len(cur) % 2:
                nxt.append(cur[-1])
            self.lv.append(nxt)

    @property
    def size(self):
        return len(self.lv[0])

    def chain(self, s):
        """[e_0, e_1, ...] of the prefix of s leaves: e_l is node (s-1) >> l of
        the prefix tree's level l; the last entry is MTH(0, s)"""
        if s not in self._chains:
            e, out, last, l = self.lv[0][s - 1], [], s - 1, 0
            out.append(e)
            while last > 0:
                if last & 1:
                    e = node(self.lv[l][last - 1], e)
                out.append(e)
                l, last = l + 1, last >> 1
            self._chains[s] = out
        return self._chains[s]

    def root(self, s):
        return self.chain(s)[-1]

    def _at(self, s, l, i):
        return self.chain(s)[l] if i == (s - 1) >> l else self.lv[l][i]

    def audit_path(self, m, s):
        assert 0 <= m < s <= self.size
        out, l = [], 0
        while (s - 1) >> l > 0:
            sib = (m >> l) ^ 1
            if sib <= (s - 1) >> l:
                out.append(self._at(s, l, sib))
            l += 1
        return out

    def consistency_proof(self, a, b):
        assert 0 <= a <= b <= self.size
        if a == 0 or a == b:
            return []
        out, node_, last, l = [], a - 1, b - 1, 0
        while node_ & 1:
            node_, last, l = node_ >> 1, last >> 1, l + 1
        if node_:
            out.append(self._at(b, l, node_))
        while last:
            if node_ & 1:
                out.append(self.lv[l][node_ - 1])
            elif node_ < last:
                out.append(self._at(b, l, node_ + 1))
            node_, last, l = node_ >> 1, last >> 1, l + 1
        return out


def rfc_mth(hashes):
    """RFC 6962 section 2.1 over leaf hashes (independent of LevelTree)"""
    if len(hashes) == 1:
        return hashes[0]
    k = 1 << ((len(hashes) - 1).bit_length() - 1)
    return node(rfc_mth(hashes[:k]), rfc_mth(hashes[k:]))


def rfc_path(m, hashes):
    """RFC 6962 section 2.1.1 PATH(m, D[n]), bottom-up"""
    if len(hashes) == 1:
        return []
    k = 1 << ((len(hashes) - 1).bit_length() - 1)
    if m < k:
        return rfc_path(m, hashes[:k]) + [rfc_mth(hashes[k:])]
    return rfc_path(m - k, hashes[k:]) + [rfc_mth(hashes[:k])]


def rfc_proof(m, hashes, b=True):
    """RFC 6962 section 2.1.2 SUBPROOF(m, D[n], b)"""
    n = len(hashes)
    if m == n:
        return [] if b else [rfc_mth(hashes)]
    k = 1 << ((n - 1).bit_length() - 1)
    if m <= k:
        return rfc_proof(m, hashes[:k], b) + [rfc_mth(hashes[k:])]
    return rfc_proof(m - k, hashes[k:], False) + [rfc_mth(hashes[:k])]
