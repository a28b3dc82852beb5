"""State-proof test helpers: the reference fixture tests/golden/state_proofs.json
(tools/gen_state_proofs_golden.py), the kernels' headers built for the host
(tools/hostcheck/stateproofcheck.cpp) and the packing of queries into the
arrays of pv_state_proof_verify."""
import base64
import ctypes
import json
import os
import subprocess

import numpy as np

from conftest import GOLDEN, REPO

HC_DIR = os.path.join(REPO, 'tools', 'hostcheck')
OK, VALUE_MISMATCH, NODE_MISSING, MALFORMED = range(4)   # PV_SP_* of plenum_verify.h
_host_lib = None
_fixture = None


def host_lib():
    """csrc/pv_sha3.h + pv_trie_proof.h built for the host"""
    global _host_lib
    if _host_lib is None:
        subprocess.run(['make', '-s', '-C', HC_DIR, 'libstateproofcheck.so'], check=True)
        so = ctypes.CDLL(os.path.join(HC_DIR, 'libstateproofcheck.so'))
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        so.sc_sha3_256.restype = None
        so.sc_sha3_256.argtypes = [vp, u64, u64, vp]
        so.sc_state_proof_verify.restype = None
        so.sc_state_proof_verify.argtypes = [vp] * 10 + [u64, u64, u64, vp]
        so.sc_rlp_split_list.restype = ctypes.c_int
        so.sc_rlp_split_list.argtypes = [vp, u64, vp, vp, u64, ctypes.POINTER(u64)]
        _host_lib = so
    return _host_lib


def list_header(n):
    if n < 56:
        return bytes([192 + n])
    ls = n.to_bytes((n.bit_length() + 7) // 8, 'big')
    return bytes([247 + len(ls)]) + ls


def serialize(nodes):
    """rlp(list of nodes) from the nodes' own RLP: what Trie.serialize_proof gives"""
    body = b''.join(nodes)
    return list_header(len(body)) + body


def encode_value(v):
    """PruningState.encode_kv_for_verification's value: rlp([v]), None -> b''"""
    if v is None:
        return b''
    if len(v) == 1 and v[0] < 128:
        item = v
    elif len(v) < 56:
        item = bytes([128 + len(v)]) + v
    else:
        ls = len(v).to_bytes((len(v).bit_length() + 7) // 8, 'big')
        item = bytes([183 + len(ls)]) + ls + v
    return list_header(len(item)) + item


class Row:
    """one reference call: (root, [(key, value or None)], proof nodes) -> verdict"""
    __slots__ = ('trie', 'kind', 'root', 'kvs', 'nodes', 'verdict', 'multi')

    def __init__(self, trie, kind, root, kvs, nodes, verdict, multi):
        self.trie, self.kind, self.root, self.kvs, self.nodes = trie, kind, root, kvs, nodes
        self.verdict, self.multi = verdict, multi

    @property
    def lenient(self):
        """the serialized proof holds a length that overruns its enclosing item: the
        reference's verdict is recorded, the project's is False by rule"""
        return '/lenient' in self.kind

    @property
    def expected(self):
        return False if self.lenient else self.verdict

    @property
    def serialized(self):
        return serialize(self.nodes)


def fixture():
    """[Row] of the fixture, single-key rows first, loaded once"""
    global _fixture
    if _fixture is None:
        with open(os.path.join(GOLDEN, 'state_proofs.json')) as fh:
            d = json.load(fh)
        nodes = [base64.b64decode(x) for x in d['nodes']]
        roots = [bytes.fromhex(r) for r in d['roots']]
        keys = [base64.b64decode(k) for k in d['keys']]
        # a value is base64, or [node, offset, length]: those bytes of that node
        values = [base64.b64decode(v) if isinstance(v, str) else nodes[v[0]][v[1]:v[1] + v[2]] for v in d['values']]
        tries, kinds = d['tries'], d['kinds']

        def flip(i, bit):
            b = bytearray(nodes[i])
            b[bit // 8] ^= 1 << (bit % 8)
            return bytes(b)

        proof = lambda p: [flip(*x) if isinstance(x, list) else nodes[x] for x in p]   # noqa: E731
        kv = lambda k, v: (keys[k], None if v < 0 else values[v])                       # noqa: E731
        rows = [Row(tries[t], kinds[kd], roots[r], [kv(k, v)], proof(p), bool(ok), False)
                for t, kd, r, k, v, p, ok in d['rows']]
        rows += [Row(tries[t], kinds[kd], roots[r], [kv(k, v) for k, v in kvs], proof(p), bool(ok), True)
                 for t, kd, r, kvs, p, ok in d['multi']]
        _fixture = rows
    return _fixture


class Packed:
    """The arrays of one pv_state_proof_verify call over `rows`: each row is one
    proof (its serialized bytes in the blob, nodes found by `split`) and one query
    per (key, value) pair.  Rows whose proof does not split add no proof and no
    query; `row_queries[i]` = (first query, count) or None for those."""

    def __init__(self, rows, split, pad_front=0):
        chunks, beg, end, first, roots = [b'\x5a' * pad_front], [], [], [0], []
        pidx, keys, vals, self.row_queries = [], [], [], []
        pos = pad_front
        for r in rows:
            ser = r.serialized
            ranges = split(ser)
            if ranges is None:
                self.row_queries.append(None)
                continue
            for b, e in ranges:
                beg.append(pos + b)
                end.append(pos + e)
            chunks.append(ser)
            pos += len(ser)
            first.append(len(beg))
            roots.append(r.root)
            self.row_queries.append((len(pidx), len(r.kvs)))
            for k, v in r.kvs:
                pidx.append(len(roots) - 1)
                keys.append(k)
                vals.append(encode_value(v))
        # 16 readable bytes after the last node, as the kernels' loads need (the
        # host entry point adds its own; the host build reads this array directly)
        self.blob_len = pos
        self.blob = np.frombuffer(b''.join(chunks) + b'\0' * 16, np.uint8).copy()
        self.beg, self.end = np.array(beg, np.uint64), np.array(end, np.uint64)
        self.first = np.array(first, np.uint64)
        self.roots = np.frombuffer(b''.join(roots), np.uint8).copy() if roots else np.zeros(0, np.uint8)
        self.pidx = np.array(pidx, np.uint32)
        self.keys, self.koff = _pack(keys)
        self.vals, self.voff = _pack(vals)
        self.N, self.P, self.Q = len(beg), len(roots), len(pidx)

    @classmethod
    def single(cls, nodes, root, key, val):
        """one proof of the given node byte strings (taken as they are, not split out of
        a serialized proof) and one query with the ENCODED value `val`"""
        self = object.__new__(cls)
        ends = np.cumsum([len(n) for n in nodes]).astype(np.uint64)
        self.blob_len = int(ends[-1]) if len(nodes) else 0
        self.blob = np.frombuffer(b''.join(nodes) + b'\0' * 16, np.uint8).copy()
        self.end = ends
        self.beg = np.concatenate([np.zeros(1, np.uint64), ends[:-1]]) if len(nodes) else ends
        self.first = np.array([0, len(nodes)], np.uint64)
        self.roots = np.frombuffer(root, np.uint8).copy()
        self.pidx = np.zeros(1, np.uint32)
        self.keys, self.koff = _pack([key])
        self.vals, self.voff = _pack([val])
        self.N, self.P, self.Q = len(nodes), 1, 1
        self.row_queries = [(0, 1)]
        return self

    def verdicts(self, status):
        """per row: every query PV_SP_OK (False for a proof that did not split)"""
        return [False if q is None else bool((status[q[0]:q[0] + q[1]] == OK).all()) for q in self.row_queries]


def _pack(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b''.join(msgs) + b'\0' * 4, np.uint8).copy(), off


def decode(b):
    """strict RLP decode of one item -> bytes or nested lists (the test's own reader)"""
    def item(pos, lim):
        b0 = b[pos]
        if b0 < 128:
            return b[pos:pos + 1], pos + 1
        if b0 < 184:
            ll, n, is_list = 0, b0 - 128, False
        elif b0 < 192:
            ll, n, is_list = b0 - 183, None, False
        elif b0 < 248:
            ll, n, is_list = 0, b0 - 192, True
        else:
            ll, n, is_list = b0 - 247, None, True
        if n is None:
            n = int.from_bytes(b[pos + 1:pos + 1 + ll], 'big')
        pb = pos + 1 + ll
        assert pb + n <= lim
        if not is_list:
            return b[pb:pb + n], pb + n
        out, p = [], pb
        while p < pb + n:
            x, p = item(p, pb + n)
            out.append(x)
        return out, pb + n
    x, end = item(0, len(b))
    assert end == len(b)
    return x


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else ctypes.c_void_p(0)


def host_statuses(pk):
    """sc_state_proof_verify over a Packed -> status uint8[Q]"""
    st = np.full(pk.Q, 0xee, np.uint8)
    if pk.Q:
        host_lib().sc_state_proof_verify(ptr(pk.blob), ptr(pk.beg), ptr(pk.end), ptr(pk.first), ptr(pk.roots),
                                         ptr(pk.pidx), ptr(pk.keys), ptr(pk.koff), ptr(pk.vals), ptr(pk.voff),
                                         pk.N, pk.P, pk.Q, ptr(st))
    return st


def host_split(data):
    """rlp_split_list of pv_trie_proof.h on the host -> [(begin, end)] or None"""
    buf = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    cap = max(len(data), 1)
    beg, end = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    count = ctypes.c_uint64(0)
    rc = host_lib().sc_rlp_split_list(ptr(buf), len(data), ptr(beg), ptr(end), cap, ctypes.byref(count))
    if rc != 0:
        return None
    return list(zip(beg[:count.value].tolist(), end[:count.value].tolist()))


def host_sha3(blob, beg, end):
    """SHA3-256 of blob[beg:end] in place (blob: uint8 array with 16 spare bytes after end)"""
    out = np.zeros(32, np.uint8)
    host_lib().sc_sha3_256(ptr(blob), beg, end, ptr(out))
    return out.tobytes()
