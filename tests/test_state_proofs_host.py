"""State proofs on the CPU: the Python mirror (plenum_gpu.state_proofs below its
GPU threshold) and the routines the kernels run (csrc/pv_sha3.h,
csrc/pv_trie_proof.h, built for the host) against hashlib and the reference
fixture tests/golden/state_proofs.json.

Rows marked '/lenient' hold a serialized proof in which some length overruns its
enclosing item.  The reference's decoder slices such a length off and re-encodes
the node before hashing it, so it accepts 56 of those 136 proofs; the project
answers False for all of them by rule (Row.expected)."""
import hashlib
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import _state_proofs as sp
import _trie_hostile as th

BOUNDARY = [0, 1, 135, 136, 137, 271, 272, 273, 407, 408, 1000]


@pytest.fixture(scope='module')
def rows():
    return sp.fixture()


@pytest.fixture(scope='module')
def mirror(monkeypatch_module):
    from plenum_gpu import state_proofs
    monkeypatch_module.setattr(state_proofs, 'GPU_MIN_ITEMS', 1 << 62)   # every size through the mirror
    return state_proofs


@pytest.fixture(scope='module')
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope='module')
def host_packed(rows):
    pk = sp.Packed(rows, sp.host_split)
    return pk, sp.host_statuses(pk)


def _items(rows):
    out = []
    for r in rows:
        proof = r.serialized
        if r.multi:
            out.append((r.root, dict(r.kvs), proof))
        else:
            out.append((r.root, r.kvs[0][0], r.kvs[0][1], proof))
    return out


def test_fixture_covers_the_cases(rows):
    kinds = {r.kind.split('/lenient')[0] for r in rows}
    for want in ('own', 'wrong_value', 'none_for_present', 'other_proof', 'flipped', 'dropped', 'wrong_root',
                 'shuffled', 'reversed', 'duplicated', 'extra_nodes', 'blank_root', 'absent/blank_slot',
                 'absent/leaf_mismatch', 'absent/ext_mismatch', 'absent/branch_no_value', 'absent/longer_than_leaf',
                 'absent_with_value/blank_slot', 'all_right', 'one_wrong', 'one_absent_with_value',
                 'one_absent_none'):
        assert want in kinds, want
    assert all(r.verdict for r in rows if r.kind in ('own', 'shuffled', 'reversed', 'duplicated', 'extra_nodes'))
    assert max(len(n) for r in rows for n in r.nodes) > 3 * 136      # leaves of 3 or more Keccak blocks
    assert any(r.lenient and r.verdict for r in rows)


def test_mirror_equals_reference_on_every_row(rows, mirror):
    got = mirror.verify_state_proofs_batch(_items(rows))
    bad = [(r.trie, r.kind) for r, g in zip(rows, got) if bool(g) != r.expected]
    assert not bad, bad[:10]
    # outside the marked rows that is the reference's own verdict
    assert all(r.expected == r.verdict for r in rows if not r.lenient)


def test_mirror_single_calls_and_unserialized(rows, mirror):
    V = mirror.GpuStateVerifier
    decode = sp.decode
    picked = [r for r in rows if not r.lenient and r.kind not in ('flipped', 'dropped')][::7] + \
             [r for r in rows if r.multi and not r.lenient]
    for r in picked:
        nodes = [decode(n) for n in r.nodes]
        if r.multi:
            assert V.verify_state_proof_multi(r.root, dict(r.kvs), r.serialized, serialized=True) == r.verdict
            assert V.verify_state_proof_multi(r.root, dict(r.kvs), nodes) == r.verdict
        else:
            k, v = r.kvs[0]
            assert V.verify_state_proof(r.root, k, v, r.serialized, serialized=True) == r.verdict
            assert V.verify_state_proof(r.root, k, v, nodes) == r.verdict
            assert V.verify_state_proof(r.root, k.decode('latin-1') if max(k, default=0) < 128 else k, v,
                                        nodes) == r.verdict


def test_encoder_against_the_fixture_nodes(rows, mirror):
    nodes = {n for r in rows if not r.kind.startswith('flipped') for n in r.nodes}
    assert len(nodes) > 300
    inline = 0
    for n in nodes:
        dec = sp.decode(n)
        inline += any(isinstance(x, list) for x in dec)
        assert mirror.rlp_encode(dec) == n
    assert inline      # nodes with inline children are among them
    for r in rows:
        if r.kind == 'own':
            assert mirror.rlp_encode([sp.decode(n) for n in r.nodes]) == r.serialized
    assert mirror.rlp_encode(b'') == b'\x80' and mirror.rlp_encode(b'\x7f') == b'\x7f'
    assert mirror.rlp_encode(b'\x80') == b'\x81\x80' and mirror.rlp_encode([]) == b'\xc0'
    assert mirror.rlp_encode([b'x' * 56]) == b'\xf8\x3a\xb8\x38' + b'x' * 56
    assert mirror.rlp_encode([[b'a', [b'b']], b'']) == b'\xc5\xc3\x61\xc1\x62\x80'
    for r in rows:
        for k, v in r.kvs:
            assert mirror.GpuStateVerifier.encode_kv_for_verification(k, v)[1] == sp.encode_value(v)
    assert mirror.GpuStateVerifier.encode_kv_for_verification('k1', None) == (b'k1', b'')


def test_host_sha3_boundary_lengths_at_every_offset():
    rng = random.Random(3)
    for n in BOUNDARY:
        m = bytes(rng.getrandbits(8) for _ in range(n))
        want = hashlib.sha3_256(m).digest()
        for off in range(8):
            blob = np.frombuffer(b'\xa5' * off + m + b'\x5a' * 16, np.uint8).copy()
            assert sp.host_sha3(blob, off, off + n) == want, (n, off)


def test_host_sha3_random_lengths():
    rng = random.Random(4)
    msgs = [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 4096))) for _ in range(200)]
    blob = np.frombuffer(b''.join(msgs) + b'\0' * 16, np.uint8).copy()
    pos = 0
    for m in msgs:
        assert sp.host_sha3(blob, pos, pos + len(m)) == hashlib.sha3_256(m).digest(), len(m)
        pos += len(m)


def test_host_walk_equals_reference_on_every_row(rows, host_packed):
    pk, st = host_packed
    assert set(st.tolist()) <= {sp.OK, sp.VALUE_MISMATCH, sp.NODE_MISSING, sp.MALFORMED}
    got = pk.verdicts(st)
    bad = [(r.trie, r.kind) for r, g in zip(rows, got) if g != r.expected]
    assert not bad, bad[:10]
    # every status occurs, so the comparison below means something
    assert {sp.OK, sp.VALUE_MISMATCH, sp.NODE_MISSING} <= set(st.tolist())


def test_host_statuses_equal_mirror_statuses(rows, mirror, host_packed):
    pk, st = host_packed
    mst, queries = mirror.state_proof_statuses(_items(rows))
    assert len(mst) == len(st)
    assert (mst == st).all(), np.nonzero(mst != st)[0][:10]
    for q, (first, count, fixed) in zip(pk.row_queries, queries):
        assert (q is None) == (fixed is False)
        if q is not None:
            assert q == (first, count)


def test_malformed_nodes_by_rule(mirror):
    """a node reachable only through a SHA3 preimage: False, with the status of the rule"""
    def status(nodes, key, val=b''):
        root = hashlib.sha3_256(nodes[0]).digest()
        blob = b''.join(nodes)
        ranges, pos = [], 0
        for n in nodes:
            ranges.append((pos, pos + len(n)))
            pos += len(n)
        m = mirror.walk_status(blob, ranges, [hashlib.sha3_256(n).digest() for n in nodes], root, key, val)
        assert sp.host_statuses(sp.Packed.single(nodes, root, key, val))[0] == m
        return m

    leaf = b'\xc5\x83\x20\x6b\x31\x76'
    assert status([leaf], b'k1', b'v') == sp.OK
    assert status([leaf], b'k1') == sp.VALUE_MISMATCH
    assert status([leaf + b'\x00'], b'k1', b'v') == sp.MALFORMED            # bytes after the list
    assert status([b'\xc6\x83\x20\x6b\x31\x76'], b'k1', b'v') == sp.MALFORMED   # the list overruns the node
    assert status([b'\xc3\x80\x80\x80'], b'k1') == sp.MALFORMED             # 3 items
    assert status([b'\xc2\x80\x76'], b'k1') == sp.MALFORMED                 # empty path item
    assert status([b'\xc3\xc1\x20\x76'], b'k1') == sp.MALFORMED             # the path is a list
    assert status([b'\xc6\x83\x20\x6b\x31\xc1\x76'], b'k1') == sp.MALFORMED  # the value is a list
    ext = b'\xe2\x00\xa0' + hashlib.sha3_256(leaf).digest()
    assert status([ext, leaf], b'k1', b'v') == sp.MALFORMED                 # an extension with an empty path
    ext = b'\xc3\x16\x81\x99'
    assert status([ext, leaf], b'k1', b'v') == sp.NODE_MISSING              # a 1-byte child reference
    assert status([b'\xd2' + b'\x80' * 18], b'k1') == sp.MALFORMED          # 18 items


def test_rlp_split_list_valid_truncated_and_overlong(rows, mirror):
    ser = next(r for r in rows if r.kind == 'own' and len(r.nodes) >= 4).serialized
    ranges = sp.host_split(ser)
    assert ranges == mirror.rlp_split_list(ser)
    assert b''.join(ser[b:e] for b, e in ranges) == ser[ranges[0][0]:] and len(ranges) >= 4
    for data in (b'', b'\x80', b'\x7f', b'\xc0', b'\xc1', b'\xc1\x80', b'\xc1\x80\x80', b'\xc2\x81', b'\xf8',
                 b'\xf8\x01\x80', b'\xf9\x00\x01\x80', b'\xff' + b'\xff' * 8, b'\xbf' + b'\xff' * 8,
                 ser[:-1], ser + b'\x00', ser[:len(ser) // 2], ser[1:]):
        assert sp.host_split(data) == mirror.rlp_split_list(data), data[:12]
    assert sp.host_split(b'\xc0') == [] and sp.host_split(b'\xc1\x80') == [(1, 2)]
    assert sp.host_split(ser[:-1]) is None and sp.host_split(ser + b'\x00') is None and sp.host_split(b'') is None
    assert sp.host_split(b'\xf8\x01\x80') == [(2, 3)]        # lenient: a long form for a short length
    rng = random.Random(5)
    for _ in range(2000):
        data = bytearray(ser[:rng.randint(1, len(ser))])
        for _ in range(rng.randint(0, 3)):
            data[rng.randrange(len(data))] = rng.getrandbits(8)
        assert sp.host_split(bytes(data)) == mirror.rlp_split_list(bytes(data))


def test_unsplittable_serialized_proof_is_false(rows, mirror):
    r = next(r for r in rows if r.kind == 'own')
    k, v = r.kvs[0]
    assert mirror.GpuStateVerifier.verify_state_proof(r.root, k, v, r.serialized, serialized=True) is True
    assert mirror.GpuStateVerifier.verify_state_proof(r.root, k, v, r.serialized[:-1], serialized=True) is False
    assert mirror.GpuStateVerifier.verify_state_proof_multi(r.root, {k: v}, b'\x83abc', serialized=True) is False
    got = mirror.verify_state_proofs_batch([(r.root, k, v, r.serialized), (r.root, k, v, r.serialized + b'\0'),
                                            (r.root, {k: v}, r.serialized), (b'short', k, v, r.serialized)])
    assert got.dtype == bool and got.tolist() == [True, False, True, False]


def test_multi_without_pairs_is_true_iff_the_root_node_is_there(rows, mirror):
    """verify_spv_proof_multi with no pairs only sets the root hash: True iff that node is
    among the proof's nodes (or the root is the blank root)"""
    V = mirror.GpuStateVerifier
    r = next(r for r in rows if r.kind == 'own' and len(r.nodes) >= 3)
    root_node = next(n for n in r.nodes if hashlib.sha3_256(n).digest() == r.root)
    without = [n for n in r.nodes if n != root_node]
    assert V.verify_state_proof_multi(r.root, {}, r.serialized, serialized=True) is True
    assert V.verify_state_proof_multi(r.root, {}, sp.serialize(without), serialized=True) is False
    assert V.verify_state_proof_multi(r.root, {}, [sp.decode(n) for n in r.nodes]) is True
    assert V.verify_state_proof_multi(r.root, {}, [sp.decode(n) for n in without]) is False
    assert V.verify_state_proof_multi(mirror.BLANK_ROOT, {}, b'\xc0', serialized=True) is True
    assert V.verify_state_proof_multi(r.root, {}, b'\xc0', serialized=True) is False
    assert mirror.verify_state_proofs_batch([(r.root, {}, r.serialized), (r.root, {}, sp.serialize(without)),
                                             (r.root, dict(r.kvs), r.serialized)]).tolist() == [True, False, True]


def test_header_self_check_under_sanitizers(tmp_path):
    """tools/hostcheck/stateproofcheck_main.cpp: its own process, built with
    AddressSanitizer + UBSan; SHA3 at every offset of exact-size buffers, the
    walk over truncated, flipped and random node bytes, and the hostile-node
    table as a case file"""
    subprocess.run(['make', '-s', '-C', sp.HC_DIR, 'stateproofcheck_asan'], check=True)
    cases = []
    for row in th.ROWS:
        proved = [th.prove_twin(row)[0].value(q) for q in range(len(th.PROVE_KEYS))]
        cases += [(row, key, val, th.verify_twin(row, key, val)) for _, key, val in th.verify_queries(row, proved)]
    lenb = lambda b: struct.pack('<Q', len(b)) + b  # noqa: E731
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(b'SVC1' + struct.pack('<I', len(cases)))
        for row, key, val, status in cases:
            fh.write(struct.pack('<Q', len(row.nodes)) + b''.join(lenb(n) for n in row.nodes) + row.root +
                     lenb(key) + lenb(val) + struct.pack('<I', status))
    r = subprocess.run([os.path.join(sp.HC_DIR, 'stateproofcheck_asan'), path], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'stateproofcheck: {} cases ok'.format(len(cases)) in r.stdout and 'stateproofcheck ok' in r.stdout
