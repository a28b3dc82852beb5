"""Merkle audit paths and consistency proofs on the CPU: the Python mirror of
MerkleVerifier, the hashlib restatement of path / chain / consistency proof,
and the per-proof routines the kernels run (csrc/pv_merkle_proof.h, built for
the host) against the reference fixture tests/golden/merkle_proofs.json."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import _merkle as mk
import _merkle_proofs as mp

HC_DIR = mp.HC_DIR


@pytest.fixture(scope='module')
def fx():
    return mp.fixture()


@pytest.fixture(scope='module')
def tree():
    return mp.LevelTree([mp.leaf(d) for d in mk.fixture()['leaves']])


def _exc_class(name):
    from plenum_gpu import exceptions
    return ValueError if name == 'ValueError' else getattr(exceptions, name)


def _check_outcome(row, fn, *args):
    """fn(*args) returns True or raises the recorded class with the recorded text"""
    if row['exc'] is None:
        assert fn(*args) is True, row['what']
        return
    with pytest.raises(_exc_class(row['exc'])) as ei:
        fn(*args)
    assert type(ei.value) is _exc_class(row['exc']), row['what']
    assert str(ei.value) == row['msg'], row['what']


def _incl_args(row):
    from plenum_gpu.merkle_proofs import STH
    return (bytes.fromhex(row['leaf_hash']), row['index'], mp.unhex(row['path']),
            STH(row['tree_size'], bytes.fromhex(row['root'])))


def _cons_args(row):
    return (row['old'], row['new'], bytes.fromhex(row['old_root']), bytes.fromhex(row['new_root']),
            mp.unhex(row['proof']))


def test_exception_hierarchy():
    """ledger/error.py:44-70"""
    from plenum_gpu.exceptions import ConsistencyError, Error, ProofError, VerifyError
    assert issubclass(VerifyError, Error) and issubclass(Error, Exception)
    assert issubclass(ConsistencyError, VerifyError) and issubclass(ProofError, VerifyError)
    assert not issubclass(ProofError, ConsistencyError) and not issubclass(ConsistencyError, ProofError)
    import plenum_gpu
    assert plenum_gpu.GpuMerkleVerifier.__name__ == 'GpuMerkleVerifier'
    assert plenum_gpu.GpuMerkleTree.__name__ == 'GpuMerkleTree'


def test_python_mirror_reproduces_every_fixture_row(fx, tree):
    from plenum_gpu.merkle_proofs import STH, GpuMerkleVerifier
    v = GpuMerkleVerifier()
    leaves = mk.fixture()['leaves']
    roots = {int(s): bytes.fromhex(h) for s, h in fx['roots'].items()}
    for r in fx['audit_paths']:
        path = mp.unhex(r['path'])
        assert v.verify_leaf_hash_inclusion(tree.lv[0][r['m']], r['m'], path, STH(r['s'], roots[r['s']])) is True
        assert v.verify_leaf_inclusion(leaves[r['m']], r['m'], path, STH(r['s'], roots[r['s']])) is True
        assert v.audit_path_length(r['m'], r['s']) == len(path)
        assert v._calculate_root_hash_from_audit_path(tree.lv[0][r['m']], r['m'], list(path), r['s']) == roots[r['s']]
    for r in fx['consistency']:
        a, b = r['a'], r['b']
        assert v.verify_tree_consistency(a, b, roots[a] if a else b'', roots[b], mp.unhex(r['proof'])) is True
    for r in fx['neg_inclusion'] + fx['wide']:
        _check_outcome(r, v.verify_leaf_hash_inclusion, *_incl_args(r))
    for r in fx['neg_consistency']:
        _check_outcome(r, v.verify_tree_consistency, *_cons_args(r))
    assert any(r['exc'] == 'ConsistencyError' for r in fx['neg_consistency'])
    assert any(r['exc'] == 'ValueError' for r in fx['neg_inclusion'])


def test_batch_methods_below_the_gpu_threshold_run_on_the_host(fx):
    """size dispatch: small batches never touch the library; one entry per item,
    None or the exception the single-item method raises"""
    from plenum_gpu import merkle_proofs
    from plenum_gpu.merkle_proofs import GpuMerkleVerifier
    v = GpuMerkleVerifier()
    rows = (fx['neg_inclusion'] + fx['wide'])[:merkle_proofs.GPU_MIN_ITEMS - 1]
    args = [_incl_args(r) for r in rows]
    got = v.verify_leaf_hash_inclusion_batch(*[list(c) for c in zip(*args)])
    for r, e in zip(rows, got):
        assert (e is None) == (r['exc'] is None), r['what']
        if e is not None:
            assert type(e) is _exc_class(r['exc']) and str(e) == r['msg'], r['what']
    rows = fx['neg_consistency']
    got = v.verify_tree_consistency_batch([_cons_args(r) for r in rows])
    for r, e in zip(rows, got):
        assert (e is None) == (r['exc'] is None), r['what']
        if e is not None:
            assert type(e) is _exc_class(r['exc']) and str(e) == r['msg'], r['what']


def test_restatement_reproduces_the_fixture(fx, tree):
    for r in fx['audit_paths']:
        assert [h.hex() for h in tree.audit_path(r['m'], r['s'])] == r['path'], (r['m'], r['s'])
    for r in fx['consistency']:
        assert [h.hex() for h in tree.consistency_proof(r['a'], r['b'])] == r['proof'], (r['a'], r['b'])
    for s, h in fx['roots'].items():
        assert tree.root(int(s)).hex() == h, s
    d = hashlib.sha256()
    for s in range(1, 71):
        for m in range(s):
            d.update(b''.join(tree.audit_path(m, s)))
    assert d.hexdigest() == fx['digest_paths_le70']
    d = hashlib.sha256()
    for b in range(1, 71):
        for a in range(1, b + 1):
            d.update(b''.join(tree.consistency_proof(a, b)))
    assert d.hexdigest() == fx['digest_cons_le70']
    # and the RFC 6962 recursions, which share no code with the level-wise form
    lh = tree.lv[0]
    for s in (1, 2, 3, 6, 7, 8, 13, 33, 70):
        for m in range(s):
            assert tree.audit_path(m, s) == mp.rfc_path(m, lh[:s])
        for a in range(1, s + 1):
            assert tree.consistency_proof(a, s) == mp.rfc_proof(a, lh[:s])


# ------------------------------------------------- the header's routines on the host
@pytest.fixture(scope='module')
def lib():
    return mp.host_lib()


host_inclusion, host_consistency = mp.host_inclusion, mp.host_consistency


def test_header_routines_give_the_fixture_verdicts(lib, fx):
    seen = set()
    for r in fx['neg_inclusion'] + fx['wide']:
        if mp.negative(r):
            assert r['exc'] == 'ValueError'
            continue
        want, comp, stop = mp.expect_inclusion(r)
        st, got_comp, got_stop = host_inclusion(lib, *[a for a in _incl_args(r)[:2]], r['tree_size'],
                                                mp.unhex(r['path']), bytes.fromhex(r['root']))
        assert st == want, r['what']
        if comp is not None:
            assert got_comp == comp, r['what']
        if stop is not None:
            assert got_stop == stop, r['what']
        seen.add(st)
    assert seen == {mp.OK, mp.BAD_RANGE, mp.TOO_SHORT, mp.TOO_LONG, mp.ROOT_MISMATCH}
    seen = set()
    for r in fx['neg_consistency']:
        if mp.negative(r):
            assert r['exc'] == 'ValueError'
            continue
        want, c0, c1 = mp.expect_consistency(r)
        st, g0, g1 = host_consistency(lib, *_cons_args(r))
        assert st == want, r['what']
        if c0 is not None:
            assert g0 == c0, r['what']
        if c1 is not None:
            assert g1 == c1, r['what']
        seen.add(st)
    assert seen == {mp.OK, mp.BAD_RANGE, mp.TOO_SHORT, mp.ROOT_MISMATCH, mp.INCONSISTENT}


def test_header_routines_generate_the_fixture_paths_and_proofs(lib, fx, tree):
    t = lib.mc_tree_new(b''.join(tree.lv[0]), tree.size)
    try:
        depth = lib.mc_tree_depth(t)
        assert depth == len(tree.lv) - 1 == 11
        out, root = np.zeros((depth + 1, 32), np.uint8), np.zeros(32, np.uint8)
        for r in fx['audit_paths']:
            n = lib.mc_audit_path(t, r['m'], r['s'], out.ctypes.data, root.ctypes.data)
            assert [out[j].tobytes().hex() for j in range(n)] == r['path'], (r['m'], r['s'])
            assert root.tobytes().hex() == fx['roots'][str(r['s'])]
        for r in fx['consistency']:
            n = lib.mc_cons_proof(t, r['a'], r['b'], out.ctypes.data)
            assert [out[j].tobytes().hex() for j in range(n)] == r['proof'], (r['a'], r['b'])
        d = hashlib.sha256()
        for s in range(1, 71):
            for m in range(s):
                n = lib.mc_audit_path(t, m, s, out.ctypes.data, root.ctypes.data)
                d.update(out[:n].tobytes())
        assert d.hexdigest() == fx['digest_paths_le70']
        d = hashlib.sha256()
        for b in range(1, 71):
            for a in range(1, b + 1):
                n = lib.mc_cons_proof(t, a, b, out.ctypes.data)
                d.update(out[:n].tobytes())
        assert d.hexdigest() == fx['digest_cons_le70']
        for m, s in [(0, 0), (5, 5), (0, tree.size + 1)]:   # refused, not clamped
            assert lib.mc_audit_path(t, m, s, out.ctypes.data, root.ctypes.data) == 0xffffffff
        for a, b in [(3, 2), (1, tree.size + 1)]:
            assert lib.mc_cons_proof(t, a, b, out.ctypes.data) == 0xffffffff
    finally:
        lib.mc_tree_free(t)


def test_walk_restatements_give_the_fixture_verdicts(lib, fx, tree):
    """tests/_merkle_device.py ref_inclusion / ref_consistency (the expectation
    of the device-buffer GPU tests' class tables) on every fixture row: the
    fixture's verdict, and what the header's routines leave in their outputs"""
    import _merkle_device as md
    for r in fx['audit_paths']:
        rt = bytes.fromhex(fx['roots'][str(r['s'])])
        assert md.ref_inclusion(tree.lv[0][r['m']], r['m'], r['s'], mp.unhex(r['path']), rt) == (mp.OK, rt, 0)
    for r in fx['neg_inclusion'] + fx['wide']:
        if mp.negative(r):
            continue
        args = (bytes.fromhex(r['leaf_hash']), r['index'], r['tree_size'], mp.unhex(r['path']),
                bytes.fromhex(r['root']))
        got = md.ref_inclusion(*args)
        want = mp.expect_inclusion(r)
        assert all(w is None or w == g for w, g in zip(want, got)), r['what']
        assert got == host_inclusion(lib, *args), r['what']
    for r in fx['consistency']:
        a, b = r['a'], r['b']
        rb = bytes.fromhex(fx['roots'][str(b)])
        ra = bytes.fromhex(fx['roots'][str(a)]) if a else rb
        assert md.ref_consistency(a, b, ra, rb, mp.unhex(r['proof']))[0] == mp.OK
    for r in fx['neg_consistency']:
        if mp.negative(r):
            continue
        got = md.ref_consistency(*_cons_args(r))
        want = mp.expect_consistency(r)
        assert all(w is None or w == g for w, g in zip(want, got)), r['what']
        assert got == host_consistency(lib, *_cons_args(r)), r['what']


def test_request_builders_weave_valid_and_refused(tree):
    """tests/_merkle_device.py path_requests / proof_requests: alternating, the
    edges and the 64-bit traps present, valid exactly where LevelTree accepts"""
    import _merkle_device as md
    n = 1000
    for k in (1, 63, 64, 65, 257, 1000):
        for phase in (0, 1):
            for reqs, ok in ((md.path_requests(n, k, phase), lambda a, b: 0 <= a < b <= n),
                             (md.proof_requests(n, k, phase), lambda a, b: 0 <= a <= b <= n)):
                assert len(reqs) == k
                assert [v for _, _, v in reqs] == [(i + phase) % 2 == 0 for i in range(k)]
                assert all(ok(a, b) == v for a, b, v in reqs)
                assert all(0 <= a < 2 ** 64 and 0 <= b < 2 ** 64 for a, b, _ in reqs)
    paths = {(a, b) for a, b, v in md.path_requests(n, 1000, 0) if v}
    assert {(0, 1), (0, n), (n - 1, n), (511, 512), (512, 513), (0, 513), (255, 511)} <= paths
    assert len(paths - set(md.path_edges(n))) >= 64
    proofs = {(a, b) for a, b, v in md.proof_requests(n, 1000, 0) if v}
    assert {(0, 0), (0, n), (n, n), (1, 1), (511, 512), (513, n), (512, 513), (255, 257)} <= proofs
    assert len(proofs - set(md.proof_edges(n))) >= 64
    # every trap is out of range as 64 bits and in range once truncated to 32
    low = 2 ** 32 - 1
    assert sum(1 for a, b in md.path_refusals(n) if 0 <= (a & low) < (b & low) <= n) >= 4
    assert sum(1 for a, b in md.proof_refusals(n) if 0 <= (a & low) <= (b & low) <= n) >= 4
    assert {(2 ** 64 - 1, n), (0, 2 ** 63)} <= set(md.path_refusals(n))
    assert all(x[0] < 2 ** 64 and x[1] < 2 ** 64 for x in md.path_refusals(n) + md.proof_refusals(n))


def test_second_trip_class_tables(lib, fx):
    """the class tables the GPU test repeats past one grid of the proof kernels
    (tests/_merkle_device.py) against the fixture, LevelTree's RFC 6962
    recursions and the header's routines on the host"""
    import _merkle_device as md
    lh = [bytes.fromhex(h) for h in mk.fixture()['leaf_hashes']]
    t5 = md.small_tree(lh)
    n = t5.size
    assert n == 5 and len(t5.lv) - 1 == 3
    for s in range(1, n + 1):
        assert t5.root(s).hex() == fx['roots'][str(s)]
    fx_paths = {(r['m'], r['s']): r['path'] for r in fx['audit_paths']}
    fx_proofs = {(r['a'], r['b']): r['proof'] for r in fx['consistency']}
    ht = lib.mc_tree_new(b''.join(t5.lv[0]), n)
    try:
        assert lib.mc_tree_depth(ht) == 3
        out, root = np.zeros((4, 32), np.uint8), np.zeros(32, np.uint8)
        pc = md.path_classes(t5)
        assert len(pc) == 18 and sum(p is None for _, _, p, _ in pc) == 3
        for m, s, path, rt in pc:
            got = lib.mc_audit_path(ht, m, s, out.ctypes.data, root.ctypes.data)
            if path is None:
                assert got == md.REFUSED and rt is None and not (0 <= m < s <= n)
                continue
            assert got == len(path) <= 3 and out[:got].tobytes() == b''.join(path) and root.tobytes() == rt
            assert path == mp.rfc_path(m, lh[:s]) and rt == mp.rfc_mth(lh[:s])
            if (m, s) in fx_paths:
                assert [h.hex() for h in path] == fx_paths[(m, s)]
        assert {(m, s) for m, s, p, _ in pc if p is not None} == {(m, s) for s in range(1, 6) for m in range(s)}
        cc = md.proof_classes(t5)
        assert len(cc) == 23 and sum(p is None for _, _, p in cc) == 2
        for a, b, proof in cc:
            got = lib.mc_cons_proof(ht, a, b, out.ctypes.data)
            if proof is None:
                assert got == md.REFUSED and not (0 <= a <= b <= n)
                continue
            assert got == len(proof) <= 4 and out[:got].tobytes() == b''.join(proof)
            if a >= 1:
                assert proof == mp.rfc_proof(a, lh[:b])
            if (a, b) in fx_proofs:
                assert [h.hex() for h in proof] == fx_proofs[(a, b)]
    finally:
        lib.mc_tree_free(ht)
    ic = md.incl_classes(t5)
    assert [w[0] for _, w in ic] == [mp.OK] * 15 + [mp.ROOT_MISMATCH, mp.TOO_SHORT, mp.TOO_LONG, mp.BAD_RANGE]
    for it, want in ic:
        assert host_inclusion(lib, *it) == want, it[1:3]
        if want[0] == mp.OK:
            assert want[1] == t5.root(it[2]) == it[4]
    assert ic[16][1][2] == 1 and ic[15][1][1] == t5.root(n)     # stopped at node 1; the true root computed
    cc = md.cons_classes(t5)
    assert [w[0] for _, w in cc] == [mp.OK] * 21 + [mp.ROOT_MISMATCH, mp.TOO_SHORT, mp.BAD_RANGE, mp.INCONSISTENT]
    for it, want in cc:
        assert host_consistency(lib, *it) == want, it[:2]
    assert cc[24][1][2] == t5.root(n) and cc[24][1][1] == t5.root(3) != cc[24][0][2]


def test_header_self_check_under_sanitizers():
    """tools/hostcheck/merklecheck_main.cpp: its own process, built with
    AddressSanitizer + UBSan; every path and proof of trees of 1..130 leaves
    generated, verified and verified again mutated"""
    subprocess.run(['make', '-s', '-C', HC_DIR, 'merklecheck_asan'], check=True)
    r = subprocess.run([os.path.join(HC_DIR, 'merklecheck_asan')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout
