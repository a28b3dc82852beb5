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


def test_header_self_check_under_sanitizers():
    """tools/hostcheck/merklecheck_main.cpp: its own process, built with
    AddressSanitizer + UBSan; every path and proof of trees of 1..130 leaves
    generated, verified and verified again mutated"""
    subprocess.run(['make', '-s', '-C', HC_DIR, 'merklecheck_asan'], check=True)
    r = subprocess.run([os.path.join(HC_DIR, 'merklecheck_asan')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout
