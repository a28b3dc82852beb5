"""Pruning the resident trie store on the GPU (pv_state_store_prune: k_trie_prune_seed /
k_trie_prune_level, the keep-flag scans, k_trie_prune_copy and k_trie_store_rehash into fresh
buffers) against the host build of csrc/pv_trie_prune.h (tools/hostcheck/stateprunecheck.cpp) on
everything the ABI exposes, against the sets the fixtures recorded from the reference keep
reachable, and through the proofs and updates served at the kept roots afterwards.  The stores are
those of tests/test_state_prune_host.py (tests/_state_prune.py)."""
import ctypes
import random

import numpy as np
import pytest

import _state_apply as sa
import _state_build as sb
import _state_prune as pr
import _state_store as ss

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -22
SP_OK, SP_NODE_MISSING, SP_MALFORMED = 0, 2, 3


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


def last_error():
    from plenum_gpu import _native as nat
    return nat.load().pv_last_error().decode()


def raw_prune(store_id, roots, apply, digest_cap=None, want_status=True):
    """pv_state_store_prune as the ABI has it -> (rc, root_status, n_kept, bytes_kept, n_missing, digests)"""
    from plenum_gpu import _native as nat
    lib = nat.load()
    rts = np.frombuffer(b''.join(roots) + b'\0', np.uint8).copy()
    status = np.full(max(len(roots), 1), 0xee, np.uint8)
    kept, nbytes, missing = (ctypes.c_uint64(0) for _ in range(3))
    dig = None if digest_cap is None else np.zeros((max(digest_cap, 1), 32), np.uint8)
    u8p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731
    rc = lib.pv_state_store_prune(store_id, u8p(rts), len(roots), apply, u8p(status) if want_status else None,
                                  ctypes.byref(kept), ctypes.byref(nbytes), ctypes.byref(missing), u8p(dig),
                                  digest_cap or 0)
    return rc, [int(x) for x in status[:len(roots)]], kept.value, nbytes.value, missing.value, dig


def check_gpu_equals_host(mod, adds, roots):
    """a GPU store and a host twin filled by the same add calls and pruned to the same roots agree
    on root_status, the four counts, kept_digests and info(), in the reporting call and after the
    compaction -> (the still open GPU store, the host twin's dict)"""
    st = mod.GpuStateStore(node_hint=1)
    try:
        with pr.HostStore() as hs:
            for nodes in adds:
                assert st.add_nodes(nodes) == hs.add_nodes(nodes)
            assert st.info() == hs.info()
            before = st.info()
            rep, h_rep = st.reachable(roots, want_digests=True), hs.prune(roots, apply=False)
            assert h_rep['rc'] == pr.PR_OK and st.info() == before
            for k in ('n_kept', 'bytes_kept', 'n_missing', 'root_status', 'digests'):
                assert rep[k] == h_rep[k], k
            got, want = st.prune(roots, want_digests=True), hs.prune(roots)
            assert want['rc'] == pr.PR_OK
            for k in ('n_kept', 'bytes_kept', 'n_missing', 'root_status', 'digests'):
                assert got[k] == want[k], k
            assert st.info() == hs.info()
            assert st.info() == {'n_nodes': want['n_kept'], 'n_unique': want['n_kept'], 'n_bytes': want['bytes_kept'],
                                 'n_slots': max(64, 1 << (2 * want['n_kept'] - 1).bit_length() if want['n_kept'] else 64)}
    except BaseException:
        st.close()
        raise
    return st, want


def same_proofs(a, b):
    return ((a.status == b.status).all() and (a.node_count == b.node_count).all() and
            (a.proof_off == b.proof_off).all() and (a.val_rel == b.val_rel).all() and
            (a.val_len == b.val_len).all() and (a.blob == b.blob).all())


# ------------------------------------------------------------------ 1. the fixture cases
@pytest.mark.parametrize('name', [n for n, _, _ in pr.fixture_cases()])
def test_fixture_case_keeps_what_the_reference_reaches(mod, name, monkeypatch):
    from plenum_gpu import state_proofs
    monkeypatch.setattr(state_proofs, 'GPU_MIN_ITEMS', 0)
    c = next(c for n, _, c in pr.fixture_cases() if n == name)
    step = 'update_state' if name.startswith('up/') else 'apply_batch'
    before = c.batches[-2].reachable if len(c.batches) > 1 else c.base_reachable
    for keep_two in (False, True):
        with mod.GpuStateStore(node_hint=1) as st:
            root = st.build_state(c.base)
            assert root == c.base_root
            roots, state, gone = [root], dict(c.base), set()
            for b in c.batches:
                root = getattr(st, step)(root, b.items)
                assert root == b.root
                roots.append(root)
                for k, v in b.items:
                    if v is None:
                        state.pop(k, None)
                        gone.add(k)
                    else:
                        state[k] = v
                        gone.discard(k)
            keep = roots[-2:] if keep_two else roots[-1:]
            got = st.prune(keep, want_digests=True)
            want = c.batches[-1].reachable | (before if keep_two else set())
            assert set(got['digests']) == want and got['n_kept'] == len(want) and got['n_missing'] == 0
            assert st.info()['n_nodes'] == st.info()['n_unique'] == len(want)
            if keep_two:
                continue
            keys, absent = list(state), sorted(gone)
            if root == mod.BLANK_ROOT:
                assert st.info()['n_nodes'] == 0
            res = st.generate_state_proofs_batch([(root, k) for k in keys + absent])
            assert all(r is not None for r in res)
            assert [r[1] for r in res] == [state[k] for k in keys] + [None] * len(absent)
            if res:
                ok = state_proofs.verify_state_proofs_batch(
                    [(root, k, state.get(k), r[0]) for k, r in zip(keys + absent, res)])
                assert ok.all()


@pytest.mark.parametrize('name', ['up/mixed300', 'rm/mixed300', 'wave63', 'wave64', 'wave65', 'chain', 'mixed4096'])
def test_shape_equals_host_twin(mod, name):
    nodes, roots = pr.filled(name)
    for keep in (roots[-1:], roots[-2:]):
        st, want = check_gpu_equals_host(mod, [nodes], keep)
        st.close()
        assert want['digests'] == pr.Want(nodes, keep).digests


# ------------------------------------------------------------------ 2. walk equivalence
def test_walks_at_kept_roots_are_byte_identical_and_dropped_roots_are_gone(mod):
    base = sb.mixed_pairs(4096, 77)
    rng = random.Random(77)
    with mod.GpuStateStore(node_hint=1) as st:
        roots = [mod._build_gpu(base, st._id)[0]]
        state, touched = dict(base), []
        for i in range(8):
            batch = sa.batch_onto(sorted(state.items()), 64, 700 + i, removals=0.5)
            roots.append(mod._apply_gpu(st._id, roots[-1], batch)[0])
            sa.state_after(state, batch)
            touched += [k for k, _ in batch]
        assert len(set(roots)) == 9
        kept = [roots[0], roots[5], roots[8]]
        pool = [k for k, _ in base] + touched + [sb.sha3(b'absent %d' % i) for i in range(256)]
        keys = [rng.choice(pool) for _ in range(4096)]
        ridx = [rng.randrange(3) for _ in range(4096)]
        before = st.prove(kept, ridx, keys)
        assert (before.status == SP_OK).all() and (before.val_len == 0).any() and (before.val_len > 0).any()
        n_before = st.info()['n_nodes']
        got = st.prune(kept)
        assert got['root_status'] == [SP_OK] * 3 and got['n_missing'] == 0 and got['n_kept'] < n_before
        after = st.prove(kept, ridx, keys)
        assert same_proofs(before, after)
        for r in (roots[1], roots[4], roots[7]):
            assert int(st.prove([r], None, [keys[0]]).status[0]) == SP_NODE_MISSING
            with pytest.raises(KeyError):
                st.generate_state_proof(keys[0], r)


# ------------------------------------------------------------------ 3. life goes on
def test_apply_add_and_a_second_prune_after_a_prune(mod):
    nodes, roots = pr.filled('rm/mixed300')
    c = next(c for n, _, c in pr.fixture_cases() if n == 'rm/mixed300')
    state = dict(c.base)
    for b in c.batches:
        for k, v in b.items:
            state[k] = v
            if v is None:
                del state[k]
    batch = [(k, None) for k in sorted(state)[:20]] + [(b'after the prune %d' % i, b'v' * (i + 1)) for i in range(30)]
    with mod.GpuStateStore(node_hint=1) as st, mod.GpuStateStore(node_hint=1) as twin:
        st.add_nodes(nodes)
        twin.add_nodes(nodes)
        first = st.prune(roots[-1:], want_digests=True)
        info = st.info()
        again = st.prune(roots[-1:], want_digests=True)                  # nothing left to drop
        assert again == first and st.info() == info
        new = st.apply_batch(roots[-1], batch)
        assert new == twin.apply_batch(roots[-1], batch) != roots[-1]
        keys = [k for k, _ in batch]
        a, b = st.prove([new], [0] * len(keys), keys), twin.prove([new], [0] * len(keys), keys)
        assert same_proofs(a, b)
        # the shrunken buffers grow again: more nodes and bytes than the capacities left by the prune
        extra, _ = pr.ext_chain(4 * first['n_kept'] + 70, b'grow')
        assert sum(len(x) for x in extra) > first['bytes_kept']
        n0 = st.info()
        assert st.add_nodes(extra) == len(extra)
        n1 = st.info()
        assert n1['n_nodes'] == n0['n_nodes'] + len(extra) and n1['n_slots'] > n0['n_slots']
        assert n1['n_bytes'] == n0['n_bytes'] + sum(len(x) for x in extra)
        # the capacities were the powers of two holding the kept data: under twice of it
        assert n1['n_bytes'] > 2 * first['bytes_kept'] and n1['n_nodes'] > 2 * first['n_kept']
        a = st.prove([new, pr.sha3(extra[-1])], [0] * len(keys) + [1], keys + [b'\x11'])
        assert same_proofs(st.prove([new], [0] * len(keys), keys), b) and int(a.status[-1]) == SP_OK
        assert int(a.node_count[-1]) == 3                                # key 0x11: two extensions, then a mismatch


# ------------------------------------------------------------------ 4. edges
@pytest.mark.parametrize('n', [1, 32, 33, 63, 64, 65])
def test_kept_counts_at_the_table_wave_and_bitmap_word_edges(mod, n):
    junk, _ = pr.ext_chain(70, b'junk')
    chain, root = pr.ext_chain(n, b'kept')
    st, want = check_gpu_equals_host(mod, [junk[:33] + chain, junk[33:] + chain], [root])
    with st:
        assert want['n_kept'] == n and want['digests'] == [pr.sha3(x) for x in chain]
        assert st.info()['n_slots'] == (64 if n <= 32 else 128 if n <= 64 else 256)
        pr_ = st.prove([root], None, [b'\x11' * 40])
        assert int(pr_.status[0]) == SP_OK and int(pr_.node_count[0]) == n


def test_duplicate_ids_are_dropped(mod):
    nodes, roots = pr.filled('up/mixed300')
    st, want = check_gpu_equals_host(mod, [nodes, nodes[::-1], nodes[:100]], roots[-1:])
    st.close()
    assert want['n_kept'] == pr.Want(nodes, roots[-1:]).n_kept


def test_two_roots_sharing_all_but_one_path(mod):
    base = sb.mixed_pairs(300, 31)
    b0 = sb.host_build(base)
    with sa.HostStore() as hs:
        hs.add_nodes(b0.nodes())
        b1 = hs.apply(b0.root, [(base[150][0], sb._encode(b'one key changed'))])
    nodes = b0.nodes() + b1.nodes()
    st, want = check_gpu_equals_host(mod, [nodes], [b0.root, b1.root])
    st.close()
    assert want['n_kept'] == len(set(nodes)) and 0 < b1.n_nodes < 12 and b1.n_nodes < b0.n_nodes


def test_blank_roots(mod):
    nodes, roots = pr.filled('rm/mixed300')
    st, want = check_gpu_equals_host(mod, [nodes], [mod.BLANK_ROOT])
    with st:
        assert (want['n_kept'], want['root_status']) == (0, [SP_OK])
        assert st.info() == {'n_nodes': 0, 'n_unique': 0, 'n_bytes': 0, 'n_slots': 64}
        assert st.generate_state_proof(b'k', mod.BLANK_ROOT, serialize=True) == b'\xc0'
        assert st.add_nodes(nodes[:10]) == 10                            # an emptied store takes nodes again
    st, want = check_gpu_equals_host(mod, [nodes], [mod.BLANK_ROOT, roots[-1], mod.BLANK_ROOT])
    st.close()
    assert want['n_kept'] == pr.Want(nodes, roots[-1:]).n_kept and want['root_status'] == [SP_OK] * 3


def test_the_reporting_call_leaves_the_store_and_its_proofs_alone(mod):
    nodes, roots = pr.filled('rm/mixed300')
    keys = [sb.sha3(b'%d' % i) for i in range(8)]
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(nodes)
        info, proofs = st.info(), st.prove(roots, list(range(len(roots))), keys[:len(roots)])
        rep = st.reachable(roots[-1:], want_digests=True)
        assert rep['n_kept'] == pr.Want(nodes, roots[-1:]).n_kept and rep['digests'] == pr.Want(nodes, roots[-1:]).digests
        rc, status, kept, nbytes, missing, _ = raw_prune(st._id, roots[-1:], 0, want_status=False)
        assert (rc, kept, nbytes, missing) == (OK, rep['n_kept'], rep['bytes_kept'], 0)
        assert st.info() == info and same_proofs(proofs, st.prove(roots, list(range(len(roots))), keys[:len(roots)]))


# ------------------------------------------------------------------ 5. values, partial stores, malformed nodes
def test_a_value_that_looks_like_a_reference_is_not_followed(mod):
    nodes, root, dropped = pr.value_trap()
    st, want = check_gpu_equals_host(mod, [nodes], [root])
    with st:
        assert want['n_kept'] == 2 and not (set(want['digests']) & dropped)
        for d in dropped:
            assert int(st.prove([d], None, [b'k']).status[0]) == SP_NODE_MISSING
        got = st.prove([root], [0, 0], [b'\x31\x23', b''])
        assert (got.status == SP_OK).all() and got.value(0) in dropped and got.value(1) in dropped


def test_a_store_filled_from_proofs_keeps_its_proofs(mod):
    rows = [r for r in ss.proof_rows() if r.kind == 'own']
    trie = max(ss.tries(), key=lambda t: len(ss.tries()[t][1]))
    rows = [r for r in rows if r.trie == trie][:4]
    root, keys = rows[0].root, [r.kvs[0][0] for r in rows]
    nodes = []
    with mod.GpuStateStore(node_hint=1) as st:
        for r in rows:
            st.add_serialized_proof(r.serialized)
            nodes += [n for n in r.nodes]
        before = st.prove([root], [0] * len(keys), keys)
        assert (before.status == SP_OK).all()
        got = st.prune([root], want_digests=True)
        assert got['n_missing'] > 0 and set(got['digests']) == {pr.sha3(n) for n in nodes}
        assert got['n_missing'] == pr.Want(nodes, [root]).n_missing
        assert same_proofs(before, st.prove([root], [0] * len(keys), keys))


def test_a_malformed_inline_child_keeps_its_parent(mod):
    nodes, root, hidden, leaf = pr.malformed_parent()
    st, want = check_gpu_equals_host(mod, [nodes[:2], nodes[2:]], [root])
    with st:
        assert set(want['digests']) == {root, leaf}
        assert int(st.prove([root], None, [b'\x00']).status[0]) == SP_MALFORMED
        assert int(st.prove([hidden], None, [b'\x00']).status[0]) == SP_NODE_MISSING
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(nodes)
        assert int(st.prove([root], None, [b'\x00']).status[0]) == SP_MALFORMED


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_store_unchanged(mod):
    nodes, roots = pr.filled('rm/mixed300')
    wrong = pr.sha3(b'no such root')
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(nodes)
        info = st.info()
        proofs = st.prove(roots[:1], None, [b'k'])
        assert raw_prune(0x7fff0000, roots[-1:], 1)[0] == EINVAL and 'no state store' in last_error()
        assert raw_prune(st._id, [], 1)[0] == EINVAL and 'free the store' in last_error()
        rc, status, kept, _, _, _ = raw_prune(st._id, [roots[-1], wrong], 1)
        assert (rc, status) == (EINVAL, [SP_OK, SP_NODE_MISSING]) and 'root 1 ' in last_error()
        assert kept == pr.Want(nodes, roots[-1:]).n_kept
        with pytest.raises(KeyError):
            st.prune([roots[-1], wrong])
        assert st.reachable([wrong])['root_status'] == [SP_NODE_MISSING]
        for apply in (0, 1):
            rc, _, kept, _, _, dig = raw_prune(st._id, roots[-1:], apply, digest_cap=kept - 1)
            assert rc == EINVAL and last_error().startswith('digest capacity too small')
            assert kept == pr.Want(nodes, roots[-1:]).n_kept and not dig.any()
        with pytest.raises(ValueError):
            st.prune([])
        assert st.info() == info and same_proofs(proofs, st.prove(roots[:1], None, [b'k']))
        sid = st._id
    assert raw_prune(sid, roots[-1:], 1)[0] == EINVAL and 'no state store' in last_error()


def test_the_timed_prune_is_the_same_prune(mod):
    from plenum_gpu import _native as nat
    lib = nat.load()
    nodes, roots = pr.filled('up/mixed300')
    want = pr.Want(nodes, roots[-2:])
    rts = np.frombuffer(b''.join(roots[-2:]), np.uint8).copy()
    kept, nbytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ms = [ctypes.c_float(-1.0) for _ in range(3)]
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(nodes)
        rc = lib.pv_time_state_store_prune(st._id, rts.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(kept),
                                           ctypes.byref(nbytes), *[ctypes.byref(x) for x in ms])
        assert rc == OK, last_error()
        assert (kept.value, nbytes.value) == (want.n_kept, want.bytes_kept) and st.info() == want.info()
        assert all(0.0 <= x.value < 1000.0 for x in ms)
        assert st.reachable(roots[-2:], want_digests=True)['digests'] == want.digests
        rc = lib.pv_time_state_store_prune(st._id, rts.ctypes.data_as(ctypes.c_void_p), 2, None, None, None, None, None)
        assert rc == EINVAL and st.info() == want.info()


def test_inline_nesting_up_to_the_limit_and_the_refusal_past_it(mod):
    nodes, root, leaf = pr.nested(pr.MAX_INLINE)
    st, want = check_gpu_equals_host(mod, [nodes], [root])
    st.close()
    assert set(want['digests']) == {root, leaf}
    nodes, root, leaf = pr.nested(pr.MAX_INLINE + 1)
    with mod.GpuStateStore(node_hint=1) as st:
        st.add_nodes(nodes)
        info = st.info()
        for apply in (0, 1):
            rc, status, _, _, _, _ = raw_prune(st._id, [root], apply)
            assert (rc, status) == (EINVAL, [SP_OK]) and 'nest' in last_error()
            assert st.info() == info
        assert int(st.prove([root], None, [b'\x11' * 5]).status[0]) == SP_OK    # still served
        assert st.prune([leaf])['n_kept'] == 1                                  # the junk node not reached: no refusal
