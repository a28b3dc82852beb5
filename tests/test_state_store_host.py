"""The resident trie node store on the CPU: the Python mirror
(plenum_gpu.state_store.walk_host) against the reference fixture
tests/golden/state_proofs.json, and the routines the kernels run
(csrc/pv_trie_store.h built for the host, tools/hostcheck/statestorecheck.cpp)
against the mirror, byte for byte.

A scenario is (add batches, roots, root_idx, keys, max_nodes).  Every scenario is
run on the host build and on the mirror by its own test, and all of them once
more by statestorecheck_asan, a program of its own under AddressSanitizer + UBSan
with every buffer at its exact size."""
import os
import subprocess

import pytest

import _state_proofs as sp
import _state_store as ss
import _trie_hostile as th


def run_host(sc):
    """-> (host Result, mirror Result, HostStore) of one scenario; the two must agree"""
    batches, roots, ridx, keys, max_nodes = sc
    st = ss.HostStore(1)
    for b in batches:
        st.add(b)
    got = st.prove(roots, ridx, keys, max_nodes)
    want = ss.mirror_prove(st.db, st.id_of, roots, ridx, keys, max_nodes)
    assert got.rc == 0
    assert got.same(want) is None, got.same(want)
    info = st.info()
    assert info['n_nodes'] == sum(len(b) for b in batches) and info['n_unique'] == len(st.db)
    assert info['n_nodes'] <= info['n_slots'] // 2
    return got, want, st


# ------------------------------------------------------------------ 1. fixture, mirror
def test_mirror_reproduces_every_reference_proof():
    from plenum_gpu.state_proofs import GpuStateVerifier, rlp_split_list
    from plenum_gpu.state_store import walk_host
    tr = ss.tries()
    assert sorted(len(db) for _, db in tr.values()) == [2, 2, 8, 10, 343]
    rows = ss.proof_rows()
    assert len(rows) == 409 and sum(r.kind == 'own' for r in rows) == 331
    depths = set()
    for r in rows:
        root, db = tr[r.trie]
        key, value = r.kvs[0]
        st, nodes, got, proof, rel = walk_host(db, r.root, key)
        assert st == ss.OK, (r.trie, r.kind)
        assert sorted(nodes) == sorted(r.nodes), (r.trie, r.kind)        # the reference's multiset
        split = [proof[b:e] for b, e in rlp_split_list(proof)]
        assert split == nodes[::-1] and ss.sha3(split[-1]) == r.root      # root last
        assert got == sp.encode_value(value) and proof[rel:rel + len(got)] == got
        assert GpuStateVerifier.verify_state_proof(r.root, key, value, proof, serialized=True) is True
        depths.add(len(nodes))
    assert min(depths) == 1 and max(depths) == 9


def test_mirror_blank_root_and_missing_nodes():
    from plenum_gpu.state_proofs import BLANK_ROOT, GpuStateVerifier
    from plenum_gpu.state_store import walk_host
    assert walk_host({}, BLANK_ROOT, b'k') == (ss.OK, [], b'', b'\xc0', 0)
    assert GpuStateVerifier.verify_state_proof(BLANK_ROOT, b'k', None, b'\xc0', serialized=True) is True
    assert walk_host({}, b'\x11' * 32, b'k') == (ss.NODE_MISSING, [], b'', None, 0)
    for sc in ss.sc_missing()[:-1]:
        (nodes,), (root,), _, (key,), _ = sc
        db = {ss.sha3(n): n for n in nodes}
        st, got, _, proof, _ = walk_host(db, root, key)
        assert st == ss.NODE_MISSING and proof is None


# ------------------------------------------------------------------ 2. host build == mirror
@pytest.mark.parametrize('name', ['fixture', 'built'])
def test_host_build_equals_mirror(name):
    got, want, _ = run_host(ss.SCENARIOS[name]())
    assert (got.status == ss.OK).all()
    assert (got.val_len == 0).any() and (got.val_len > 0).any()      # absent and present keys
    if name == 'fixture':
        rows = ss.proof_rows()
        for q, r in enumerate(rows):
            assert got.value(q) == sp.encode_value(r.kvs[0][1])
            assert int(got.node_count[q]) == len(r.nodes)


def test_host_sizing_call_and_small_capacity():
    batches, roots, ridx, keys, _ = ss.sc_built()
    st = ss.HostStore(1)
    st.add(batches[0])
    full = st.prove(roots, ridx, keys)
    sizing = st.prove(roots, ridx, keys, sizing=True)
    assert sizing.rc == 0 and (sizing.proof_off == full.proof_off).all() and (sizing.status == full.status).all()
    short = st.prove(roots, ridx, keys, proof_cap=int(full.proof_off[-1]) - 1)
    assert short.rc == -22 and (short.proof_off == full.proof_off).all()


# ------------------------------------------------------------------ 3. table edges
def _digest(word0, tail):
    return int(word0).to_bytes(4, 'little') + ss.sha3(b'tail%d' % tail)[:28]


TABLE_BATCHES = {}      # the raw-digest batches of the tests below, for the sanitizer run


def _table_store(name):
    """a HostStore whose add_digests calls are recorded under `name`"""
    st = ss.HostStore(1)
    TABLE_BATCHES[name] = []
    plain = st.add_digests

    def add_digests(digests):
        TABLE_BATCHES[name].append(('digests', list(digests)))
        return plain(digests)
    st.add_digests = add_digests
    return st


def test_table_equal_first_words_and_wrapping_chain():
    st = _table_store('chains')
    same = [_digest(0x12345607, t) for t in range(3)]            # one first word, three tails
    wrap = [_digest(0xabcdef3f + 64 * t, t) for t in range(3)]   # start slot 63 of 64: 63, 0, 1
    assert st.add_digests(same + wrap) == 6 and st.info()['n_slots'] == 64
    assert [st.find(d) for d in same + wrap] == list(range(6))
    assert [st.slot_of(i) for i in range(3)] == [7, 8, 9]
    assert [st.slot_of(i) for i in range(3, 6)] == [63, 0, 1]
    assert st.find(_digest(0x12345607, 99)) == -1 and st.find(_digest(0xabcdef3f, 99)) == -1
    assert st.find(_digest(0x00000002, 0)) == -1                 # an empty start slot


def test_table_growth_at_half_load():
    st = _table_store('growth')
    d = [ss.sha3(b'n%d' % i) for i in range(40)]
    assert st.add_digests(d[:31]) == 31 and st.info()['n_slots'] == 64
    assert st.add_digests(d[31:32]) == 1
    assert st.info() == {'n_nodes': 32, 'n_unique': 32, 'n_bytes': 0, 'n_slots': 64}    # exactly slots / 2
    assert st.add_digests(d[32:33]) == 1 and st.info()['n_slots'] == 128                # slots / 2 + 1
    assert [st.find(x) for x in d[:33]] == list(range(33))
    assert st.add_digests(d[33:] + d[:40]) == 7 and st.info()['n_slots'] == 256         # two doublings in one add
    assert [st.find(x) for x in d] == list(range(40))


def test_table_duplicates_inside_and_across_batches():
    st = _table_store('duplicates')
    a, b, c = (ss.sha3(x) for x in (b'a', b'b', b'c'))
    assert st.add_digests([a, b, a, a]) == 2
    assert [st.is_dup(i) for i in range(4)] == [False, False, True, True]
    assert st.add_digests([b, c]) == 1 and st.is_dup(4) and not st.is_dup(5)
    assert [st.find(x) for x in (a, b, c)] == [0, 1, 5]
    assert st.info()['n_nodes'] == 6 and st.info()['n_unique'] == 3
    assert [st.slot_of(i) for i in (2, 3, 4)] == [-1, -1, -1]
    # growth re-inserts only the nodes that hold a slot
    st.add_digests([ss.sha3(b'x%d' % i) for i in range(40)])
    assert st.info()['n_slots'] == 128 and [st.find(x) for x in (a, b, c)] == [0, 1, 5]
    assert st.info()['n_unique'] == 43


# ------------------------------------------------------------------ 4. list headers of the pack
def test_pack_list_header_boundaries():
    got, _, _ = run_host(ss.sc_boundaries())
    sizes = (55, 56, 255, 256, 65535, 65536)
    heads = [int(got.proof_off[q + 1] - got.proof_off[q]) - n for q, n in enumerate(sizes)]
    assert heads == [1, 2, 2, 3, 3, 4]
    for q, n in enumerate(sizes):
        proof = got.proof(q)
        assert sp.host_split(proof) == [(heads[q], heads[q] + n)]
        assert got.value(q) == ss.leaf_trie(n)[2]


# ------------------------------------------------------------------ 5. history
def test_one_store_serves_both_versions():
    kv0, kv1, (r0, _), (r1, _) = ss.history()
    assert r0 != r1 and set(kv0) - set(kv1) and set(kv1) - set(kv0)
    assert any(kv0[k] != kv1[k] for k in set(kv0) & set(kv1))
    got, _, st = run_host(ss.sc_history())
    assert st.info()['n_nodes'] > st.info()['n_unique']          # the versions share nodes
    keys = sorted(set(kv0) | set(kv1))
    for q, k in enumerate(keys):
        assert got.value(q) == kv0.get(k, b''), k
        assert got.value(len(keys) + q) == kv1.get(k, b''), k
    removed = next(iter(set(kv0) - set(kv1)))
    q = keys.index(removed)
    assert got.val_len[q] > 0 and got.val_len[len(keys) + q] == 0 and got.status[len(keys) + q] == ss.OK


# ------------------------------------------------------------------ 6. hostile bytes, limits
def test_hostile_root_nodes_give_the_mirrors_status():
    assert len(ss.flipped_roots()) >= 3
    got, _, _ = run_host(ss.sc_hostile())
    assert set(got.status.tolist()) <= {ss.OK, ss.NODE_MISSING, ss.MALFORMED}
    assert (got.status == ss.MALFORMED).any()


def test_path_too_long_reports_the_true_count():
    got, _, st = run_host(ss.sc_too_long())
    assert len(got.status) >= 1 and (got.status == ss.PATH_TOO_LONG).all() and (got.node_count == 9).all()
    assert got.proof_off[-1] == 0
    batches, roots, ridx, keys, _ = ss.sc_too_long()
    again = st.prove(roots, ridx, keys, max_nodes=9)
    assert (again.status == ss.OK).all() and (again.node_ids[:, :2] == got.node_ids).all()


def test_missing_nodes_count_the_nodes_before():
    cases = ss.sc_missing()
    for i, sc in enumerate(cases[:-1]):
        got, _, _ = run_host(sc)
        assert got.status[0] == ss.NODE_MISSING and got.node_count[0] == i and got.proof_off[1] == 0
    assert len(cases) - 1 >= 6
    got, _, _ = run_host(cases[-1])
    assert got.status.tolist() == [ss.NODE_MISSING, ss.OK] and got.node_count.tolist() == [0, 0]
    assert got.proof(1) == b'\xc0' and got.proof(0) == b''


def test_every_scenario_under_sanitizers(tmp_path):
    """tools/hostcheck/statestorecheck_main.cpp: its own process, built with
    AddressSanitizer + UBSan; insert, walk and pack of every scenario above with every
    buffer at its exact size, outputs equal to the host build's"""
    cases = []
    for sc in [f() for f in ss.SCENARIOS.values()] + ss.sc_missing() + [th.prove_scenario(r) for r in th.ROWS]:
        got, _, st = run_host(sc)
        info = st.info()
        batches, roots, ridx, keys, max_nodes = sc
        cases.append((batches, roots, ridx, keys, got.max_nodes, got, info['n_nodes'], info['n_unique']))
    for test in (test_table_equal_first_words_and_wrapping_chain, test_table_growth_at_half_load,
                 test_table_duplicates_inside_and_across_batches):
        test()
    for batches in TABLE_BATCHES.values():          # the table's edges: adds alone, no query
        st = ss.HostStore(1)
        for _, digests in batches:
            st.add_digests(digests)
        info = st.info()
        cases.append((batches, [], None, [], 1, ss.Result(0, 1), info['n_nodes'], info['n_unique']))
    assert len(cases) >= 15
    path = str(tmp_path / 'cases.bin')
    ss.write_cases(path, cases)
    subprocess.run(['make', '-s', '-C', ss.HC_DIR, 'statestorecheck_asan'], check=True)
    r = subprocess.run([os.path.join(ss.HC_DIR, 'statestorecheck_asan'), path], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'statestorecheck ok: {} cases'.format(len(cases)) in r.stdout
