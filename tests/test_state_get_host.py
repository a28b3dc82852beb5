"""Reads from the resident trie node store on the CPU: the routines the kernels run
(csrc/pv_trie_get.h built for the host, tools/hostcheck/stategetcheck.cpp) against the Python
mirror (plenum_gpu.state_store.get_host) and against the values the reference recorded in
tests/golden/state_proofs.json, state_update.json and state_remove.json, for every key they hold;
and all of it once more by stategetcheck_asan, a program of its own under AddressSanitizer +
UBSan with every buffer at its exact size."""
import os
import subprocess

import pytest

import _state_apply as sa
import _state_get as sg
import _state_proofs as sp
import _state_store as ss
import _state_update as su

CASES = []      # (scenario, decode, host Result) of every read below, for the sanitizer run


def read(sc, decode):
    got, _ = sg.run_host(sc, decode)
    CASES.append((sc, decode, got))
    return got


def near(key):
    """absent keys near a present one: cut short, made longer, its last nibble and its first changed"""
    out = [key + b'\x01', key[:-1] + bytes([key[-1] ^ 1]), bytes([key[0] ^ 0x10]) + key[1:]] if key else [b'\x00']
    return out + ([key[:-1]] if key else [])


def check_state(sc_nodes, root, state):
    """every key of `state` = {key: raw value} reads its value at `root` in both modes, and the keys
    near it (near every key of a small state, near about forty keys of a large one) read what the
    state says: absent, unless they are keys of the state themselves"""
    keys = list(state)
    probes = [k for key in keys[::max(1, len(keys) // 40)] for k in near(key)]
    allk = keys + probes
    sc = ([sc_nodes], [root], [0] * len(allk), allk)
    dec = read(sc, True)
    raw = read(sc, False)
    assert (dec.status == sg.OK).all() and (raw.status == sg.OK).all()
    for q, k in enumerate(allk):
        want = state.get(k)
        assert dec.value(q) == want, (k, q)
        assert raw.value(q) == (None if want is None else sp.encode_value(want)), (k, q)


# ------------------------------------------------------------------ 1. the reference's values
def test_every_key_of_the_proof_fixture():
    tr = ss.tries()
    rows = [r for r in ss.proof_rows()]
    for name in sorted(tr):
        root, db = tr[name]
        state = {}
        for r in rows:
            if r.trie == name and r.root == root:
                k, v = r.kvs[0]
                state.setdefault(k, v)
        present = {k: v for k, v in state.items() if v is not None}
        absent = [k for k, v in state.items() if v is None]
        assert present
        # the fixture's tries hold more keys than its rows name: only the rows' own keys are compared
        keys = list(present) + absent
        sc = ([list(db.values())], [root], [0] * len(keys), keys)
        dec, raw = read(sc, True), read(sc, False)
        assert (dec.status == sg.OK).all()
        for q, k in enumerate(keys):
            assert dec.value(q) == state[k], (name, k)
            assert raw.value(q) == (None if state[k] is None else sp.encode_value(state[k])), (name, k)


@pytest.mark.parametrize('mod', [su, sa], ids=['state_update', 'state_remove'])
def test_every_key_of_the_batch_fixtures(mod):
    """the state after each recorded batch, rebuilt by the mirrors and pinned by the recorded roots"""
    from plenum_gpu.state_store import apply_host, build_host
    assert len(mod.fixture()) >= 10
    for c in mod.fixture():
        state = dict(c.base)
        root, db = build_host(c.base) if c.base else (c.base_root, {})
        assert root == c.base_root, c.name
        nodes = dict(db)
        check_state(list(nodes.values()), root, state)
        for b in c.batches:
            root, new = apply_host(nodes, root, b.items)
            assert root == b.root, c.name
            nodes.update(new)
            for k, v in b.items:
                if v is None:
                    state.pop(k, None)
                else:
                    state[k] = v
            if root != sg_blank():
                check_state(list(nodes.values()), root, state)


def sg_blank():
    from plenum_gpu.state_proofs import BLANK_ROOT
    return BLANK_ROOT


# ------------------------------------------------------------------ 2. the scenarios
@pytest.mark.parametrize('name', sorted(sg.scenarios()))
@pytest.mark.parametrize('decode', [False, True], ids=['raw', 'decode'])
def test_host_build_equals_mirror(name, decode):
    read(sg.scenarios()[name], decode)


def test_shapes_read_what_was_set():
    batches, roots, ridx, keys = sg.sc_shapes()
    from plenum_gpu.state_store import rlp_decode
    dec, raw = read(sg.sc_shapes(), True), read(sg.sc_shapes(), False)
    want = dict(sg.SHAPE_PAIRS)
    for q, k in enumerate(keys[:len(sg.SHAPE_PAIRS) + len(sg.SHAPE_ABSENT)]):
        assert raw.value(q) == want.get(k), k
        assert dec.value(q) == (rlp_decode(want[k])[0] if k in want else None), k
    tail = dec.values()[len(sg.SHAPE_PAIRS) + len(sg.SHAPE_ABSENT):]
    assert tail[0] is not None and tail[1:] == [None] * 6        # one leaf: its key, four near it; the blank root
    assert (dec.status == sg.OK).all()


def test_payload_boundaries_and_the_empty_payload():
    got = read(sg.sc_payloads(), True)
    pls = sg.payloads()
    assert [got.value(q) for q in range(len(pls))] == [p for _, p in pls]
    assert got.found.tolist() == [1] * len(pls) + [0]
    assert got.value(0) == b'' and got.value(len(pls)) is None      # found with length 0 is not absent
    raw = read(sg.sc_payloads(), False)
    heads = [len(raw.value(q)) - len(p) for q, (_, p) in enumerate(pls)]
    # string header + list header: a 55-byte payload is a 56-byte item (a long list header), a
    # 56-byte payload takes a long string header too; the same one byte later at 255 / 256
    assert heads == [2, 1, 2, 2, 3, 4, 5, 6, 6]


def test_hostile_values_are_malformed_and_neighbours_are_not():
    batches, roots, ridx, keys = sg.sc_hostile()
    dec, raw = read(sg.sc_hostile(), True), read(sg.sc_hostile(), False)
    assert (raw.status == sg.OK).all() and raw.found.all()
    n = len(sg.HOSTILE_VALUES)
    for i, v in enumerate(sg.HOSTILE_VALUES):
        good, bad = 2 * i, 2 * i + 1
        assert raw.value(bad) == v
        assert (dec.status[bad], dec.found[bad], dec.value(bad)) == (sg.MALFORMED, 0, None), v
        assert dec.status[good] == sg.OK and dec.value(good) == sg._v(20 + i, 40 + i)
        assert sg.host_decode(v) is None
    for i, (v, payload) in enumerate(sg.LENIENT_VALUES):
        assert dec.status[2 * n + i] == sg.OK and dec.value(2 * n + i) == payload, v
        assert sg.host_decode(v) == payload


def test_first_item_and_list_header_forms():
    """a byte below 0x80, a short string, long strings with one and two length bytes; both list headers"""
    from plenum_gpu.state_store import decode_value_host
    for n, first, head in ((1, None, 0xc1), (1, 0x81, 0xc2), (55, 0xb7, 0xf8), (56, 0xb8, 0xf8), (255, 0xb8, 0xf9),
                           (256, 0xb9, 0xf9), (1100, 0xb9, 0xf9), (20, 0x94, 0xd5)):
        p = b'\x05' if first is None else (b'\x85' if n == 1 else sg._v(n, n))
        v = sg.enc(p)
        assert v[0] == head and (first is None or v[1 + (head >= 0xf8) * (head - 0xf7)] == first)
        assert sg.host_decode(v) == p == decode_value_host(v)


def test_roots():
    batches, roots, ridx, keys = sg.sc_roots()
    got = read(sg.sc_roots(), True)
    # old at the old root, new at the new
    assert got.value(2) == sg._v(40, 62) and got.value(6 + 2) == b'new value'
    assert [got.value(q) for q in (0, 6)] == [sg._v(40, 60)] * 2
    assert got.status[12] == sg.NODE_MISSING and got.found[12] == 0                  # a root the store does not hold
    # the keys under the missing child only
    assert got.status[13:].tolist() == [sg.OK, sg.NODE_MISSING, sg.OK, sg.OK]


def test_sizing_call_small_capacity_and_decode_2():
    batches, roots, ridx, keys = sg.sc_count(65)
    st = sg.HostStore(batches)
    full = st.get(roots, ridx, keys, True)
    sizing = st.get(roots, ridx, keys, True, sizing=True)
    assert sizing.rc == 0 and (sizing.val_off == full.val_off).all() and (sizing.found == full.found).all()
    short = st.get(roots, ridx, keys, True, val_cap=int(full.val_off[-1]) - 1)
    assert short.rc == -22 and (short.val_off == full.val_off).all() and (short.status == full.status).all()
    assert st.get(roots, ridx, keys, 2).rc == -22


# ------------------------------------------------------------------ 3. under sanitizers
def test_every_read_under_sanitizers(tmp_path):
    """tools/hostcheck/stategetcheck_main.cpp: its own process, built with AddressSanitizer +
    UBSan; the read walk, the decode and the copy of every read of this module with every buffer
    at its exact size, outputs equal to the host build's; and the decode alone over each hostile
    and lenient stored value in an allocation of exactly its length"""
    if len(CASES) < 20:      # run alone: the scenarios at least
        for sc in sg.scenarios().values():
            read(sc, False)
            read(sc, True)
        test_every_key_of_the_proof_fixture()
    cases = [(sc[0], sc[1], sc[2], sc[3], dec, got) for sc, dec, got in CASES]
    values = [(v, None) for v in sg.HOSTILE_VALUES] + list(sg.LENIENT_VALUES) + \
             [(sg.enc(p), p) for _, p in sg.payloads()]
    path = str(tmp_path / 'cases.bin')
    sg.write_cases(path, cases, values)
    subprocess.run(['make', '-s', '-C', sg.HC_DIR, 'stategetcheck_asan'], check=True)
    r = subprocess.run([os.path.join(sg.HC_DIR, 'stategetcheck_asan'), path], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'stategetcheck ok: {} cases, {} values'.format(len(cases), len(values)) in r.stdout
