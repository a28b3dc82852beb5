"""The conditions of tests/_bls_cases.py on the reference alone (the C oracle and
tests/_bn254_py.py), CPU only: they keep tests/test_gpu_bls_shapes.py from
passing vacuously -- every signature class has the verdict its name says, every
ragged segment holds both verdicts, the key-set checks sit on the indices the
two grouping paths differ at, and the message pool reaches every round of
hash_group and every SHA-256 padding edge."""
import hashlib

import numpy as np
import pytest

import _bls_cases as C
import _bn254_py as bn


def test_ragged_cases_are_complete_and_deterministic():
    c = C.ragged()
    assert len(c['want']) == len(c['labels']) == len(c['sig']) == sum(C.RAGGED_COUNTS) == 143
    assert len(c['keys']) == 12 and len(set(c['labels'])) == 143
    assert [int((c['kidx'] == e).sum()) for e in range(12)] == list(C.RAGGED_COUNTS)
    # scattered: no key's checks are contiguous in the call once it has more than one
    for e, cnt in enumerate(C.RAGGED_COUNTS):
        pos = np.nonzero(c['kidx'] == e)[0]
        assert cnt < 2 or pos[-1] - pos[0] >= cnt, e
    first = c['sig'].tobytes() + c['kidx'].tobytes() + c['midx'].tobytes() + c['want'].tobytes()
    C.ragged.cache_clear()
    d = C.ragged()
    assert d['sig'].tobytes() + d['kidx'].tobytes() + d['midx'].tobytes() + d['want'].tobytes() == first
    assert d['labels'] == c['labels']


def test_ragged_key_entries():
    c = C.ragged()
    keys = [k.tobytes() for k in c['keys']]
    orc = C.oracle()
    for e in list(range(8)) + [10, 11]:
        assert bn.g2_from_bytes(keys[e]) is not None and orc.bls_oracle_g2_in_subgroup(keys[e]) == 1, e
    assert len(set(keys[:8] + [keys[10]])) == 9 and keys[11] == keys[0]
    assert keys[8] == bytes(128) and bn.g2_from_bytes(keys[8]) is None            # off the twist: O, status 1
    assert not C.key_outside_g2(keys[8])
    q = bn.g2_from_bytes(keys[9])                                                  # on the twist, order not r: status 2
    assert q is not None and bn.g2_mul(q, bn.R) is not None and C.key_outside_g2(keys[9])
    assert C.RAGGED_STATUS == [0 if (e < 8 or e > 9) else (1 if e == 8 else 2) for e in range(12)]


def test_every_class_has_its_oracle_verdict():
    """the expected vector (oracle + the header's rule for key 9) equals the class
    table's column on all 143 checks; for valid keys that is the oracle alone"""
    c = C.ragged()
    bad = [lab for lab, w, t in zip(c['labels'], c['want'], c['table']) if w != t]
    assert not bad, bad
    seen = {}
    for lab, w, k in zip(c['labels'], c['want'], c['kidx']):
        if k not in (8, 9):
            seen.setdefault(lab.split(':')[1], set()).add(int(w))
    assert seen == {name: {v} for name, v in C.CLASS_VERDICT.items()}
    # key 8 (O): only sigma = O verifies (the oracle); key 9: nothing does (the header's rule)
    for e, verdicts in C.SPECIAL_VERDICT.items():
        got = {lab.split(':')[1]: int(w) for lab, w, k in zip(c['labels'], c['want'], c['kidx']) if k == e}
        assert got == dict(zip(C.SPECIAL_CLASSES[e], verdicts)), e
    assert not c['want'][c['kidx'] == 9].any()


def test_class_encodings():
    """the corrupted sigmas are what their names say (tests/_bn254_py.py decodes them)"""
    sk, sk2 = C.secret(0), C.secret(1)
    m, m2 = C.pool()[3], C.pool()[4]
    s = {name: f(sk, sk2, m, m2) for name, f, _ in C.CLASSES}
    assert all(len(v) == 128 for v in s.values())
    pt = bn.g1_from_bytes(s['valid'])
    assert pt == bn.g1_mul(bn.hash_to_g1(m), int.from_bytes(sk, 'big'))
    assert bn.g1_from_bytes(s['negated']) == bn.g1_neg(pt)
    assert bn.g1_from_bytes(s['compressed']) == pt and s['compressed'][0] in (2, 3) and not any(s['compressed'][33:])
    assert bn.g1_from_bytes(s['compressed-wrong-parity']) == bn.g1_neg(pt)
    assert bn.g1_from_bytes(s['sigma-O']) is None and bn.g1_from_bytes(s['x-plus-p']) is None
    assert int.from_bytes(s['x-plus-p'][1:33], 'big') == pt[0] + bn.P
    assert bn.g1_from_bytes(s['y-bitflip']) is None
    assert bn.g1_from_bytes(s['other-key']) == bn.g1_mul(bn.hash_to_g1(m), int.from_bytes(sk2, 'big'))
    assert bn.g1_from_bytes(s['other-message']) == bn.g1_mul(bn.hash_to_g1(m2), int.from_bytes(sk, 'big'))


def test_ragged_segments_hold_both_verdicts():
    c = C.ragged()
    for e, cnt in enumerate(C.RAGGED_COUNTS):
        w = set(c['want'][c['kidx'] == e].tolist())
        if cnt >= 7:
            assert w == {0, 1}, e
    assert set(c['want'][c['kidx'] == 0].tolist()) == {1}       # the lone live group of a wave is a valid check
    assert set(c['want'][c['kidx'] == 9].tolist()) == {0}
    # counts on both sides of each kernel's padding, an empty segment between full ones
    assert {7, 8, 9, 15, 16, 17, 31, 33, 1, 0} <= set(C.RAGGED_COUNTS) and C.RAGGED_COUNTS[10] == 0


@pytest.mark.parametrize('nkeys', [2048, 2049])
def test_keysets_sit_on_both_sides_of_group_local_keys(nkeys):
    c = C.keyset(nkeys)
    assert len(c['keys']) == nkeys and (nkeys > C.GROUP_LOCAL_KEYS) == (nkeys == 2049)
    vk = C.valid_keys()
    assert all(c['keys'][e].tobytes() == vk[e % 8] for e in (0, 1, 7, 8, 255, 256, 2047, nkeys - 1))
    counts = {int(e): int((c['kidx'] == e).sum()) for e in set(c['kidx'].tolist())}
    assert counts == C.KEYSET_COUNTS[nkeys]
    assert {0, 1, 255, 256, 2046, 2047} <= set(counts) and (2048 in counts) == (nkeys == 2049)
    assert set(counts.values()) == {1, 2, 9, 17} and 38 <= len(c['want']) <= 42
    for e in (2047, nkeys - 1):
        assert set(c['want'][c['kidx'] == e].tolist()) == {0, 1}, e
    # the verdicts are the three classes' (valid keys: the oracle alone decides)
    for lab, w in zip(c['labels'], c['want']):
        assert int(w) == C.CLASS_VERDICT[lab.split(':')[1]], lab
    assert c['kidx'].tolist() != sorted(c['kidx'].tolist())


def test_pool_increment_counts_and_hash_group_rounds():
    msgs = C.pool()
    assert len(msgs) == 25 and len(msgs) % 8 != 0
    edge = msgs[:len(C.HASH_EDGE_I)]
    assert list(edge) == [b'hash-edge %d' % i for i in C.HASH_EDGE_I]
    inc = [C.increments(m) for m in edge]
    assert inc == list(C.INCREMENTS) == list(range(13)) + [14]
    # hash_group tries 4 candidates per round: rounds one to four are all reached
    assert {min(n // 4, 3) for n in inc} == {0, 1, 2, 3}
    # increments() is hash_to_g1's loop: the point it stops at is hash_to_g1's, and the oracle's
    for m, n in zip(edge, inc):
        x = (int.from_bytes(hashlib.sha256(m).digest(), 'big') + n) % bn.P
        assert bn.hash_to_g1(m)[0] == x
        assert C.hash_to_g1(m) == bn.g1_to_bytes(bn.hash_to_g1(m))
    for m in msgs[len(edge):]:
        assert C.hash_to_g1(m) == bn.g1_to_bytes(bn.hash_to_g1(m))


def test_hash_group_stride_covers_every_candidate():
    """hash_group's schedule (4 candidates per round, the lowest square wins, advance
    by 4) on the pool's digests gives hash_to_g1's x; a schedule that skips a
    candidate (advance by 5) does not -- the pool tells them apart.  A stride
    below 4 only overlaps the rounds: every candidate is still tried, in rising
    order, so the lowest square still wins and no output can differ (it costs
    rounds, not verdicts)."""
    def grouped(m, step):
        x0 = int.from_bytes(hashlib.sha256(m).digest(), 'big')
        while True:
            for c in range(4):
                x = (x0 + c) % bn.P
                if bn.is_qr(x ** 3 + bn.B):
                    return x
            x0 += step
    msgs = C.pool()
    assert all(grouped(m, 4) == bn.hash_to_g1(m)[0] for m in msgs)
    assert any(grouped(m, 5) != bn.hash_to_g1(m)[0] for m in msgs)
    assert all(grouped(m, 3) == bn.hash_to_g1(m)[0] for m in msgs)


def test_pool_layout_and_padding_edges():
    msgs = C.pool()
    rand = msgs[len(C.HASH_EDGE_I):]
    assert [len(m) for m in rand] == list(C.PAD_EDGE_LENGTHS) == [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128]
    blob, off = C.pack(msgs)
    assert int(off[-1]) == len(blob) == sum(len(m) for m in msgs)
    assert {int(o) % 4 for o in off[:-1]} == {0, 1, 2, 3}
    assert all(blob[int(off[i]):int(off[i + 1])].tobytes() == msgs[i] for i in range(len(msgs)))
    assert C.pool() is msgs and len(set(msgs)) == 25


def test_hash_checks_against_oracle():
    c = C.hash_checks()
    assert len(c['want']) == 50 and len(c['keys']) == 1
    for lab, w, m in zip(c['labels'], c['want'], c['midx']):
        assert lab == 'msg{}:{}'.format(m, 'valid' if w else 'next-message'), lab
    assert sorted(c['midx'].tolist()) == sorted(list(range(25)) * 2) and int(c['want'].sum()) == 25


def test_small_pieces_reference():
    """part 4's references: the sums pass through O and go on; the key sums of the
    multi-signature checks are k2 and k; the oracle takes scalars unreduced"""
    sets = C.aggregate_sets()
    s, ns, t = sets[0]
    ps, pt = bn.g1_from_bytes(s), bn.g1_from_bytes(t)
    assert bn.g1_add(ps, bn.g1_from_bytes(ns)) is None
    assert C.aggregate_sigs(sets[0]) == t
    assert C.aggregate_sigs(sets[1]) == bn.g1_to_bytes(bn.g1_add(ps, ps))
    assert C.aggregate_sigs(sets[2]) == s
    assert C.aggregate_sigs(sets[3]) == bn.g1_to_bytes(bn.g1_add(pt, pt))
    assert C.aggregate_sigs((s, ns)) == C.G1_INF
    assert [C.verify_multi(*c) for c in C.multi_checks()] == [1, 0, 1, 0]
    m = C.pool()[1]
    h = C.hash_to_g1(m)
    sc = {k: C.sign(k.to_bytes(32, 'big'), m) for k in C.EDGE_SCALARS}
    assert sc[1] == h and sc[bn.R + 1] == h and sc[bn.R - 1] == C.g1_neg_bytes(h)
    assert sc[2] == bn.g1_to_bytes(bn.g1_mul(bn.hash_to_g1(m), 2))
    for k in ((1 << 255), (1 << 256) - 1):
        assert sc[k] == bn.g1_to_bytes(bn.g1_mul(bn.hash_to_g1(m), k % bn.R))
    g = bn.g2_from_bytes(C.generator())
    for k in C.EDGE_SCALARS:
        assert C.pubkey(k.to_bytes(32, 'big')) == bn.g2_to_bytes(bn.g2_mul(g, k % bn.R)), k
