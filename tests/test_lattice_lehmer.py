"""The Lehmer rounds of the lattice stage (csrc/pv_lattice.h hs_euclid_lehmer)
on the host build: the same status, |c|, d and sign as the classical
one-step-at-a-time loop, on the device check's h, 20,000 further random h and
the planted families of tests/_lattice_cases.py; the same as a restatement
over Python integers; and once more as a program of its own under
AddressSanitizer + UBSan.  Exact integers everywhere: there is no tolerance.

hc_half_scalars is the product's form (the Lehmer rounds); hc_half_scalars_lehmer
and hc_half_scalars_classic name the two loops explicitly, the classical one being
the reference."""
import ctypes
import os
import struct
import subprocess

import _devcheck_cases as D
import _lattice_cases as LC


def _run(fn, h):
    c, d = ctypes.create_string_buffer(20), ctypes.create_string_buffer(20)
    neg = ctypes.c_uint32(7)
    st = fn(h.to_bytes(32, 'little'), c, d, ctypes.byref(neg))
    if st != D.HS_HALF:
        return st, 0, 0, 0
    return st, int.from_bytes(c.raw, 'little'), int.from_bytes(d.raw, 'little'), neg.value


def _three(h):
    hc = LC.hc()
    return _run(hc.hc_half_scalars, h), _run(hc.hc_half_scalars_lehmer, h), _run(hc.hc_half_scalars_classic, h)


def _same_as_classic(hs, what):
    for i, h in enumerate(hs):
        built, lehmer, classic = _three(h)
        assert lehmer == classic, '{} case {}: h = {:#x}'.format(what, i, h)
        assert built == classic, '{} case {} (as built): h = {:#x}'.format(what, i, h)


def test_devcheck_h_same_as_classic():
    """every h of the device check, the quotients around 2^32 included: host against host has no exception"""
    _same_as_classic([h for _, h, _ in D.lattice_h()], 'lattice_h')


def test_random_h_same_as_classic():
    _same_as_classic(LC.random_h(20000), 'random')


def test_planted_families_same_as_classic():
    for name, hs in LC.families().items():
        _same_as_classic(hs, name)
    _same_as_classic([LC.longest()], '98 steps')


def test_families_take_the_paths_they_are_named_for():
    f = LC.families()
    # a planted quotient above the cofactor cap of 2^27 ends its round and is taken by one fallback step
    for e, place, h in LC.planted_in_round():
        st, s, ks = LC.rounds(h)
        assert st in (D.HS_HALF, D.HS_DEFER)
        if e >= 2 ** 27:
            assert s[2] >= 2, (hex(e), place)             # the planted step and the exit step
    # 60 quotients of 1 fill a round up to the cofactor cap: Fibonacci(41) > 2^27, at most 40 steps in one round
    for h in f['ones']:
        st, s, ks = LC.rounds(h)
        assert st == D.HS_HALF or st == D.HS_DEFER
        assert 30 <= max(ks) <= 40, ks
    # leading words that agree to 60 bits: a round that proves at most its quotient of 1, then a fallback
    # step that defers on the quotient of about 2^61
    for h in f['close leading words']:
        st, s, ks = LC.rounds(h)
        assert st == D.HS_DEFER and ks[-1] == 0 and ks[-2] <= 1, ks
    assert any(LC.rounds(h)[1][3] >= 2 for h in LC.planted_all()), 'no zero-progress round before the exit'
    for h in f['exit after a full round']:
        st, s, ks = LC.rounds(h)
        assert ks[-1] == 0 and ks[-2] >= 15 and s[4] == 1
    for h in f['exit after a cut round']:
        st, s, ks = LC.rounds(h)
        assert ks[-1] == 0 and 1 <= ks[-2] <= 2 and s[4] == 1
    for h in f['exit after a fallback step']:
        st, s, ks = LC.rounds(h)
        assert ks[-2:] == [0, 0] and s[4] == 1
    for h in f['small']:
        assert LC.rounds(h)[1] == [0, 0, 0, 0, 0]
    # the exit is always found by an exact full-width step
    for h in LC.random_h(2000):
        st, s, ks = LC.rounds(h)
        if h >= 2 ** 128 and st == D.HS_HALF:
            assert s[4] == 1 and ks[-1] == 0
        assert s[0] == len(ks) and s[1] == sum(ks) and s[2] == s[3] == ks.count(0)
        assert s[1] + s[2] == len(D.euclid_quotients(h)) or st == D.HS_DEFER


def test_round_statistics():
    """DESIGN §4's figures: about six proving rounds, 71 leading-word steps and one full-width step per h"""
    hs = LC.random_h(20000)
    tot = [0] * 5
    for h in hs:
        s = LC.rounds(h)[1]
        tot = [a + b for a, b in zip(tot, s)]
    rounds, inner, fallback = (tot[0] - tot[3]) / len(hs), tot[1] / len(hs), tot[2] / len(hs)
    print('proving rounds {:.3f}, inner steps {:.2f}, fallback steps {:.4f}'.format(rounds, inner, fallback))
    assert 5.4 < rounds < 6.4 and 69 < inner < 73 and 0.99 < fallback < 1.05


def test_same_as_python_integers():
    """Euclid over Python integers plus the selection rule, and check_half's properties of every HS_HALF"""
    hs = [h for _, h, _ in D.lattice_h()] + list(LC.planted_all()) + [LC.longest()] + list(LC.random_h(20000))
    hc = LC.hc()
    n_half = n_defer = 0
    for i, h in enumerate(hs):
        got = _run(hc.hc_half_scalars_lehmer, h)
        D.check_half(h, got[0], got[1], got[2], got[3], 'case {}'.format(i))
        want = LC.py_half_scalars(h)
        if want is None:
            assert D.near_2_32(h)
            continue
        assert got == want, 'case {}: h = {:#x}'.format(i, h)
        n_half += got[0] == D.HS_HALF
        n_defer += got[0] == D.HS_DEFER
    assert n_half > 20000 and n_defer > 20


def test_under_sanitizers(tmp_path):
    """latticecheck_asan, a program of its own: the three forms over the same case list"""
    hs = [h for _, h, _ in D.lattice_h()] + list(LC.planted_all()) + [LC.longest()] + list(LC.random_h(20000))
    # bytes outside the contract as well (h >= L, h >= 8L): memory-safe and bounded whatever comes in
    hs += [D.L, D.L8 - 1, D.L8, D.L8 + 1, 2 ** 256 - 1, 2 ** 255, 2 ** 192, 2 ** 160 + 1]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(b'LAT1' + struct.pack('<I', len(hs)))
        for h in hs:
            fh.write(h.to_bytes(32, 'little'))
    subprocess.run(['make', '-s', '-C', D.HC_DIR, 'latticecheck_asan'], check=True)
    r = subprocess.run([os.path.join(D.HC_DIR, 'latticecheck_asan'), path], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'latticecheck ok: {} cases'.format(len(hs)) in r.stdout
