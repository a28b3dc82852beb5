"""The sort of state keys on the CPU: the host build of csrc/pv_trie_sort.h
(tools/hostcheck/statesortcheck.cpp: the rounds of words, the composite, the flag pass, with
std::stable_sort or with the device's counting passes per round) against the Python mirror
(plenum_gpu.state_store.sort_keys_host) on every case list of tests/_state_sort.py; the stand-alone
sanitizer program runs the same cases with exact-size buffers.

Rounds.  The header's cost rule is one round per 8 bytes that two distinct keys share, plus one
when equal keys end on a word boundary.  Distinct random 32-byte keys: 1.  The 64-key chain: its last
two keys share 31 bytes, three whole words, so 4 rounds for the distinct keys and 5 =
ceil(32 / 8) + 1, the bound, once one of them occurs twice (as it does wherever the tests inject
stale occurrences).  Keys sharing 200 bytes with an 8-byte tail: 25 shared words, so 26 rounds
for distinct keys and 27 with a key present twice."""
import os
import re
import subprocess

import numpy as np
import pytest

import _state_sort as so
from conftest import REPO


@pytest.mark.parametrize('name', [n for n, _ in so.accepted_cases()])
def test_twin_equals_mirror(name):
    keys = dict(so.accepted_cases())[name]
    want = so.mirror(keys)
    for lsd in (False, True):
        rc, perm, rounds, _ = so.host_sort(keys, lsd=lsd)
        assert rc == so.OK
        assert perm.dtype == want.dtype and perm.shape == want.shape and (perm == want).all(), (name, lsd)
        assert (rounds >= 1) == bool(keys)


def test_mirror_is_sorted_with_last_wins():
    keys = [b'ab\x01', b'ab', b'ab\x00\x00', b'ab\x00', b'ab', b'', b'ab\x00']
    assert list(so.mirror(keys)) == [5, 4, 6, 2, 0]
    assert [keys[i] for i in so.mirror(keys)] == [b'', b'ab', b'ab\x00', b'ab\x00\x00', b'ab\x01']
    assert list(so.host_sort(keys)[1]) == [5, 4, 6, 2, 0]


def test_key_starts_fall_on_every_residue():
    """the edge keys, packed back to back, start at every byte offset mod 8, and so do keys behind a lead-in"""
    keys = so.edge_keys()
    assert len(so.short_strings()) == 156 and b'' in keys and len(keys) == 156 * (1 + len(so.PREFIX_LENGTHS))
    blob, off = so.pack(keys)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8))
    want = so.mirror(keys)
    for lead in range(1, 9):
        blob, off = so.pack(keys, lead=lead)
        rc, perm, _, _ = so.host_sort(None, off=off, blob=blob)
        assert rc == so.OK and (perm == want).all()


@pytest.mark.parametrize('keys,rounds', [
    (so.shuffled(so.size_keys(257), 1), 1),
    (so.chain_keys(), 4),
    (so.chain_keys(copies=9), 5),
    (so.shared_keys(300, 200, 8, 61), 26),
    (so.shared_keys(300, 200, 8, 61, copies=1), 27),
    ([b'\x11' * 32] * 5, 5),
    ([b'abcdefg'] * 2, 1), ([b'abcdefgh'] * 2, 2), ([b'abcdefghi'] * 2, 2),
    ([b''], 1), ([b'k' * 1024], 1), (so.long_keys(), 129),
], ids=['random32', 'chain', 'chain_dup', 'shared200', 'shared200_dup', 'equal32', 'equal7', 'equal8', 'equal9',
        'empty', 'one1024', 'long1024'])
def test_rounds(keys, rounds):
    for lsd in (False, True):
        rc, perm, got, _ = so.host_sort(keys, lsd=lsd)
        assert rc == so.OK and got == rounds and (perm == so.mirror(keys)).all()


def test_refusals():
    keys = so.too_long_keys()
    assert so.host_sort(keys) == (so.BAD_LENGTH, None, 0, 17)
    blob, off = so.pack([b'abc', b'de', b'f'])
    off[2] = 2                                     # decreases at key 1, and key 2 grows by as much
    assert so.host_sort(None, off=off, blob=blob) == (so.BAD_OFFSET, None, 0, 1)
    keys[3] = b'\x66' * 2000                       # the first of two long keys is named
    assert so.host_sort(keys) == (so.BAD_LENGTH, None, 0, 3)


def test_constants_match_the_header():
    from plenum_gpu import state_store
    text = open(os.path.join(REPO, 'indy-plenum_amd', 'csrc', 'pv_trie_sort.h')).read()
    tile = int(re.search(r'constexpr uint32_t TS_TILE = (\d+);', text).group(1))
    block = int(re.search(r'constexpr uint32_t TS_BLOCK = (\d+);', text).group(1))
    items = int(re.search(r'constexpr uint32_t TS_ITEMS = (\d+);', text).group(1))
    longest = int(re.search(r'constexpr uint64_t TS_MAX_KEY_BYTES = (\d+);', text).group(1))
    assert state_store.SORT_TILE == so.TILE == tile == block * items == so.host_lib().ss_tile()
    assert state_store.SORT_MAX_KEY_BYTES == longest == so.host_lib().ss_max_key_bytes() == 1024


def test_asan_program(tmp_path):
    """statesortcheck_asan: every case list and the refusals, each buffer at its exact size"""
    subprocess.run(['make', '-s', '-C', so.HC_DIR, 'statesortcheck_asan'], check=True)
    cases = []
    for name, keys in so.accepted_cases():
        rc, perm, rounds, _ = so.host_sort(keys)
        assert rc == so.OK and (perm == so.mirror(keys)).all()
        cases.append((keys, None, so.OK, 0, so.mirror(keys), rounds))
    cases.append((so.too_long_keys(), None, so.BAD_LENGTH, 17, None, 0))
    cases.append(([b'abc', b'de', b'f'], np.array([0, 3, 2, 6], np.uint64), so.BAD_OFFSET, 1, None, 0))
    path = os.path.join(str(tmp_path), 'cases.bin')
    so.write_cases(path, cases)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(so.HC_DIR, 'statesortcheck_asan'), path], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors='replace')
    assert r.returncode == 0, out[-4000:]
    assert '{} cases ok'.format(len(cases)) in out
