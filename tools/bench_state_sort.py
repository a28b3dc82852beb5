"""Measure the device sort of state keys and the fused build on one GPU.

    python tools/bench_state_sort.py [--repeat 3] [--window 0.5] [--sizes 4096,65536,1048576]
                                     [--cross 256,1024,4096,16384,65536,262144,1048576]
                                     [--out profiles/state_sort.json]

The method of tools/bench_state_build.py: HIP events around the C-ABI device entry points (each
ends with a stream synchronize), one warm-up per shape, windows of at least --window seconds, every
shape repeated --repeat times, medians.  Three key mixes per size, each with values of 2 - 250
bytes, the pairs in a seeded random order:

  random32   distinct random 32-byte keys (what sha256(nym) gives): one round
  mixed      the mixed state of tools/bench_state_build.py: two thirds 32-byte digests, one third
             attr:%d keys, which share a word
  shared24   32-byte keys that share their first 24 bytes: four rounds

Per size and mix:

  sort             pv_state_sort_device: the permutation alone
  sort_gather      pv_time_state_sort_device: the sort and the gather of the kept pairs into compact
                   blobs; `sort_ms` / `gather_ms` are its own event times of the two steps, `rounds`
                   the rounds the sort ran
  fused_build      pv_state_build_unsorted_device over the unsorted pairs, node outputs written
  sorted_build     pv_state_build_device over the same pairs sorted beforehand, in the same run;
                   sort_adds_ms = fused_build - sorted_build is what sorting on the device costs
  tmp_bytes_per_key  the sort's and the gather's temporaries (records, scan words, digit table,
                   permutation, offsets and the compact copies of keys and values), from the sizes

`wall` compares, on the clock of the host and for random32 keys, the fused build including the
upload of the unsorted pairs with the unchanged host form pv_state_build on the same unsorted
input (which sorts on one host thread and uploads); both return the root and the sizes only.
The host form is the comparand, not under test.  `crossover_keys` is the smallest measured size
from which on the device-sorted path is the quicker one, or null with the reason.
Writes one JSON line.  Without a GPU it fails.
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'indy-plenum_amd'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_state_build import wall  # noqa: E402
from bench_state_proofs import p, stream, timed  # noqa: E402
from bench_state_store import median  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def keys_of(mix, n, rng):
    if mix == 'random32':
        keys = {rng.randbytes(32) for _ in range(n)}
        while len(keys) < n:
            keys.add(rng.randbytes(32))
        return list(keys)
    if mix == 'mixed':
        return [hashlib.sha256(b'did:%d' % i).digest() if i % 3 else b'attr:%d' % i for i in range(n)]
    prefix = rng.randbytes(24)
    return [prefix + i.to_bytes(4, 'big') + hashlib.sha256(b'%d' % i).digest()[:4] for i in range(n)]


def unsorted_pairs(mix, n, rng):
    prs = [(k, sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])) for k in keys_of(mix, n, rng)]
    rng.shuffle(prs)
    return prs


def tmp_bytes_per_key(n, key_bytes, val_bytes):
    blocks = (n + sst.SORT_TILE - 1) // sst.SORT_TILE
    sort = 2 * 16 * n + 8 * (n + 1) + 8 * 256 * blocks + 4 * n
    gather = 2 * 8 * (n + 1) + key_bytes + val_bytes + 32
    return {'sort': sort / n, 'gather': gather / n}


def host_arrays(prs):
    kblob, koff = nat.pack_messages([k for k, _ in prs])
    vblob, voff = nat.pack_messages([v for _, v in prs])
    pad = lambda a: np.concatenate([a, np.zeros(16, np.uint8)])   # noqa: E731
    return pad(kblob), koff.copy(), pad(vblob), voff.copy()


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rng = random.Random(2000)
    res = {'tool': 'tools/bench_state_sort.py', 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    up = lambda arr: torch.from_numpy(arr.view(np.uint8)).to(dev)   # noqa: E731
    root, root2 = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    for n in a.sizes:
        res['sizes'][str(n)] = {}
        for mix in ('random32', 'mixed', 'shared24'):
            prs = unsorted_pairs(mix, n, rng)
            hk, hko, hv, hvo = host_arrays(prs)
            d_k, d_ko, d_v, d_vo = up(hk), up(hko), up(hv), up(hvo)
            sk, sko, sv, svo = (up(x) for x in host_arrays(sorted(prs)))
            perm = torch.zeros(4 * n, dtype=torch.uint8, device=dev)
            kept, rounds = ctypes.c_uint64(0), ctypes.c_uint32(0)
            ms_sort, ms_gather = ctypes.c_float(0), ctypes.c_float(0)
            step = {'sort': [], 'gather': []}

            def sort():
                nat._check('pv_state_sort_device', lib.pv_state_sort_device(p(d_k), p(d_ko), n, p(perm),
                                                                            ctypes.byref(kept), 0, stream()))

            def sort_gather():
                nat._check('pv_time_state_sort_device', lib.pv_time_state_sort_device(
                    p(d_k), p(d_ko), p(d_v), p(d_vo), n, 0, stream(), ctypes.byref(kept), ctypes.byref(rounds),
                    ctypes.byref(ms_sort), ctypes.byref(ms_gather)))
                step['sort'].append(ms_sort.value)
                step['gather'].append(ms_gather.value)

            def build(entry, bufs, out_root, blob=None, bcap=0, off=None, ncap=0, dig=None):
                nat._check(entry, getattr(lib, entry)(
                    *[p(b) for b in bufs], n, -1, sst._root_ptr(out_root), ctypes.byref(nn), ctypes.byref(nb), p(blob),
                    bcap, p(off), ncap, p(dig), 0, stream()))
            build('pv_state_build_device', (sk, sko, sv, svo), root)      # sizes
            nodes, nbytes = nn.value, nb.value
            o_blob = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
            o_off = torch.zeros(nodes + 1, dtype=torch.int64, device=dev)
            o_dig = torch.zeros(nodes * 32, dtype=torch.uint8, device=dev)
            f_dig = torch.zeros(nodes * 32, dtype=torch.uint8, device=dev)
            s = {'keys': n, 'nodes': nodes, 'key_bytes': int(hko[-1]), 'value_bytes': int(hvo[-1])}
            runs = [timed(sort, a.window) for _ in range(a.repeat)]
            assert kept.value == n
            s['sort'] = {'runs': runs, 'ms': median(runs)}
            runs = [timed(sort_gather, a.window) for _ in range(a.repeat)]
            s['sort_gather'] = {'runs': runs, 'ms': median(runs), 'rounds': rounds.value,
                                'sort_ms': sorted(step['sort'])[len(step['sort']) // 2],
                                'gather_ms': sorted(step['gather'])[len(step['gather']) // 2]}
            # alternate the two builds, so that both see the same machine
            fused, plain = [], []
            for _ in range(a.repeat):
                fused.append(timed(lambda: build('pv_state_build_unsorted_device', (d_k, d_ko, d_v, d_vo), root2,
                                                 o_blob, nbytes, o_off, nodes, f_dig), a.window))
                plain.append(timed(lambda: build('pv_state_build_device', (sk, sko, sv, svo), root, o_blob, nbytes,
                                                 o_off, nodes, o_dig), a.window))
            assert root.tobytes() == root2.tobytes() and torch.equal(o_dig, f_dig), 'the fused and the sorted build differ'
            s['fused_build'] = {'runs': fused, 'ms': median(fused)}
            s['sorted_build'] = {'runs': plain, 'ms': median(plain)}
            s['sort_adds_ms'] = s['fused_build']['ms'] - s['sorted_build']['ms']
            for name in ('sort', 'sort_gather', 'fused_build', 'sorted_build'):
                s[name]['keys_per_s'] = n / s[name]['ms'] * 1e3
            s['tmp_bytes_per_key'] = tmp_bytes_per_key(n, s['key_bytes'], s['value_bytes'])
            res['sizes'][str(n)][mix] = s
            print(n, mix, {k: (round(v['ms'], 4) if isinstance(v, dict) and 'ms' in v else v) for k, v in s.items()})

    # ---- wall clock: the fused build with its upload against the host form on the same unsorted input
    cross = {}
    for n in a.cross:
        prs = unsorted_pairs('random32', n, rng)
        hk, hko, hv, hvo = host_arrays(prs)

        def device_path():
            bufs = [up(x) for x in (hk, hko, hv, hvo)]
            nat._check('pv_state_build_unsorted_device', lib.pv_state_build_unsorted_device(
                *[p(b) for b in bufs], n, -1, sst._root_ptr(root2), ctypes.byref(nn), ctypes.byref(nb), None, 0, None,
                0, None, 0, stream()))

        def host_path():
            nat._check('pv_state_build', lib.pv_state_build(
                hk.ctypes.data, hko.ctypes.data, hv.ctypes.data, hvo.ctypes.data, n, -1, sst._root_ptr(root),
                ctypes.byref(nn), ctypes.byref(nb), None, 0, None, 0, None))
        cross[str(n)] = {'device_sorted_ms': wall(device_path, a.wall_window), 'host_form_ms': wall(host_path, a.wall_window)}
        assert root.tobytes() == root2.tobytes(), 'the fused build and the host form differ'
        print('wall', n, {k: round(v, 3) for k, v in cross[str(n)].items()})
    res['wall'] = cross
    ahead = [n for n in a.cross if cross[str(n)]['device_sorted_ms'] < cross[str(n)]['host_form_ms']]
    behind = [n for n in a.cross if n not in ahead]
    from_on = [n for n in ahead if all(m < n for m in behind)]
    res['crossover_keys'] = min(from_on) if from_on else None
    if not from_on:
        res['crossover_note'] = 'the device-sorted path does not overtake the host form at the sizes measured'
    print('crossover_keys', res['crossover_keys'])

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')


def main():
    ints = lambda s: [int(x) for x in s.split(',')]   # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--wall-window', type=float, default=0.3)
    ap.add_argument('--sizes', type=ints, default=[4096, 65536, 1 << 20])
    ap.add_argument('--cross', type=ints, default=[256, 1024, 4096, 16384, 65536, 262144, 1 << 20])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_sort.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_sort: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
