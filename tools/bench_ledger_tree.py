"""Measure the ledger write cycle of the resident Merkle tree on one GPU.

    python tools/bench_ledger_tree.py [--repeat 3] [--window 0.5]

Every entry point here is synchronous, so a call is timed on the host clock
from entry to return; one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times, A and B windows alternating in
one process.  On a 2^20-leaf tree:

  A  stage_<k>    pv_merkle_tree_stage_hashes_device of k = 100 / 1,000 leaf hashes (k_merkle_edge,
                  one launch), each followed by an untimed discard
  B  extend_<k>   pv_merkle_tree_extend_hashes_device of the same hashes on a sibling tree (one
                  k_merkle_level_keep launch per level: the path extend has always taken)
  discard_1000    pv_merkle_tree_discard of 1,000 staged leaves back to 2^20 (one k_merkle_edge
                  launch whose 20 levels each hash with a left sibling: the longest chain there is)
  *_from_2p20m1   the A/B pair of 1,000 from 2^20 - 1 leaves, where stage's chain is as long
  hash_store_*    pv_merkle_tree_hash_store_device over the whole tree / the last 1,000 leaves
  check_nodes_*   pv_merkle_tree_check_nodes (nodes uploaded from host memory inside the call)
  host_replay     one-thread Python replay of Ledger.treeWithAppliedTxns for 1,000 leaves
                  (frontier copy plus one append per leaf, hashlib)

The selection rule of DESIGN section 19 is evaluated on the medians: the
one-launch path stays selected for stage only where A's median lies below B's
by more than the spread of B's repeats.  hash_store / check_nodes report the
bytes they move (nodes and leaves read and written once) over their time,
beside the 8 TB/s HBM3E peak.  Writes one JSON line to
profiles/ledger_tree.json.  Without a GPU it fails.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'indy-plenum_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from plenum_gpu import _native as nat  # noqa: E402

N = 1 << 20
HBM_PEAK = 8.0e12
EXTEND_CALLS = 6000   # a sibling tree grows with every timed extend: 6M leaves at most, inside its capacity


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def timed(fn, window, after=None, max_calls=None):
    ms, t0 = [], time.perf_counter()
    while (not ms or time.perf_counter() - t0 < window) and (max_calls is None or len(ms) < max_calls):
        a = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - a) * 1e3)
        if after:
            after()
    ms.sort()
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'calls': len(ms)}


def host_replay(frontier, leaves):
    """Ledger.treeWithAppliedTxns: copy the compact tree, append leaf by leaf, read the root"""
    stack = list(frontier)   # (height, hash), largest subtree first
    for leaf in leaves:
        stack.append((0, hashlib.sha256(b'\x00' + leaf).digest()))
        while len(stack) >= 2 and stack[-2][0] == stack[-1][0]:
            (h, r), (_, l) = stack.pop(), stack.pop()
            stack.append((h + 1, hashlib.sha256(b'\x01' + l + r).digest()))
    acc = stack[-1][1]
    for _, h in reversed(stack[:-1]):
        acc = hashlib.sha256(b'\x01' + h + acc).digest()
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_ledger_tree: no GPU (a measurement needs one)')
    nat.ensure_init()
    lib = nat.load()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(19)
    leaf_hashes = torch.randint(0, 256, (N, 32), dtype=torch.uint8, device=dev, generator=g)
    more = torch.randint(0, 256, (1000, 32), dtype=torch.uint8, device=dev, generator=g)
    torch.cuda.synchronize()

    def check(name, rc):
        nat._check(name, rc)

    def new_tree(n=N):
        h = ctypes.c_int32(0)
        check('pv_merkle_tree_create', lib.pv_merkle_tree_create(1 << 23, 0, ctypes.byref(h)))
        check('pv_merkle_tree_extend_hashes_device',
              lib.pv_merkle_tree_extend_hashes_device(h.value, p(leaf_hashes), n, None))
        return h.value

    def stage(h, k):
        check('pv_merkle_tree_stage_hashes_device', lib.pv_merkle_tree_stage_hashes_device(h, p(more), k, None, None))

    def discard(h, k):
        check('pv_merkle_tree_discard', lib.pv_merkle_tree_discard(h, k, None))

    def extend(h, k):
        check('pv_merkle_tree_extend_hashes_device', lib.pv_merkle_tree_extend_hashes_device(h, p(more), k, None))

    out = {'tool': 'tools/bench_ledger_tree.py', 'device': torch.cuda.get_device_name(0), 'leaves': N,
           'window_s': a.window, 'hbm_peak_bytes_per_s': HBM_PEAK, 'timing': 'host clock around synchronous calls',
           'runs': []}
    ta = new_tree()
    n_nodes = N - 1
    leaf_out = torch.zeros((N, 32), dtype=torch.uint8, device=dev)
    node_out = torch.zeros((n_nodes, 32), dtype=torch.uint8, device=dev)
    cnt = ctypes.c_uint64(0)

    def hash_store(first, last):
        check('pv_merkle_tree_hash_store_device', lib.pv_merkle_tree_hash_store_device(
            ta, first, last, p(leaf_out), p(node_out), n_nodes, ctypes.byref(cnt), None))

    hash_store(0, N)
    assert cnt.value == n_nodes
    all_nodes = node_out.cpu().numpy()
    hash_store(N - 1000, N)
    tail_count = cnt.value
    tail_nodes = np.ascontiguousarray(node_out[:tail_count].cpu().numpy())
    bad, at = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def check_nodes(first, last, arr):
        check('pv_merkle_tree_check_nodes', lib.pv_merkle_tree_check_nodes(
            ta, first, last, ctypes.c_void_p(arr.ctypes.data), ctypes.byref(bad), ctypes.byref(at)))
        assert bad.value == 0

    for rep in range(a.repeat):
        rec = {}
        for k in (100, 1000):
            stage(ta, k)
            discard(ta, k)                                   # warm-up
            rec['stage_%d' % k] = timed(lambda: stage(ta, k), a.window, after=lambda: discard(ta, k))
            tb = new_tree()
            extend(tb, k)                                    # warm-up
            rec['extend_%d' % k] = timed(lambda: extend(tb, k), a.window, max_calls=EXTEND_CALLS)
            lib.pv_merkle_tree_free(tb)
        # the same pair from 2^20 - 1 leaves: every level above the new leaves hashes with a left
        # sibling (from 2^20 the upper levels only move a node up), and extend's tree stops being
        # such a base after its first call -- reported, not part of the rule
        tw, tb = new_tree(N - 1), new_tree(N - 1)
        stage(tw, 1000)
        discard(tw, 1000)
        rec['stage_1000_from_2p20m1'] = timed(lambda: stage(tw, 1000), a.window, after=lambda: discard(tw, 1000))
        extend(tb, 1000)
        rec['extend_1000_from_2p20m1'] = timed(lambda: extend(tb, 1000), a.window, max_calls=EXTEND_CALLS)
        lib.pv_merkle_tree_free(tw)
        lib.pv_merkle_tree_free(tb)
        stage(ta, 1000)
        rec['discard_1000'] = timed(lambda: discard(ta, 1000), a.window, after=lambda: stage(ta, 1000))
        discard(ta, 1000)
        for name, first, last, nodes in (('all', 0, N, n_nodes), ('last_1000', N - 1000, N, tail_count)):
            moved = 2 * 32 * (nodes + last - first)
            hash_store(first, last)
            r = timed(lambda: hash_store(first, last), a.window)
            r.update(bytes_moved=moved, bytes_per_s=moved / (r['ms_median'] * 1e-3))
            r['fraction_of_hbm_peak'] = r['bytes_per_s'] / HBM_PEAK
            rec['hash_store_' + name] = r
            arr = all_nodes if name == 'all' else tail_nodes
            moved = 2 * 32 * nodes
            check_nodes(first, last, arr)
            r = timed(lambda: check_nodes(first, last, arr), a.window)
            r.update(bytes_moved=moved, bytes_per_s=moved / (r['ms_median'] * 1e-3),
                     note='includes the upload of the nodes from host memory')
            r['fraction_of_hbm_peak'] = r['bytes_per_s'] / HBM_PEAK
            rec['check_nodes_' + name] = r
        out['runs'].append(rec)
    lib.pv_merkle_tree_free(ta)

    # the selection rule
    sel = {}
    for k in (100, 1000):
        am = sorted(r['stage_%d' % k]['ms_median'] for r in out['runs'])
        bm = sorted(r['extend_%d' % k]['ms_median'] for r in out['runs'])
        sel[str(k)] = {'stage_ms_median': am[len(am) // 2], 'extend_ms_median': bm[len(bm) // 2],
                       'extend_spread_ms': bm[-1] - bm[0],
                       'stage_faster_beyond_spread': am[len(am) // 2] < bm[len(bm) // 2] - (bm[-1] - bm[0])}
    out['selection'] = sel
    out['one_launch_selected_for_stage'] = all(v['stage_faster_beyond_spread'] for v in sel.values())

    leaves = [os.urandom(200) for _ in range(1000)]
    fr = [(b, hashlib.sha256(b'frontier-%d' % b).digest()) for b in reversed(range(21)) if (N >> b) & 1]
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        host_replay(fr, leaves)
    out['host_replay_1000'] = {'ms': (time.perf_counter() - t0) * 1e3 / reps,
                               'note': 'one-thread Python/hashlib replay of treeWithAppliedTxns on this host'}
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    line = json.dumps(out, sort_keys=True)
    with open(os.path.join(REPO, 'profiles', 'ledger_tree.json'), 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
