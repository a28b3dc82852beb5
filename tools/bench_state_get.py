"""Measure reads from the resident trie node store against the only way to read before them: the
proof path.

    python tools/bench_state_get.py [--repeat 5] [--window 0.5] [--queries 262144]

One process, the two sides alternated within every repeat, one warm-up per shape, windows of at
least --window seconds.  Two stores, each built on the device (pv_state_build) from seeded pairs
of a 32-byte key and a payload of 2..250 bytes, as tools/bench_state_store.py: the 4,096-key store
and the 2^20-key store.  The queries are --queries random present keys, decode = 1.

  device   pv_state_store_get_device (k_trie_get + the scan + k_trie_get_copy + the 8-byte read of
           the total, in one call) against pv_state_store_walk_device + pv_state_store_pack_device
           (k_trie_prove, k_trie_proof_pack) on the same queries, HIP events around the calls.  The
           scan of proof_len that a caller of the comparand runs between its two calls is NOT in
           its time (it is prepared once): the comparand is favoured.
  host     pv_state_store_get against pv_state_store_prove on the first 100 / 1,000 / --queries of
           them at the 4,096-key store and at the 2^20-key store, wall clock around the call
           (uploads, kernels, copies back).
  bytes    what each returns per query: the bytes of the blob plus the per-query arrays.

Every figure is the median of the repeats' medians with the lowest and the highest repeat beside it;
a difference inside that spread is no difference.  Writes one JSON line to profiles/state_get.json
(--out names another file).  Without a GPU it fails.
"""
import argparse
import hashlib
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'indy-plenum_amd'))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_state_proofs import p, stream, timed  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def spread(runs):
    """repeats of timed() -> the median of their medians, the lowest and the highest"""
    m = sorted(r['ms_median'] for r in runs)
    return {'ms': m[len(m) // 2], 'ms_low': m[0], 'ms_high': m[-1], 'repeats': len(m),
            'calls': sum(r['calls'] for r in runs)}


def wall(fn, window):
    """timed() with the host clock around a synchronous call"""
    fn()
    ms, t0 = [], time.perf_counter()
    while not ms or (time.perf_counter() - t0 < window and len(ms) < 2000):
        a = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - a) * 1e3)
    ms.sort()
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'calls': len(ms)}


def verdict(new, old):
    """faster / slower only when the two spreads do not overlap"""
    if new['ms_high'] < old['ms_low']:
        return 'get faster'
    if old['ms_high'] < new['ms_low']:
        return 'get slower'
    return 'inside the spread'


def bench_store(lib, a, n_keys, host_sizes):
    dev = torch.device('cuda:0')
    rng = random.Random(1600 + n_keys)
    t = lambda arr, dt: torch.from_numpy(np.array(arr, dt)).to(dev)   # noqa: E731
    kv = [(hashlib.sha256(b'did:%d' % i).digest(), rng.randbytes(rng.randint(2, 250))) for i in range(n_keys)]
    store = sst.GpuStateStore(node_hint=2 * n_keys)
    root = store.build_state(kv)
    sid = store._id
    out = {'keys': n_keys, 'store': store.info()}
    Q = a.queries
    pick = [rng.randrange(n_keys) for _ in range(Q)]
    keys = [kv[j][0] for j in pick]
    kblob, koff = nat.pack_messages(keys)
    d_k = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
    d_koff = t(koff.view(np.int64), np.int64)
    d_root = torch.frombuffer(bytearray(root), dtype=torch.uint8).to(dev)
    d_ridx = torch.zeros(Q, dtype=torch.int32, device=dev)

    # ---- device: the read
    status, found = (torch.zeros(Q, dtype=torch.uint8, device=dev) for _ in range(2))
    voff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    nat._check('pv_state_store_get_device', lib.pv_state_store_get_device(
        sid, p(d_root), p(d_ridx), 1, p(d_k), p(d_koff), Q, 1, p(status), p(found), p(voff), None, 0, stream()))
    vtotal = int(voff[-1])
    vals = torch.zeros(vtotal + 16, dtype=torch.uint8, device=dev)

    def get():
        nat._check('pv_state_store_get_device', lib.pv_state_store_get_device(
            sid, p(d_root), p(d_ridx), 1, p(d_k), p(d_koff), Q, 1, p(status), p(found), p(voff), p(vals), vtotal,
            stream()))

    # ---- device: the comparand, walk + pack
    max_nodes = 2 * 32 + 1
    pstatus = torch.zeros(Q, dtype=torch.uint8, device=dev)
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    ids = torch.zeros(Q * max_nodes, dtype=torch.int32, device=dev)
    plen, vrel, vlen = (torch.zeros(Q, dtype=torch.int64, device=dev) for _ in range(3))

    def walk():
        nat._check('pv_state_store_walk_device', lib.pv_state_store_walk_device(
            sid, p(d_root), p(d_ridx), 1, p(d_k), p(d_koff), Q, max_nodes, p(pstatus), p(count), p(ids), p(plen),
            p(vrel), p(vlen), stream()))
    walk()
    poff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    poff[1:] = torch.cumsum(plen, 0)
    ptotal = int(poff[-1])
    proofs = torch.zeros(ptotal + 16, dtype=torch.uint8, device=dev)

    def prove():
        walk()
        nat._check('pv_state_store_pack_device', lib.pv_state_store_pack_device(
            sid, p(ids), p(count), max_nodes, p(poff), Q, p(proofs), stream()))

    g_runs, p_runs = [], []
    for _ in range(a.repeat):             # alternated
        g_runs.append(timed(get, a.window))
        p_runs.append(timed(prove, a.window))
    assert int(status.max()) == sp.PV_SP_OK and int(found.min()) == 1 and int(pstatus.max()) == sp.PV_SP_OK
    # the same values by both paths, at the size timed
    h_voff, h_vals = voff.cpu().numpy(), vals.cpu().numpy()
    h_poff, h_proofs = poff.cpu().numpy(), proofs.cpu().numpy()
    h_vrel, h_vlen = vrel.cpu().numpy(), vlen.cpu().numpy()
    for q in range(0, Q, max(1, Q // 4096)):
        o = int(h_poff[q] + h_vrel[q])
        stored = h_proofs[o:o + int(h_vlen[q])].tobytes()
        got = h_vals[int(h_voff[q]):int(h_voff[q + 1])].tobytes()
        assert got == sst.rlp_decode(stored)[0] == kv[pick[q]][1], 'the read and the proof disagree'
    g, pr = spread(g_runs), spread(p_runs)
    out['device'] = {
        'queries': Q, 'get': dict(g, queries_per_s=Q / g['ms'] * 1e3),
        'walk_pack': dict(pr, queries_per_s=Q / pr['ms'] * 1e3), 'nodes_per_query': int(count.sum()) / Q,
        'get_over_walk_pack': g['ms'] / pr['ms'], 'verdict': verdict(g, pr),
        'bytes_per_query': {'get': vtotal / Q + 8 + 2, 'walk_pack': ptotal / Q + 8 + 8 + 8 + 4 + 1}}

    # ---- host forms, wall clock
    out['host'] = {}
    rts = np.frombuffer(root, np.uint8).copy()
    for n in host_sizes:
        n = min(n, Q)
        kb, ko = nat.pack_messages(keys[:n])
        ridx = np.zeros(n, np.uint32)
        hs, hf = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        hvo = np.zeros(n + 1, np.uint64)
        vcap = int(h_voff[n]) if n < Q else vtotal
        hv = np.zeros(vcap + 16, np.uint8)
        cnt = np.zeros(n, np.uint32)
        hpo, hvr, hvl = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        pcap = int(h_poff[n])
        hp = np.zeros(pcap + 16, np.uint8)
        ptr = lambda x: x.ctypes.data                                           # noqa: E731

        def hget():
            nat._check('pv_state_store_get', lib.pv_state_store_get(
                sid, ptr(rts), ptr(ridx), 1, ptr(kb), ptr(ko), n, 1, ptr(hs), ptr(hf), ptr(hvo), ptr(hv), vcap))

        def hprove():
            nat._check('pv_state_store_prove', lib.pv_state_store_prove(
                sid, ptr(rts), ptr(ridx), 1, ptr(kb), ptr(ko), n, max_nodes, ptr(hs), ptr(cnt), ptr(hpo), ptr(hvr),
                ptr(hvl), ptr(hp), pcap))
        g_runs, p_runs = [], []
        for _ in range(a.repeat):
            g_runs.append(wall(hget, a.window))
            p_runs.append(wall(hprove, a.window))
        g, pr = spread(g_runs), spread(p_runs)
        out['host'][str(n)] = {'get': g, 'prove': pr, 'get_over_prove': g['ms'] / pr['ms'], 'verdict': verdict(g, pr),
                               'bytes_returned': {'get': vcap + 10 * n + 8, 'prove': pcap + 29 * n + 8}}
    store.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--queries', type=int, default=1 << 18)
    ap.add_argument('--big', type=int, default=1 << 20, help='keys of the large store')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_get.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_get: no GPU (a measurement needs one)')
    nat.ensure_init()
    lib = nat.load()
    res = {'tool': 'tools/bench_state_get.py', 'device': torch.cuda.get_device_name(0), 'repeat': a.repeat,
           'window_s': a.window, 'stores': {}}
    # a stream of its own: the library takes a NULL stream for "its own", so on torch's default
    # stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        for n_keys in (4096, a.big):
            res['stores'][str(n_keys)] = bench_store(lib, a, n_keys, (100, 1000, a.queries))
            s = res['stores'][str(n_keys)]
            print(n_keys, 'device', {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s['device'].items()})
            for n, h in s['host'].items():
                print(n_keys, 'host', n, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in h.items()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
