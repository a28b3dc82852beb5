"""Measure the resident trie node store on one GPU, device-resident.

    python tools/bench_state_store.py [--repeat 3] [--window 0.5] [--queries 262144]

Timed with HIP events around the C-ABI device entry points (each ends with a
stream synchronize), one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times to show the spread.  The trie is
the 4,096-key trie of tools/bench_state_proofs.py and the queries are --queries
random present keys, as in profiles/state_proofs.json.  Shapes:

  insert_1_call    pv_state_store_add_device of all the trie's nodes into a fresh store
                   (created with room for them: no growth), one call
  insert_64_calls  the same nodes in 64 calls into a fresh 64-slot store (the table doubles
                   on the way: k_trie_store_rehash is in the time)
  walk             pv_state_store_walk_device (k_trie_prove) alone
  pack             pv_state_store_pack_device (k_trie_proof_pack) alone
  verify_same      the comparand: pv_state_proof_verify_device on the very proofs generated
                   (every proof's nodes hashed, then walked)

and, one thread on this host, the Python mirror walk_host (a port, not the
reference) on the first 2,000 queries.  Writes one JSON line to
profiles/state_store.json (--out names another file).  Without a GPU it fails.
"""
import argparse
import ctypes
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

from bench_state_proofs import build_trie, p, stream, timed  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def median(runs):
    return sorted(r['ms_median'] for r in runs)[len(runs) // 2]


def timed_fresh(lib, make, fn, window):
    """like timed(), for a call that needs a fresh store each time: make() -> store id
    (outside the events), fn(store) between them, the store freed after"""
    ms, t0 = [], time.perf_counter()
    for warm in (True, False):
        while warm or not ms or (time.perf_counter() - t0 < window and len(ms) < 200):
            sid = make()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(sid)
            b.record()
            b.synchronize()
            nat._check('pv_state_store_free', lib.pv_state_store_free(sid))
            if warm:
                break
            ms.append(a.elapsed_time(b))
    ms.sort()
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'calls': len(ms)}


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rng = random.Random(1600)
    res = {'tool': 'tools/bench_state_store.py', 'device': torch.cuda.get_device_name(0), 'shapes': {}}
    t = lambda arr, dt: torch.from_numpy(np.array(arr, dt)).to(dev)   # noqa: E731

    kv = []
    for i in range(4096):
        key = hashlib.sha256(b'did:%d' % i).digest() if i % 3 else b'attr:%d' % i
        kv.append((key, sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])))
    root, db = build_trie(kv)
    nodes = list(db.values())
    nblob, noff = nat.pack_messages(nodes)
    d_nblob = torch.frombuffer(bytearray(nblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
    d_noff = t(noff.view(np.int64), np.int64)
    res['trie'] = {'keys': len(kv), 'nodes': len(nodes), 'node_bytes': int(noff[-1])}

    def create(hint):
        h = ctypes.c_int32(0)
        nat._check('pv_state_store_create', lib.pv_state_store_create(hint, int(noff[-1]) if hint > 1 else 0, 0,
                                                                      ctypes.byref(h)))
        return h.value

    def add(sid, first, count):
        nat._check('pv_state_store_add_device', lib.pv_state_store_add_device(
            sid, p(d_nblob), ctypes.c_void_p(d_noff.data_ptr() + 8 * first), count, None, stream()))

    # ---- insert
    runs = [timed_fresh(lib, lambda: create(len(nodes)), lambda s: add(s, 0, len(nodes)), a.window)
            for _ in range(a.repeat)]
    ms = median(runs)
    res['shapes']['insert_1_call'] = {'nodes': len(nodes), 'runs': runs, 'ms': ms, 'nodes_per_s': len(nodes) / ms * 1e3}
    step = (len(nodes) + 63) // 64
    parts = [(f, min(step, len(nodes) - f)) for f in range(0, len(nodes), step)]

    def add64(s):
        for f, c in parts:
            add(s, f, c)
    runs = [timed_fresh(lib, lambda: create(1), add64, a.window) for _ in range(a.repeat)]
    ms = median(runs)
    res['shapes']['insert_64_calls'] = {'nodes': len(nodes), 'calls_per_insert': len(parts), 'runs': runs, 'ms': ms,
                                        'nodes_per_s': len(nodes) / ms * 1e3}

    # ---- walk and pack over one resident store
    sid = create(len(nodes))
    add(sid, 0, len(nodes))
    Q = a.queries
    pick = [rng.randrange(len(kv)) for _ in range(Q)]
    keys = [kv[j][0] for j in pick]
    kblob, koff = nat.pack_messages(keys)
    d_k = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
    d_koff = t(koff.view(np.int64), np.int64)
    d_root = torch.frombuffer(bytearray(root), dtype=torch.uint8).to(dev)
    d_ridx = torch.zeros(Q, dtype=torch.int32, device=dev)
    max_nodes = 2 * max(len(k) for k in keys) + 1
    status = torch.zeros(Q, dtype=torch.uint8, device=dev)
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    ids = torch.zeros(Q * max_nodes, dtype=torch.int32, device=dev)
    plen, vrel, vlen = (torch.zeros(Q, dtype=torch.int64, device=dev) for _ in range(3))

    def walk():
        nat._check('pv_state_store_walk_device', lib.pv_state_store_walk_device(
            sid, p(d_root), p(d_ridx), 1, p(d_k), p(d_koff), Q, max_nodes, p(status), p(count), p(ids), p(plen),
            p(vrel), p(vlen), stream()))
    runs = [timed(walk, a.window) for _ in range(a.repeat)]
    assert int(status.max()) == sp.PV_SP_OK, 'a walk did not end OK'
    ms_walk = median(runs)
    hashed = int(count.sum())
    res['shapes']['walk'] = {'queries': Q, 'max_nodes': max_nodes, 'hashed_nodes': hashed,
                             'nodes_per_query': hashed / Q, 'runs': runs, 'ms': ms_walk,
                             'queries_per_s': Q / ms_walk * 1e3}
    poff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
    poff[1:] = torch.cumsum(plen, 0)
    total = int(poff[-1])
    out = torch.zeros(total + 16, dtype=torch.uint8, device=dev)

    def pack():
        nat._check('pv_state_store_pack_device', lib.pv_state_store_pack_device(
            sid, p(ids), p(count), max_nodes, p(poff), Q, p(out), stream()))
    runs = [timed(pack, a.window) for _ in range(a.repeat)]
    ms_pack = median(runs)
    res['shapes']['pack'] = {'queries': Q, 'proof_bytes': total, 'bytes_per_proof': total / Q, 'runs': runs,
                             'ms': ms_pack, 'queries_per_s': Q / ms_pack * 1e3,
                             'gbytes_per_s_read_plus_written': 2 * total / ms_pack / 1e6}
    res['generate_ms'] = ms_walk + ms_pack
    res['generate_queries_per_s'] = Q / (ms_walk + ms_pack) * 1e3

    # ---- the comparand: verify the very proofs generated
    h_off = poff.cpu().numpy()
    h_out = out.cpu().numpy()
    h_vrel, h_vlen = vrel.cpu().numpy(), vlen.cpu().numpy()
    split = {}
    beg, end, first, vals = [], [], [0], []
    for q, j in enumerate(pick):
        o = int(h_off[q])
        if j not in split:
            split[j] = sp.rlp_split_list(h_out[o:int(h_off[q + 1])].tobytes())
        for b, e in split[j]:
            beg.append(o + b)
            end.append(o + e)
        first.append(len(beg))
        vals.append(h_out[o + int(h_vrel[q]):o + int(h_vrel[q]) + int(h_vlen[q])].tobytes())
    assert vals[:64] == [kv[j][1] for j in pick[:64]], 'generated values differ from the trie'
    vblob, voff = nat.pack_messages(vals)
    d_v = torch.frombuffer(bytearray(vblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
    d_voff = t(voff.view(np.int64), np.int64)
    d_beg, d_end, d_first = t(beg, np.int64), t(end, np.int64), t(first, np.int64)
    d_roots = torch.frombuffer(bytearray(root * Q), dtype=torch.uint8).to(dev)
    d_pidx = t(np.arange(Q), np.int32)
    vstatus = torch.ones(Q, dtype=torch.uint8, device=dev)
    dig = torch.zeros(len(beg) * 32, dtype=torch.uint8, device=dev)

    def verify():
        nat._check('pv_state_proof_verify_device', lib.pv_state_proof_verify_device(
            p(out), p(d_beg), p(d_end), p(d_first), p(d_roots), p(d_pidx), p(d_k), p(d_koff), p(d_v), p(d_voff),
            len(beg), Q, Q, p(vstatus), p(dig), 0, stream()))
    runs = [timed(verify, a.window) for _ in range(a.repeat)]
    assert int(vstatus.max()) == sp.PV_SP_OK, 'a generated proof does not verify'
    ms_ver = median(runs)
    res['shapes']['verify_same'] = {'queries': Q, 'nodes': len(beg), 'runs': runs, 'ms': ms_ver,
                                    'queries_per_s': Q / ms_ver * 1e3}
    res['generate_over_verify'] = (ms_walk + ms_pack) / ms_ver
    nat._check('pv_state_store_free', lib.pv_state_store_free(sid))

    # ---- the mirror, one thread, on the first 2,000 queries
    k = min(2000, Q)
    t0 = time.perf_counter()
    mirror = [sst.walk_host(db, root, keys[i]) for i in range(k)]
    res['cpu_python_walk_host_queries_per_s'] = k / (time.perf_counter() - t0)
    res['cpu_python_walk_host_note'] = 'a Python port of sg_walk, one thread; not the reference implementation'
    for i in range(0, k, 97):
        assert mirror[i][3] == h_out[int(h_off[i]):int(h_off[i + 1])].tobytes(), 'the mirror and the GPU disagree'
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')
    for name, s in res['shapes'].items():
        print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items() if k != 'runs'})
    print('generate / verify', round(res['generate_over_verify'], 3), 'walk_host queries/s',
          round(res['cpu_python_walk_host_queries_per_s']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--queries', type=int, default=1 << 18)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_store.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_store: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
