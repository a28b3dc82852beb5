"""Measure the batch trie build on one GPU, device-resident.

    python tools/bench_state_build.py [--repeat 3] [--window 0.5] [--sizes 4096,65536,1048576]
                                      [--queries 262144] [--mirror-max 1048576]
                                      [--out profiles/state_build.json]

Timed with HIP events around the C-ABI device entry points (each ends with a
stream synchronize), one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times to show the spread, as
tools/bench_state_store.py.  The states are mixed states like the fixture's:
two thirds 32-byte keys, values of 2 - 250 bytes; 4,096 keys is the shape of the
trie of profiles/state_proofs.json and profiles/state_store.json (other random
values).  Per size:

  build            pv_state_build_device, node blob / offsets / digests written, no store
  build_store      the same into a fresh store (created with room: no growth), no outputs
  sha3_floor       k_sha3_256 alone (pv_sha3_256_batch_device) over the very nodes the build
                   emitted: the build cannot beat hashing its own output
  store_add        pv_state_store_add_device of those nodes into a fresh store: what filling
                   the store costs once a host has produced the nodes
  mirror           build_encoded_host, one thread on this host (a port, not the reference),
                   once per size (--mirror-max bounds the sizes it runs on)

`dispatch` times the host form as Python calls it (state_root_batch's two paths,
wall clock, small batches): where the GPU call overtakes the mirror is
state_store.BUILD_GPU_MIN_ITEMS.  With --queries > 0 the largest state is then
walked, packed and verified once more (the shapes of tools/bench_state_store.py)
from the store the build filled: the figures for a store larger than the caches.
Writes one JSON line.  Without a GPU it fails.
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

from bench_state_proofs import p, stream, timed  # noqa: E402
from bench_state_store import median, timed_fresh  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def state(n, rng):
    kv = {}
    for i in range(n):
        key = hashlib.sha256(b'did:%d' % i).digest() if i % 3 else b'attr:%d' % i
        kv[key] = sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])
    return sorted(kv.items())


def wall(fn, window):
    fn()
    ts, t0 = [], time.perf_counter()
    while not ts or (time.perf_counter() - t0 < window and len(ts) < 200):
        a = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - a) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rng = random.Random(1500)
    res = {'tool': 'tools/bench_state_build.py', 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    t = lambda arr: torch.from_numpy(np.array(arr)).to(dev)   # noqa: E731
    root = np.zeros(32, np.uint8)
    last = None

    def create(nodes, nbytes):
        h = ctypes.c_int32(0)
        nat._check('pv_state_store_create', lib.pv_state_store_create(nodes, nbytes, 0, ctypes.byref(h)))
        return h.value

    for n in a.sizes:
        prs = state(n, rng)
        kblob, koff = nat.pack_messages([k for k, _ in prs])
        vblob, voff = nat.pack_messages([v for _, v in prs])
        d_k = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
        d_v = torch.frombuffer(bytearray(vblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
        d_ko, d_vo = t(koff.view(np.int64)), t(voff.view(np.int64))
        nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

        def build(store, blob=None, bcap=0, off=None, ncap=0, dig=None):
            nat._check('pv_state_build_device', lib.pv_state_build_device(
                p(d_k), p(d_ko), p(d_v), p(d_vo), n, store, sst._root_ptr(root), ctypes.byref(nn), ctypes.byref(nb),
                p(blob), bcap, p(off), ncap, p(dig), 0, stream()))
        build(-1)                                                   # sizes
        nodes, nbytes = nn.value, nb.value
        o_blob = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
        o_off = torch.zeros(nodes + 1, dtype=torch.int64, device=dev)
        o_dig = torch.zeros(nodes * 32, dtype=torch.uint8, device=dev)
        s = {'keys': n, 'nodes': nodes, 'node_bytes': nbytes, 'key_bytes': int(koff[-1]), 'value_bytes': int(voff[-1])}
        runs = [timed(lambda: build(-1, o_blob, nbytes, o_off, nodes, o_dig), a.window) for _ in range(a.repeat)]
        s['build'] = {'runs': runs, 'ms': median(runs)}
        runs = [timed_fresh(lib, lambda: create(nodes, nbytes), lambda sid: build(sid), a.window)
                for _ in range(a.repeat)]
        s['build_store'] = {'runs': runs, 'ms': median(runs)}
        dig2 = torch.zeros(nodes * 32, dtype=torch.uint8, device=dev)
        runs = [timed(lambda: nat._check('pv_sha3_256_batch_device', lib.pv_sha3_256_batch_device(
            p(o_blob), p(o_off), nodes, p(dig2), 0, stream())), a.window) for _ in range(a.repeat)]
        assert torch.equal(dig2, o_dig), 'k_sha3_256 and the build disagree on a digest'
        s['sha3_floor'] = {'runs': runs, 'ms': median(runs)}
        runs = [timed_fresh(lib, lambda: create(nodes, nbytes),
                            lambda sid: nat._check('pv_state_store_add_device', lib.pv_state_store_add_device(
                                sid, p(o_blob), p(o_off), nodes, None, stream())), a.window) for _ in range(a.repeat)]
        s['store_add'] = {'runs': runs, 'ms': median(runs)}
        for name in ('build', 'build_store', 'sha3_floor', 'store_add'):
            s[name]['keys_per_s'] = n / s[name]['ms'] * 1e3
            s[name]['nodes_per_s'] = nodes / s[name]['ms'] * 1e3
        s['build_over_sha3_floor'] = s['build']['ms'] / s['sha3_floor']['ms']
        s['build_store_over_store_add'] = s['build_store']['ms'] / s['store_add']['ms']
        if n <= a.mirror_max:
            t0 = time.perf_counter()
            m_root, m_db = sst.build_encoded_host(prs)
            dt = time.perf_counter() - t0
            assert m_root == root.tobytes(), 'the mirror and the GPU disagree on the root'
            h_dig = o_dig.cpu().numpy().reshape(-1, 32)
            assert set(m_db) == {h_dig[i].tobytes() for i in range(nodes)}, 'the mirror and the GPU disagree on a node'
            s['mirror'] = {'ms': dt * 1e3, 'keys_per_s': n / dt, 'nodes_per_s': nodes / dt,
                           'note': 'a Python port of the build, one thread; not the reference implementation'}
        res['sizes'][str(n)] = s
        print(n, {k: (round(v['ms'], 4) if isinstance(v, dict) else v) for k, v in s.items()})
        last = (prs, build, nodes, nbytes)

    # ---- the Python dispatch: host form against the mirror, wall clock
    disp = {}
    for m in (4, 8, 16, 32, 64, 96, 128, 160, 192, 256, 1024):   # names of their own: build() above closes over n
        small = state(m, rng)
        disp[str(m)] = {'gpu_ms': wall(lambda: sst._build_gpu(small, -1), 0.2),
                        'mirror_ms': wall(lambda: sst.build_encoded_host(small), 0.2)}
    res['dispatch'] = disp
    print('dispatch', {k: (round(v['gpu_ms'], 3), round(v['mirror_ms'], 3)) for k, v in disp.items()})

    # ---- the larger state: walk, pack and verify from the store the build filled
    if a.queries and last:
        prs, build, nodes, nbytes = last
        Q = a.queries
        sid = create(nodes, nbytes)
        build(sid)
        the_root = root.tobytes()
        pick = [rng.randrange(len(prs)) for _ in range(Q)]
        keys = [prs[j][0] for j in pick]
        kblob, koff = nat.pack_messages(keys)
        d_qk = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
        d_qoff = t(koff.view(np.int64))
        d_root = torch.frombuffer(bytearray(the_root), dtype=torch.uint8).to(dev)
        d_ridx = torch.zeros(Q, dtype=torch.int32, device=dev)
        max_nodes = 2 * max(len(k) for k in keys) + 1
        status = torch.zeros(Q, dtype=torch.uint8, device=dev)
        count = torch.zeros(Q, dtype=torch.int32, device=dev)
        ids = torch.zeros(Q * max_nodes, dtype=torch.int32, device=dev)
        plen, vrel, vlen = (torch.zeros(Q, dtype=torch.int64, device=dev) for _ in range(3))

        def walk():
            nat._check('pv_state_store_walk_device', lib.pv_state_store_walk_device(
                sid, p(d_root), p(d_ridx), 1, p(d_qk), p(d_qoff), Q, max_nodes, p(status), p(count), p(ids), p(plen),
                p(vrel), p(vlen), stream()))
        runs = [timed(walk, a.window) for _ in range(a.repeat)]
        assert int(status.max()) == sp.PV_SP_OK, 'a walk did not end OK'
        big = {'keys': len(prs), 'nodes': nodes, 'node_bytes': nbytes, 'queries': Q,
               'hashed_nodes_per_query': int(count.sum()) / Q}
        big['walk'] = {'runs': runs, 'ms': median(runs), 'queries_per_s': Q / median(runs) * 1e3}
        poff = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        poff[1:] = torch.cumsum(plen, 0)
        total = int(poff[-1])
        out = torch.zeros(total + 16, dtype=torch.uint8, device=dev)

        def pack():
            nat._check('pv_state_store_pack_device', lib.pv_state_store_pack_device(
                sid, p(ids), p(count), max_nodes, p(poff), Q, p(out), stream()))
        runs = [timed(pack, a.window) for _ in range(a.repeat)]
        big['pack'] = {'runs': runs, 'ms': median(runs), 'queries_per_s': Q / median(runs) * 1e3, 'proof_bytes': total}
        h_off, h_out = poff.cpu().numpy(), out.cpu().numpy()
        h_vrel, h_vlen = vrel.cpu().numpy(), vlen.cpu().numpy()
        beg, end, first = [], [], [0]
        for q in range(Q):
            o = int(h_off[q])
            for b, e in sp.rlp_split_list(h_out[o:int(h_off[q + 1])].tobytes()):
                beg.append(o + b)
                end.append(o + e)
            first.append(len(beg))
        for q in range(0, Q, 997):
            o = int(h_off[q] + h_vrel[q])
            assert h_out[o:o + int(h_vlen[q])].tobytes() == prs[pick[q]][1], 'a generated value differs from the state'
        vblob, voff = nat.pack_messages([prs[j][1] for j in pick])
        d_qv = torch.frombuffer(bytearray(vblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
        d_qvoff = t(voff.view(np.int64))
        d_beg, d_end, d_first = t(np.array(beg, np.int64)), t(np.array(end, np.int64)), t(np.array(first, np.int64))
        d_roots = torch.frombuffer(bytearray(the_root * Q), dtype=torch.uint8).to(dev)
        d_pidx = t(np.arange(Q, dtype=np.int32))
        vstatus = torch.ones(Q, dtype=torch.uint8, device=dev)
        dig = torch.zeros(len(beg) * 32, dtype=torch.uint8, device=dev)

        def verify():
            nat._check('pv_state_proof_verify_device', lib.pv_state_proof_verify_device(
                p(out), p(d_beg), p(d_end), p(d_first), p(d_roots), p(d_pidx), p(d_qk), p(d_qoff), p(d_qv), p(d_qvoff),
                len(beg), Q, Q, p(vstatus), p(dig), 0, stream()))
        runs = [timed(verify, a.window) for _ in range(a.repeat)]
        assert int(vstatus.max()) == sp.PV_SP_OK, 'a generated proof does not verify'
        big['verify_same'] = {'runs': runs, 'ms': median(runs), 'queries_per_s': Q / median(runs) * 1e3}
        nat._check('pv_state_store_free', lib.pv_state_store_free(sid))
        res['large_state'] = big
        print('large_state', {k: (round(v['ms'], 4) if isinstance(v, dict) else v) for k, v in big.items()})

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--sizes', type=lambda s: [int(x) for x in s.split(',')], default=[4096, 65536, 1 << 20])
    ap.add_argument('--queries', type=int, default=1 << 18)
    ap.add_argument('--mirror-max', type=int, default=1 << 20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_build.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_build: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
