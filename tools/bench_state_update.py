"""Measure sets onto a committed root (pv_state_update_device) on one GPU, device-resident.

    python tools/bench_state_update.py [--repeat 3] [--window 0.5] [--state 1048576]
                                       [--batches 100,1000,10000,100000] [--carried-max 100000]
                                       [--out profiles/state_update.json]

The method of tools/bench_state_build.py: HIP events around the C-ABI device entry points
(each ends with a stream synchronize), one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times, medians.  A mixed state of --state keys (two
thirds 32-byte keys, values of 2 - 250 bytes) is built into a store once.  Per batch size, a
batch of that many sets, half of them new keys and half overwrites of keys of the state:

  update           pv_state_update_device at the state's root with insert = 0 (so every call sees
                   the same store), no node outputs: the new root and the sizes
  update_outputs   the same with the node blob, offsets and digests written
  update_insert    the same with insert = 1 into the store, timed once per repeat (each call
                   grows the store, and re-inserting equal nodes only flags duplicates)
  rebuild          pv_state_build_device over all keys of the updated state, no store, no outputs:
                   the only route to that root without this call

and the nodes and node bytes the update emits, the nodes of the rebuild, and, up to
--carried-max batch keys, the merged list's length from the Python mirror over the store's
nodes (items per batch key: the key's own value plus what it carries).  The update's root is
checked against the rebuild's.  Writes one JSON line.  Without a GPU it fails.
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

from bench_state_build import state  # noqa: E402
from bench_state_proofs import p, stream, timed  # noqa: E402
from bench_state_store import median  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def upload(prs, dev):
    kblob, koff = nat.pack_messages([k for k, _ in prs])
    vblob, voff = nat.pack_messages([v for _, v in prs])
    d_k = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
    d_v = torch.frombuffer(bytearray(vblob.tobytes() + b'\0' * 16), dtype=torch.uint8).to(dev)
    t = lambda arr: torch.from_numpy(np.array(arr)).to(dev)   # noqa: E731
    return d_k, t(koff.view(np.int64)), d_v, t(voff.view(np.int64))


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rng = random.Random(1600)
    res = {'tool': 'tools/bench_state_update.py', 'device': torch.cuda.get_device_name(0), 'batches': {}}
    prs = state(a.state, rng)
    n = len(prs)
    base = dict(prs)
    d_k, d_ko, d_v, d_vo = upload(prs, dev)
    root, nn, nb = np.zeros(32, np.uint8), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def build(arrs, count, store, blob=None, bcap=0, off=None, ncap=0, dig=None):
        nat._check('pv_state_build_device', lib.pv_state_build_device(
            p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), count, store, sst._root_ptr(root), ctypes.byref(nn),
            ctypes.byref(nb), p(blob), bcap, p(off), ncap, p(dig), 0, stream()))
    build((d_k, d_ko, d_v, d_vo), n, -1)
    nodes, nbytes = nn.value, nb.value
    h = ctypes.c_int32(0)
    nat._check('pv_state_store_create', lib.pv_state_store_create(2 * nodes, 2 * nbytes, 0, ctypes.byref(h)))
    sid = h.value
    o_blob = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    o_off = torch.zeros(nodes + 1, dtype=torch.int64, device=dev)
    o_dig = torch.zeros(nodes * 32, dtype=torch.uint8, device=dev)
    build((d_k, d_ko, d_v, d_vo), n, sid, o_blob, nbytes, o_off, nodes, o_dig)
    old_root = root.copy()
    res['state'] = {'keys': n, 'nodes': nodes, 'node_bytes': nbytes}
    print('state', res['state'])
    db = None
    if a.carried_max:
        h_blob, h_off, h_dig = o_blob.cpu().numpy(), o_off.cpu().numpy(), o_dig.cpu().numpy().reshape(-1, 32)
        db = {h_dig[i].tobytes(): h_blob[int(h_off[i]):int(h_off[i + 1])].tobytes() for i in range(nodes)}
        del h_blob, h_off, h_dig
    del o_blob, o_off, o_dig
    new = np.zeros(32, np.uint8)

    for m in a.batches:
        batch = {k: sp.rlp_encode([rng.randbytes(rng.randint(2, 250))]) for k in rng.sample(sorted(base), m // 2)}
        i = 0
        while len(batch) < m:
            key = hashlib.sha256(b'did:new:%d:%d' % (m, i)).digest() if i % 3 else b'attr:new:%d:%d' % (m, i)
            batch[key] = sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])
            i += 1
        bprs = sorted(batch.items())
        b_arrs = upload(bprs, dev)
        union = dict(base)
        union.update(batch)
        u_arrs = upload(sorted(union.items()), dev)

        def update(insert, blob=None, bcap=0, off=None, ncap=0, dig=None):
            nat._check('pv_state_update_device', lib.pv_state_update_device(
                sid, sst._root_ptr(old_root), p(b_arrs[0]), p(b_arrs[1]), p(b_arrs[2]), p(b_arrs[3]), m, insert,
                sst._root_ptr(new), ctypes.byref(nn), ctypes.byref(nb), p(blob), bcap, p(off), ncap, p(dig), stream()))
        update(0)
        e_nodes, e_bytes = nn.value, nb.value
        s = {'sets': m, 'new_keys': m - m // 2, 'overwrites': m // 2, 'emitted_nodes': e_nodes, 'emitted_bytes': e_bytes}
        runs = [timed(lambda: update(0), a.window) for _ in range(a.repeat)]
        s['update'] = {'runs': runs, 'ms': median(runs)}
        x_blob = torch.zeros(e_bytes + 16, dtype=torch.uint8, device=dev)
        x_off = torch.zeros(e_nodes + 1, dtype=torch.int64, device=dev)
        x_dig = torch.zeros(e_nodes * 32, dtype=torch.uint8, device=dev)
        runs = [timed(lambda: update(0, x_blob, e_bytes, x_off, e_nodes, x_dig), a.window) for _ in range(a.repeat)]
        s['update_outputs'] = {'runs': runs, 'ms': median(runs)}
        build(u_arrs, len(union), -1)
        assert root.tobytes() == new.tobytes(), 'the update and the rebuild disagree on the root'
        s['rebuild_nodes'], s['rebuild_bytes'] = nn.value, nb.value
        runs = [timed(lambda: build(u_arrs, len(union), -1), a.window) for _ in range(a.repeat)]
        s['rebuild'] = {'runs': runs, 'ms': median(runs)}
        once = []
        for _ in range(a.repeat):
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea.record()
            update(1)
            eb.record()
            eb.synchronize()
            once.append(ea.elapsed_time(eb))
        s['update_insert'] = {'runs_ms': once, 'ms': sorted(once)[len(once) // 2]}
        s['rebuild_over_update'] = s['rebuild']['ms'] / s['update']['ms']
        s['sets_per_s'] = m / s['update']['ms'] * 1e3
        if db is not None and m <= a.carried_max:
            st, _, items = sst.merge_host(db, old_root.tobytes(), bprs)
            assert st == 0
            s['merged_items'] = len(items)
            s['items_per_key'] = len(items) / m
            s['subtree_items'] = sum(1 for it in items if it[1] == sst.ITEM_SUBTREE)
        res['batches'][str(m)] = s
        print(m, {k: (round(v['ms'], 4) if isinstance(v, dict) else v) for k, v in s.items()})
        del b_arrs, u_arrs, x_blob, x_off, x_dig

    nat._check('pv_state_store_free', lib.pv_state_store_free(sid))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--state', type=int, default=1 << 20)
    ap.add_argument('--batches', type=lambda s: [int(x) for x in s.split(',')], default=[100, 1000, 10000, 100000])
    ap.add_argument('--carried-max', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_update.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_update: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
