"""Measure pruning the resident trie store (pv_state_store_prune) on one GPU.

    python tools/bench_state_prune.py [--repeat 3] [--state 1048576] [--batches 10] [--ops 10000]
                                      [--removals 0.1] [--out profiles/state_prune.json]

The method of tools/bench_state_apply.py: HIP events around the C-ABI entry point (which ends
with a stream synchronize), one warm-up per shape, every shape repeated --repeat times with the
shapes that are compared alternating repeat by repeat, medians, and the smallest and largest
repeat as the run-to-run spread.  A prune consumes its store, so every timed call gets a fresh
one, prepared outside the events: a mixed state of --state keys (two thirds 32-byte keys, values
of 2 - 250 bytes) built into a store (pv_state_build_device), then --batches batches of --ops
operations applied with insert (pv_state_apply_device), each onto the root before it: --removals
of them removals of keys of the state, the others half overwrites, half new keys.

  prune_last       pv_state_store_prune (apply) to the last root
  prune_last3      ... to the last three roots
  report_last      the reporting call (apply == 0) to the last root: mark, flags and scans only
  phases           pv_time_state_store_prune on further fresh stores: mark / scans + copy / rehash
  rebuild          the only alternative without this call: pv_state_build_device of the final key
                   set into a fresh, empty store (created outside the events)

and the store's nodes and bytes before and after.  After the prune the last root is checked to
serve a proof.  Writes one JSON line.  Without a GPU it fails.
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
from bench_state_update import upload  # noqa: E402
from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402
from plenum_gpu import state_store as sst  # noqa: E402


def spread(ms):
    ms = sorted(ms)
    return {'ms': ms[len(ms) // 2], 'ms_lo': ms[0], 'ms_hi': ms[-1], 'calls': len(ms)}


def batches_onto(base, count, ops, share, rng):
    """`count` batches of `ops` operations, each onto the state the one before leaves -> ([sorted
    (key, encoded value or b'') pairs], the final state)"""
    cur, out = dict(base), []
    for b in range(count):
        n_rm = int(ops * share)
        n_over = (ops - n_rm) // 2
        picked = rng.sample(list(cur), n_rm + n_over)
        batch = {k: b'' for k in picked[:n_rm]}
        for k in picked[n_rm:]:
            batch[k] = sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])
        i = 0
        while len(batch) < ops:
            key = hashlib.sha256(b'did:new:%d:%d' % (b, i)).digest() if i % 3 else b'attr:new:%d:%d' % (b, i)
            batch[key] = sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])
            i += 1
        for k, v in batch.items():
            if v:
                cur[k] = v
            else:
                del cur[k]
        out.append(sorted(batch.items()))
    return out, cur


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rng = random.Random(1800)
    res = {'tool': 'tools/bench_state_prune.py', 'device': torch.cuda.get_device_name(0)}
    prs = state(a.state, rng)
    batches, final = batches_onto(dict(prs), a.batches, a.ops, a.removals, rng)
    base_arrs = upload(prs, dev)
    batch_arrs = [upload(b, dev) for b in batches]
    final_prs = sorted(final.items())
    final_arrs = upload(final_prs, dev)
    root, new = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    nn, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def create(nodes=1, nbytes=0):
        h = ctypes.c_int32(0)
        nat._check('pv_state_store_create', lib.pv_state_store_create(nodes, nbytes, 0, ctypes.byref(h)))
        return h.value

    def build(xs, count, sid):
        nat._check('pv_state_build_device', lib.pv_state_build_device(
            p(xs[0]), p(xs[1]), p(xs[2]), p(xs[3]), count, sid, sst._root_ptr(root), ctypes.byref(nn),
            ctypes.byref(nb), None, 0, None, 0, None, 0, stream()))

    def prepare():
        """a fresh store holding the state and every batch -> (store id, [the root after each step])"""
        sid = create()
        build(base_arrs, len(prs), sid)
        roots = [root.tobytes()]
        for xs, b in zip(batch_arrs, batches):
            old = np.frombuffer(roots[-1], np.uint8).copy()
            nat._check('pv_state_apply_device', lib.pv_state_apply_device(
                sid, sst._root_ptr(old), p(xs[0]), p(xs[1]), p(xs[2]), p(xs[3]), len(b), 1, sst._root_ptr(new),
                ctypes.byref(nn), ctypes.byref(nb), None, 0, None, 0, None, stream()))
            roots.append(new.tobytes())
        return sid, roots

    def info(sid):
        v = [ctypes.c_uint64(0) for _ in range(4)]
        nat._check('pv_state_store_info', lib.pv_state_store_info(sid, *[ctypes.byref(x) for x in v]))
        return dict(zip(('n_nodes', 'n_unique', 'n_bytes', 'n_slots'), (x.value for x in v)))

    kept, kbytes, missing = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)

    def prune(sid, keep, apply):
        rts = np.frombuffer(b''.join(keep), np.uint8).copy()
        nat._check('pv_state_store_prune', lib.pv_state_store_prune(
            sid, nat._ptr(rts), len(keep), apply, None, ctypes.byref(kept), ctypes.byref(kbytes),
            ctypes.byref(missing), None, 0))

    def phases(sid, keep):
        rts = np.frombuffer(b''.join(keep), np.uint8).copy()
        ms = [ctypes.c_float(0) for _ in range(3)]
        nat._check('pv_time_state_store_prune', lib.pv_time_state_store_prune(
            sid, nat._ptr(rts), len(keep), ctypes.byref(kept), ctypes.byref(kbytes), *[ctypes.byref(x) for x in ms]))
        return [x.value for x in ms]

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def free(sid):
        nat._check('pv_state_store_free', lib.pv_state_store_free(sid))

    sid, roots = prepare()
    before = info(sid)
    build(final_arrs, len(final_prs), -1)
    assert root.tobytes() == roots[-1], 'the batches and the rebuild disagree on the final root'
    res['state'] = {'keys': len(prs), 'batches': a.batches, 'operations': a.ops, 'removals': a.removals,
                    'final_keys': len(final_prs), 'rebuild_nodes': nn.value, 'rebuild_bytes': nb.value}
    res['before'] = before
    print('state', res['state'], 'before', before)
    shapes = {'last': roots[-1:], 'last3': roots[-3:]}
    res['report_last'] = timed(lambda: prune(sid, roots[-1:], 0), 0.5)
    assert info(sid) == before
    # warm-up of every shape: one consumed store each
    for keep in shapes.values():
        prune(sid, keep, 1)
        free(sid)
        sid, _ = prepare()
    free(sid)
    runs = {'prune_last': [], 'prune_last3': [], 'rebuild': []}
    ph = {'last': [], 'last3': []}
    for _ in range(a.repeat):
        for name, keep in shapes.items():
            sid, _ = prepare()
            torch.cuda.synchronize()
            runs['prune_' + name].append(event_ms(lambda: prune(sid, keep, 1)))
            after = info(sid)
            assert after['n_nodes'] == after['n_unique'] == kept.value and after['n_bytes'] == kbytes.value
            res['after_' + name] = dict(after, n_missing=missing.value)
            free(sid)
            sid, _ = prepare()
            torch.cuda.synchronize()
            ph[name].append(phases(sid, keep))
            free(sid)
        sid = create()
        torch.cuda.synchronize()
        runs['rebuild'].append(event_ms(lambda: build(final_arrs, len(final_prs), sid)))
        res['after_rebuild'] = info(sid)
        free(sid)
    for k, v in runs.items():
        res[k] = spread(v)
    for name, rows in ph.items():
        res['phases_' + name] = {k: spread([r[i] for r in rows]) for i, k in enumerate(('mark', 'scan_copy', 'rehash'))}
    res['prune_last_over_rebuild'] = res['prune_last']['ms'] / res['rebuild']['ms']
    res['prune_last3_over_rebuild'] = res['prune_last3']['ms'] / res['rebuild']['ms']
    # the pruned store still serves its root
    sid, roots = prepare()
    prune(sid, roots[-1:], 1)
    st = sst.GpuStateStore.__new__(sst.GpuStateStore)
    st._lib, st._id, st.device = lib, sid, 0
    key = final_prs[len(final_prs) // 2][0]
    proof, value = st.generate_state_proof(key, roots[-1], serialize=True, get_value=True)
    assert value == final[key] and proof
    free(sid)
    for k in ('report_last', 'prune_last', 'prune_last3', 'phases_last', 'phases_last3', 'rebuild',
              'prune_last_over_rebuild', 'prune_last3_over_rebuild', 'after_last', 'after_last3', 'after_rebuild'):
        print(k, res[k])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--state', type=int, default=1 << 20)
    ap.add_argument('--batches', type=int, default=10)
    ap.add_argument('--ops', type=int, default=10000)
    ap.add_argument('--removals', type=float, default=0.1)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_prune.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_prune: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
