"""Measure the Merkle proof kernels on one GPU, everything device-resident.

    python tools/bench_merkle_proofs.py [--repeat 3] [--window 0.5]

Timed with HIP events around the C-ABI device entry points (each ends with a
stream synchronize), one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times to show the spread.  Shapes:

  build          a 2^20-leaf tree from leaf hashes (pv_merkle_tree_extend_hashes_device)
  extend_1000    1,000 more leaf hashes onto it
  paths_full     1M audit paths at s == n (read from the levels, nothing hashed)
  paths_prefix   1M audit paths at random s < n (right-edge chain hashed per request)
  verify_incl    1M inclusion proofs of depth 20 (k_merkle_verify_incl)
  verify_cons    100k consistency proofs (k_merkle_verify_cons)
  leaf_sha256    k_sha256 over 2^20 leaves of 256 B with the 0x00 prefix (5 compressions each)

For verify_incl the line records SHA-256 compressions per second, 2 per proof
node, counted here from the proof lengths, beside the leaf kernel's rate from
the same run, and a one-thread hashlib port of the same walk on this host (a
port, not the reference implementation).  Writes one JSON line to
profiles/merkle_proofs.json.  Without a GPU it fails.
"""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, 'indy-plenum_amd'))

import torch  # noqa: E402

from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu.merkle_proofs import STH, GpuMerkleVerifier  # noqa: E402

N = 1 << 20
DEPTH = 20
Q = 1 << 20          # path / inclusion requests
QC = 100000          # consistency requests


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(name, rc):
    nat._check(name, rc)


def timed(fn, window, setup=None):
    """milliseconds per call: HIP events around fn(), calls repeated for >= window seconds"""
    ms, calls, t0 = [], 0, time.perf_counter()
    while not ms or time.perf_counter() - t0 < window:
        arg = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg) if setup else fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        calls += 1
        if calls >= 4000:
            break
    ms.sort()
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'calls': calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_merkle_proofs: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(6962)
    u8, i64 = torch.uint8, torch.int64

    # ---- leaf kernel: 2^20 leaves of 256 B -> the tree's leaf hashes
    blob = torch.randint(0, 256, (N * 256 + 16,), dtype=u8, device=dev, generator=g)
    off = (torch.arange(N + 1, dtype=i64, device=dev) * 256)
    leaf_hashes = torch.zeros((N, 32), dtype=u8, device=dev)

    def leaf_sha():
        check('pv_sha256_batch_device', lib.pv_sha256_batch_device(p(blob), p(off), N, 0, p(leaf_hashes), 0, stream()))

    # ---- tree build / extend
    handles = []

    def new_tree():
        h = ctypes.c_int32(0)
        check('pv_merkle_tree_create', lib.pv_merkle_tree_create(1 << 22, 0, ctypes.byref(h)))
        handles.append(h.value)
        return h.value

    def free_all_but(keep):
        for h in handles:
            if h != keep:
                lib.pv_merkle_tree_free(h)
        handles[:] = [keep] if keep else []

    def build(h):
        check('pv_merkle_tree_extend_hashes_device',
              lib.pv_merkle_tree_extend_hashes_device(h, p(leaf_hashes), N, stream()))

    grown = {'n': 0}

    def extend_1000(h):
        check('pv_merkle_tree_extend_hashes_device',
              lib.pv_merkle_tree_extend_hashes_device(h, p(leaf_hashes), 1000, stream()))
        grown['n'] += 1000

    # ---- requests
    stride = DEPTH + 1
    index = torch.randint(0, N, (Q,), dtype=i64, device=dev, generator=g)
    size_full = torch.full((Q,), N, dtype=i64, device=dev)
    size_pre = torch.randint(1, N, (Q,), dtype=i64, device=dev, generator=g)
    index_pre = index % size_pre
    nodes = torch.zeros((Q, stride, 32), dtype=u8, device=dev)
    lens = torch.zeros(Q, dtype=torch.int32, device=dev)
    roots = torch.zeros((Q, 32), dtype=u8, device=dev)
    tree = {}

    def paths(idx, size):
        check('pv_merkle_audit_paths_device',
              lib.pv_merkle_audit_paths_device(tree['h'], p(idx), p(size), Q, p(nodes), p(lens), p(roots), stream()))

    status = torch.zeros(Q, dtype=u8, device=dev)
    computed = torch.zeros((Q, 32), dtype=u8, device=dev)
    stop = torch.zeros(Q, dtype=i64, device=dev)
    vin = {}

    def verify_incl():
        check('pv_merkle_verify_inclusion_device', lib.pv_merkle_verify_inclusion_device(
            p(vin['leaf']), None, None, p(index), p(size_full), p(vin['nodes']), p(vin['off']), p(vin['roots']),
            None, 0, Q, p(status), p(computed), p(stop), 0, stream()))

    vc = {}

    def verify_cons():
        check('pv_merkle_verify_consistency_device', lib.pv_merkle_verify_consistency_device(
            p(vc['first']), p(vc['second']), p(vc['r0']), p(vc['r1']), None, None, 0, p(vc['nodes']), p(vc['off']),
            QC, p(vc['status']), p(vc['c0']), p(vc['c1']), 0, stream()))

    out = {'tool': 'tools/bench_merkle_proofs.py', 'device': torch.cuda.get_device_name(0), 'leaves': N,
           'requests': Q, 'consistency_requests': QC, 'window_s': a.window, 'runs': []}
    for rep in range(a.repeat):
        rec = {}
        leaf_sha()                                   # warm-up
        rec['leaf_sha256'] = timed(leaf_sha, a.window)
        free_all_but(None)
        build(new_tree())                            # warm-up
        free_all_but(None)
        rec['build'] = timed(build, a.window, setup=lambda: (free_all_but(None), new_tree())[1])
        tree['h'] = handles[-1]
        free_all_but(tree['h'])
        n_info, d_info = ctypes.c_uint64(0), ctypes.c_uint32(0)
        check('pv_merkle_tree_info', lib.pv_merkle_tree_info(tree['h'], ctypes.byref(n_info), ctypes.byref(d_info),
                                                             None))
        assert (n_info.value, d_info.value) == (N, DEPTH)
        paths(index, size_full)                      # warm-up; also the proofs verify_incl checks
        rec['paths_full'] = timed(lambda: paths(index, size_full), a.window)
        assert int(lens.min()) == DEPTH == int(lens.max())
        vin['nodes'] = nodes[:, :DEPTH].contiguous()
        vin['off'] = torch.arange(Q + 1, dtype=i64, device=dev) * DEPTH
        vin['roots'] = roots.clone()
        vin['leaf'] = leaf_hashes[index].contiguous()
        verify_incl()
        assert int(status.max()) == 0, 'generated paths must verify'
        rec['verify_incl'] = timed(verify_incl, a.window)
        compressions = 2 * int(lens.to(i64).sum())   # two per proof node, counted from the proofs
        rec['verify_incl']['compressions'] = compressions
        rec['verify_incl']['compressions_per_s'] = compressions / (rec['verify_incl']['ms_median'] * 1e-3)
        rec['leaf_sha256']['compressions'] = 5 * N
        rec['leaf_sha256']['compressions_per_s'] = 5 * N / (rec['leaf_sha256']['ms_median'] * 1e-3)
        rec['verify_incl']['ratio_to_leaf_kernel'] = (rec['verify_incl']['compressions_per_s'] /
                                                      rec['leaf_sha256']['compressions_per_s'])
        paths(index_pre, size_pre)
        rec['paths_prefix'] = timed(lambda: paths(index_pre, size_pre), a.window)
        assert int(lens.max()) <= DEPTH
        # consistency proofs of random pairs, compacted on the device, with their roots
        second = torch.randint(2, N + 1, (QC,), dtype=i64, device=dev, generator=g)
        first = 1 + torch.randint(0, N, (QC,), dtype=i64, device=dev, generator=g) % (second - 1)
        pn = torch.zeros((QC, stride, 32), dtype=u8, device=dev)
        pl = torch.zeros(QC, dtype=torch.int32, device=dev)
        check('pv_merkle_consistency_proofs_device',
              lib.pv_merkle_consistency_proofs_device(tree['h'], p(first), p(second), QC, p(pn), p(pl), stream()))
        keep = torch.arange(stride, device=dev)[None, :] < pl[:, None]
        vc['nodes'] = pn[keep].contiguous()
        vc['off'] = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(pl.to(i64), 0)])
        zero = torch.zeros(QC, dtype=i64, device=dev)
        rr = torch.zeros((2, QC, 32), dtype=u8, device=dev)
        scratch_nodes = torch.zeros((QC, stride, 32), dtype=u8, device=dev)
        scratch_len = torch.zeros(QC, dtype=torch.int32, device=dev)
        for j, sz in enumerate((first, second)):
            check('pv_merkle_audit_paths_device',
                  lib.pv_merkle_audit_paths_device(tree['h'], p(zero), p(sz), QC, p(scratch_nodes), p(scratch_len),
                                                   p(rr[j]), stream()))
        vc.update(first=first, second=second, r0=rr[0], r1=rr[1], status=torch.zeros(QC, dtype=u8, device=dev),
                  c0=torch.zeros((QC, 32), dtype=u8, device=dev), c1=torch.zeros((QC, 32), dtype=u8, device=dev))
        verify_cons()
        assert int(vc['status'].max()) == 0, 'generated consistency proofs must verify'
        rec['verify_cons'] = timed(verify_cons, a.window)
        rec['verify_cons']['proof_nodes'] = int(pl.to(i64).sum())
        grown['n'] = 0
        extend_1000(tree['h'])
        rec['extend_1000'] = timed(lambda: extend_1000(tree['h']), a.window)
        rec['extend_1000']['leaves_added'] = grown['n']
        free_all_but(None)
        out['runs'].append(rec)

    # one-thread hashlib port of the same walk on this host (a port, not the reference)
    k = 2000
    hn = vin['nodes'][:k].cpu().numpy()
    hl = vin['leaf'][:k].cpu().numpy()
    hr = vin['roots'][:k].cpu().numpy()
    hi = index[:k].cpu().numpy()
    v = GpuMerkleVerifier()
    items = [(hl[j].tobytes(), int(hi[j]), [hn[j, i].tobytes() for i in range(DEPTH)], STH(N, hr[j].tobytes()))
             for j in range(k)]
    t0 = time.perf_counter()
    for it in items:
        v.verify_leaf_hash_inclusion(*it)
    dt = time.perf_counter() - t0
    out['hashlib_port_one_thread'] = {'proofs': k, 'proofs_per_s': k / dt, 'compressions_per_s': 2 * DEPTH * k / dt,
                                      'note': 'Python/hashlib port of the walk on this host, not the reference'}
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    line = json.dumps(out, sort_keys=True)
    with open(os.path.join(REPO, 'profiles', 'merkle_proofs.json'), 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
