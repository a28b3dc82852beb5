"""Measure the SHA3-256 and state-proof kernels on one GPU, device-resident.

    python tools/bench_state_proofs.py [--repeat 3] [--window 0.5] [--proofs 262144]

Timed with HIP events around the C-ABI device entry points (each ends with a
stream synchronize), one warm-up per shape, windows of at least --window
seconds, every shape repeated --repeat times to show the spread.  Shapes:

  sha3_136        k_sha3_256 over 2^20 messages of 100..135 bytes (one 136-byte block each)
  sha3_nodes      k_sha3_256 over 2^20 messages with the length mix of trie nodes
                  (leaves 40..200 B, branches ~532 B: 1..4 blocks)
  state_proofs    pv_state_proof_verify_device over --proofs proofs of a 4,096-key trie built
                  by the Python mirror (every proof's nodes hashed, then walked)
  sha256_same_run k_sha256 over 2^20 messages of 119 bytes (2 compressions each), for scale

For sha3_* the line records messages/s and Keccak-f[1600] permutations/s and the
fraction of an instruction ceiling computed the way bench.py prices k_sha256:
the algorithmic lane-instruction count of one permutation plus one block
assembly, by instruction class, against that mix at the measured per-instruction
rates (the newest profiles/*int_rates.json scaled to the best v_mad_u64_u32
ceiling of profiles/r01_mad_peak.json).  CPU comparands, one thread on this
host: hashlib.sha3_256 and the Python mirror's walk (a port, not the reference).
Writes one JSON line to profiles/state_proofs.json (--out names another file).  Without a GPU it fails.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from plenum_gpu import _native as nat  # noqa: E402
from plenum_gpu import state_proofs as sp  # noqa: E402

N = 1 << 20

# One Keccak-f[1600] round on 32-bit halves (pv_sha3.h): theta's C = 5 lanes x 2 halves x 2
# v_bitop3_b32, D = 5 x (2 v_alignbit_b32 + 2 v_xor_b32); rho/pi = 25 x 2 v_xor_b32 (A ^ D) + 24
# rotated lanes x 2 v_alignbit_b32 (no rotation amount of the 24 is 32); chi = 25 x 2
# v_bitop3_b32; iota = 33 v_xor_b32 over the 24 rounds.  One block adds its assembly: 34
# funnel shifts, 34 x 3 selects / masks (priced as v_bfi_b32) and 34 absorb xors.
KECCAK_W = {'v_bitop3_b32': 24 * (20 + 50), 'v_alignbit_b32': 24 * (10 + 48) + 34,
            'v_xor_b32': 24 * (10 + 50) + 33 + 34, 'v_bfi_b32': 34 * 3}
# bench.py's count for one SHA-256 compression (pv_sha256.h)
SHA256_W = {'v_alignbit_b32': 64 * 6 + 48 * 4, 'v_bitop3_b32': 64 * 4 + 48 * 2, 'v_lshrrev_b32': 48 * 2,
            'v_add3_u32': 64 + 48, 'v_add_u32': 64 * 5 + 48 + 8, 'v_perm_b32': 16}


def insn_rates():
    with open(os.path.join(REPO, 'profiles', 'r01_mad_peak.json')) as fh:
        peak = max(float(x['lane_ops_per_s']) for x in json.load(fh)['results'])
    for name in ('r06_int_rates.json', 'r01_int_rates.json'):
        path = os.path.join(REPO, 'profiles', name)
        if os.path.exists(path):
            with open(path) as fh:
                r = {}
                for x in json.load(fh)['results']:
                    r[x['insn']] = max(r.get(x['insn'], 0.0), float(x['lane_ops_per_s']))
            scale = peak / r['v_mad_u64_u32']
            return {k: v * scale for k, v in r.items()}, 'profiles/' + name
    raise SystemExit('no instruction-rate profile')


def ceiling(mix, rates):
    """blocks/s of the whole chip at that instruction mix"""
    return 1.0 / sum(w / rates.get(k, rates['v_alignbit_b32']) for k, w in mix.items())


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, window):
    ms, t0 = [], time.perf_counter()
    fn()
    torch.cuda.synchronize()
    while not ms or (time.perf_counter() - t0 < window and len(ms) < 2000):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'calls': len(ms)}


def dev_msgs(lens, dev, seed):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    g = torch.Generator(device=dev).manual_seed(seed)
    blob = torch.randint(0, 256, (int(off[-1]) + 16,), dtype=torch.uint8, device=dev, generator=g)
    return blob, torch.from_numpy(off).to(dev), off


def build_trie(keys_values):
    """A trie over (key, encoded value) pairs built bottom-up -> (root hash, {hash: node RLP})"""
    db = {}

    def hp(nibbles, leaf):
        flags = (2 if leaf else 0) + (len(nibbles) & 1)
        nib = ([flags] if len(nibbles) & 1 else [flags, 0]) + list(nibbles)
        return bytes(16 * nib[i] + nib[i + 1] for i in range(0, len(nib), 2))

    def ref(node):
        enc = sp.rlp_encode(node)
        if len(enc) < 32:
            return node
        h = hashlib.sha3_256(enc).digest()
        db[h] = enc
        return h

    def make(items, depth):
        if not items:
            return b''
        if len(items) == 1:
            k, v = items[0]
            return ref([hp(k[depth:], True), v])
        first = items[0][0]
        common = 0
        while all(len(k) > depth + common and k[depth + common] == first[depth + common] for k, _ in items):
            common += 1
        if common:
            return ref([hp(first[depth:depth + common], False), make(items, depth + common)])
        slots, value = [[] for _ in range(16)], b''
        for k, v in items:
            if len(k) == depth:
                value = v
            else:
                slots[k[depth]].append((k, v))
        return ref([make(s, depth + 1) for s in slots] + [value])

    items = sorted(([n for b in k for n in (b >> 4, b & 15)], v) for k, v in keys_values)
    top = make(items, 0)
    if not isinstance(top, bytes) or len(top) != 32:
        enc = sp.rlp_encode(top)
        top = hashlib.sha3_256(enc).digest()
        db[top] = enc
    return top, db


def proof_of(root, db, key):
    """the hashed nodes on key's path, root last (as generate_state_proof orders them)"""
    out, nib = [], [n for b in key for n in (b >> 4, b & 15)]

    def walk(h, depth):
        enc = db[h]
        out.append(enc)
        node = enc
        while True:
            rng = sp.rlp_split_list(node)
            if len(rng) == 17:
                if depth == len(nib):
                    return
                b, e = rng[nib[depth]]
                depth += 1
            else:
                b0, e0 = rng[0]
                _, pb, pe = sp._rlp_item(node, b0, e0)
                flags = node[pb] >> 4
                if flags & 2:
                    return
                depth += 2 * (pe - pb - 1) + (flags & 1)
                b, e = rng[1]
            il, pb, pe = sp._rlp_item(node, b, e)
            if il:
                node = node[b:e]
                continue
            if pe - pb == 32:
                walk(node[pb:pe], depth)
            return

    walk(root, 0)
    return out[::-1]


def run(a):
    lib = nat.load()
    dev = torch.device('cuda:0')
    rates, rates_src = insn_rates()
    res = {'tool': 'tools/bench_state_proofs.py', 'device': torch.cuda.get_device_name(0), 'rates_source': rates_src,
           'keccak_insn_per_block': KECCAK_W, 'keccak_insn_total': sum(KECCAK_W.values()), 'shapes': {}}
    rng = random.Random(1600)

    def sha3_shape(name, lens):
        blob, doff, off = dev_msgs(lens, dev, 3)
        out = torch.zeros(len(lens) * 32, dtype=torch.uint8, device=dev)
        blocks = int((np.asarray(lens) // 136 + 1).sum())

        def fn():
            nat._check('pv_sha3_256_batch_device',
                       lib.pv_sha3_256_batch_device(p(blob), p(doff), len(lens), p(out), 0, stream()))
        runs = [timed(fn, a.window) for _ in range(a.repeat)]
        raw = blob.cpu().numpy().tobytes()
        got = out.cpu().numpy().reshape(-1, 32)
        for i in range(0, len(lens), 4099):
            assert got[i].tobytes() == hashlib.sha3_256(raw[off[i]:off[i + 1]]).digest(), (name, i)
        ms = sorted(r['ms_median'] for r in runs)[len(runs) // 2]
        ceil = ceiling(KECCAK_W, rates)
        res['shapes'][name] = {'messages': len(lens), 'permutations': blocks, 'runs': runs, 'ms': ms,
                               'messages_per_s': len(lens) / ms * 1e3, 'permutations_per_s': blocks / ms * 1e3,
                               'ceiling_permutations_per_s': ceil, 'frac': blocks / ms * 1e3 / ceil}
        return raw, off

    raw, off = sha3_shape('sha3_136', [rng.randint(100, 135) for _ in range(N)])
    sha3_shape('sha3_nodes', [rng.choice([rng.randint(40, 200), rng.randint(40, 200), 532, rng.randint(300, 540)])
                              for _ in range(N)])
    t0 = time.perf_counter()
    k = 200000
    for i in range(k):
        hashlib.sha3_256(raw[off[i]:off[i + 1]]).digest()
    res['cpu_hashlib_sha3_messages_per_s'] = k / (time.perf_counter() - t0)

    # ---- k_sha256 in the same run
    lens = [119] * N
    blob, doff, off2 = dev_msgs(lens, dev, 4)
    out = torch.zeros(N * 32, dtype=torch.uint8, device=dev)

    def fn256():
        nat._check('pv_sha256_batch_device',
                   lib.pv_sha256_batch_device(p(blob), p(doff), N, -1, p(out), 0, stream()))
    runs = [timed(fn256, a.window) for _ in range(a.repeat)]
    ms = sorted(r['ms_median'] for r in runs)[len(runs) // 2]
    c256 = ceiling(SHA256_W, rates)
    res['shapes']['sha256_same_run'] = {'messages': N, 'compressions': 2 * N, 'runs': runs, 'ms': ms,
                                        'messages_per_s': N / ms * 1e3, 'compressions_per_s': 2 * N / ms * 1e3,
                                        'ceiling_compressions_per_s': c256, 'frac': 2 * N / ms * 1e3 / c256}

    # ---- state proofs over a 4,096-key trie
    kv = []
    for i in range(4096):
        key = hashlib.sha256(b'did:%d' % i).digest() if i % 3 else b'attr:%d' % i
        kv.append((key, sp.rlp_encode([rng.randbytes(rng.randint(2, 250))])))
    root, db = build_trie(kv)
    proofs = [proof_of(root, db, k) for k, _ in kv]
    Q = a.proofs
    pick = [rng.randrange(len(kv)) for _ in range(Q)]
    chunks, beg, end, first, pos = [], [], [], [0], 0
    ser_cache = {}
    for j in pick:
        if j not in ser_cache:
            body = b''.join(proofs[j])
            ser = sp._length_prefix(len(body), 192) + body
            ser_cache[j] = (ser, sp.rlp_split_list(ser))
        ser, ranges = ser_cache[j]
        for b, e in ranges:
            beg.append(pos + b)
            end.append(pos + e)
        chunks.append(ser)
        pos += len(ser)
        first.append(len(beg))
    keys = [kv[j][0] for j in pick]
    vals = [kv[j][1] for j in pick]
    for i in range(0, Q, 7):      # every 7th query expects another value: VALUE_MISMATCH
        vals[i] = vals[i] + b'!'
    t = lambda arr, dt: torch.from_numpy(np.asarray(arr, dt)).to(dev)   # noqa: E731
    nblob = torch.frombuffer(bytearray(b''.join(chunks) + b'\0' * 16), dtype=torch.uint8).to(dev)
    dbeg, dend, dfirst = t(beg, np.int64), t(end, np.int64), t(first, np.int64)
    droots = torch.frombuffer(bytearray(root * Q), dtype=torch.uint8).to(dev)
    dpidx = t(np.arange(Q), np.int32)
    kblob, koff = nat.pack_messages(keys)
    vblob, voff = nat.pack_messages(vals)
    dk = torch.frombuffer(bytearray(kblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
    dv = torch.frombuffer(bytearray(vblob.tobytes() + b'\0' * 4), dtype=torch.uint8).to(dev)
    dkoff, dvoff = t(koff.view(np.int64), np.int64), t(voff.view(np.int64), np.int64)
    status = torch.zeros(Q, dtype=torch.uint8, device=dev)
    dig = torch.zeros(len(beg) * 32, dtype=torch.uint8, device=dev)

    def fnsp():
        nat._check('pv_state_proof_verify_device', lib.pv_state_proof_verify_device(
            p(nblob), p(dbeg), p(dend), p(dfirst), p(droots), p(dpidx), p(dk), p(dkoff), p(dv), p(dvoff), len(beg), Q,
            Q, p(status), p(dig), 0, stream()))
    runs = [timed(fnsp, a.window) for _ in range(a.repeat)]
    st = status.cpu().numpy()
    want = np.zeros(Q, np.uint8)
    want[::7] = sp.PV_SP_VALUE_MISMATCH
    assert (st == want).all(), 'state-proof statuses differ from the expected ones'
    ms = sorted(r['ms_median'] for r in runs)[len(runs) // 2]
    nbytes = np.asarray(end) - np.asarray(beg)
    perms = int((nbytes // 136 + 1).sum())
    res['shapes']['state_proofs'] = {'queries': Q, 'proofs': Q, 'nodes': len(beg), 'nodes_per_proof': len(beg) / Q,
                                     'node_bytes': int(nbytes.sum()), 'permutations': perms, 'runs': runs, 'ms': ms,
                                     'queries_per_s': Q / ms * 1e3, 'permutations_per_s': perms / ms * 1e3}
    # the mirror, one thread, on the first 2,000 of the same queries
    k = 2000
    t0 = time.perf_counter()
    items = []
    for i in range(k):
        j = pick[i]
        items.append((root, keys[i], None, ser_cache[j][0]))
    old = sp.GPU_MIN_ITEMS
    sp.GPU_MIN_ITEMS = 1 << 62
    try:
        pk = sp._pack(items, sp.rlp_split_list)
        pk.vals = vals[:k]
        mst = sp._statuses_host(pk)
    finally:
        sp.GPU_MIN_ITEMS = old
    res['cpu_python_mirror_queries_per_s'] = k / (time.perf_counter() - t0)
    assert (mst == st[:k]).all(), 'the mirror and the GPU disagree'
    os.makedirs(os.path.join(REPO, 'profiles'), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(res) + '\n')
    for name, s in res['shapes'].items():
        print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.items() if k != 'runs'})
    print('cpu hashlib sha3 msgs/s', round(res['cpu_hashlib_sha3_messages_per_s']),
          'python mirror queries/s', round(res['cpu_python_mirror_queries_per_s']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--proofs', type=int, default=1 << 18)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'state_proofs.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_state_proofs: no GPU (a measurement needs one)')
    nat.ensure_init()
    # a stream of its own: the library takes a NULL stream for "its own", so on
    # torch's default stream the tensor work and the library's would not be ordered
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a)


if __name__ == '__main__':
    main()
