"""The device-buffer forms of the Merkle / SHA-256 family (pv_sha256_batch_device,
pv_merkle_root_device, pv_merkle_tree_extend_hashes_device,
pv_merkle_audit_paths_device, pv_merkle_consistency_proofs_device,
pv_merkle_verify_inclusion_device, pv_merkle_verify_consistency_device) for
their results, byte for byte: hashlib, the reference fixtures, LevelTree and the
header's routines built for the host are the references.

Every input is a torch device tensor.  Every output is pre-filled with 0xee and
has one guard row before and one after what the call may write.  Every blob
ends in exactly 16 bytes of 0xff.  Every call runs once with stream = NULL and
once on a stream of the test's own, on which its inputs were produced; the two
must agree."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import _merkle as mk
import _merkle_device as md
import _merkle_proofs as mp
from test_gpu_merkle_proofs import STEPS, cons_items, gpu_consistency, gpu_inclusion, incl_items

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
EE = 0xee
CUTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope='module')
def nat():
    from plenum_gpu import _native
    _native.ensure_init(1)
    return _native


@pytest.fixture(scope='module')
def lib(nat):
    return nat.load()


@pytest.fixture(scope='module')
def fx():
    return mp.fixture()


@pytest.fixture(scope='module')
def leaves():
    return mk.fixture()['leaves']


@pytest.fixture(scope='module')
def tree(leaves):
    return mp.LevelTree([mp.leaf(d) for d in leaves])


@pytest.fixture(scope='module')
def host():
    return mp.host_lib()


# ---------------------------------------------------------------- plumbing
class Null:
    """stream = NULL: the library's own stream, which does not wait for torch's"""

    def sp(self):
        torch.cuda.synchronize()
        return ctypes.c_void_p(0)


class Own:
    """a stream of the test's: the inputs are produced on it and the call is given it"""

    def __init__(self):
        self.stream = torch.cuda.Stream(DEV)

    def sp(self):
        from plenum_gpu.device import _stream
        p = _stream(DEV)
        assert p.value == self.stream.cuda_stream
        return p


def both(body):
    """body(ctx) -> anything comparable, under stream = NULL and under a stream of its own"""
    a = body(Null())
    own = Own()
    with torch.cuda.stream(own.stream):
        b = body(own)
    own.stream.synchronize()
    assert a == b, 'stream = NULL and a caller stream disagree'
    return a


def ptr(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: fixtures stay unchanged, and writable


def dev_u64(values):
    return dev(np.array(values, np.uint64).view(np.int64))


def dev_u32(values):
    return dev(np.array(values, np.uint32).view(np.int32))


def dev_dig(items):
    """32-byte values -> (len, 32) bytes on the device; never empty (the device forms want a pointer)"""
    return dev(np.frombuffer(b''.join(items) or bytes(32), np.uint8).reshape(-1, 32))


def dev_blob(blob, k=0):
    """blob at base + k of an aligned allocation -> (tensor, pointer)"""
    raw = torch.full((len(blob) + k,), 0xff, dtype=torch.uint8, device=DEV)
    raw[k:] = dev(blob)
    assert raw.data_ptr() % 16 == 0
    return raw, ptr(raw, k)


class Out:
    """rows x width bytes of 0xee with a guard row on either side"""

    def __init__(self, rows, width):
        self.t = torch.full((rows + 2, width), EE, dtype=torch.uint8, device=DEV)
        self.p = ptr(self.t, width)

    def rows(self):
        return self.t[1:-1]

    def host(self):
        """the rows, after checking that the guards are untouched"""
        h = self.t.cpu().numpy()
        assert (h[0] == EE).all() and (h[-1] == EE).all(), 'a guard row was written'
        return h[1:-1]

    def guards_ok(self):
        return bool((self.t[0] == EE).all() and (self.t[-1] == EE).all())


def words(rows_u8, dtype):
    """(k, 4 or 8) bytes -> k integers"""
    return np.ascontiguousarray(rows_u8).view(dtype).reshape(-1)


def pack_proofs(proofs):
    off = np.zeros(len(proofs) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in proofs])
    return dev_dig([h for p in proofs for h in p]), dev_u64(off)


# ------------------------------------------------- 1. pv_sha256_batch_device
def sha256_dev(lib, msgs, prefix, k, ctx):
    blob, off = md.pack(msgs)
    assert blob[-16:].tobytes() == md.TAIL and int(off[-1]) + 16 == len(blob)
    raw, bp = dev_blob(blob, k)
    off_t = dev_u64(off)
    out = Out(len(msgs), 32)
    rc = lib.pv_sha256_batch_device(bp, ptr(off_t), len(msgs), prefix, out.p, 0, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    return out.host().tobytes()


@pytest.mark.parametrize('prefix', [-1, 0x00, 0x01, 0xff])
def test_sha256_length_misalignment_prefix_grid(lib, prefix):
    msgs, _ = md.sha_grid()
    assert len(msgs) == 568
    want = md.sha_want(msgs, prefix)
    for k in range(4):
        got = both(lambda ctx: sha256_dev(lib, msgs, prefix, k, ctx))
        for i, m in enumerate(msgs):
            assert got[32 * i:32 * i + 32] == want[i], (prefix, k, i, len(m))


def test_sha256_long_message_and_every_padding_shape_before_the_tail(lib):
    batches = [md.long_message()] + md.last_message_batches()
    assert [len(b[-1]) for b in batches] == [4097, 0, 1, 55, 56, 63, 64]
    for batch in batches:
        for prefix in (-1, 0x00, 0x01, 0xff):
            for k in (0, 3):
                got = both(lambda ctx: sha256_dev(lib, batch, prefix, k, ctx))
                assert got == b''.join(md.sha_want(batch, prefix)), (len(batch[-1]), prefix, k)


# -------------------------------------------------- 2. pv_merkle_root_device
def root_dev(lib, data, with_hashes, ctx):
    n = len(data)
    blob, off = md.pack(data)
    raw, bp = dev_blob(blob)
    off_t = dev_u64(off)
    root, lh = Out(1, 32), Out(max(n, 1), 32)          # n = 0: one row that must stay as it is
    rc = lib.pv_merkle_root_device(bp, ptr(off_t), n, lh.p if with_hashes else None, root.p, 0, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    return root.host().tobytes(), lh.host().tobytes()


@pytest.mark.parametrize('n', [0, 1, 2, 3, 255, 256, 257, 511, 513, 1030])
def test_root_of_ragged_leaves_with_and_without_leaf_hashes(lib, leaves, n):
    fxm = mk.fixture()
    roots = {t['size']: bytes.fromhex(t['root']) for t in fxm['trees']}
    data = leaves[:n]
    assert n < 22 or {0, 1, 55, 56, 63, 64, 4097} <= {len(d) for d in data}
    want_root = roots[n] if n in roots else mk.mth_levelwise(data)
    want_lh = [bytes.fromhex(h) for h in fxm['leaf_hashes'][:n]] + [mk.leaf(d) for d in data[70:]]
    assert len(want_lh) == n
    if n == 0:
        assert want_root == hashlib.sha256(b'').digest()
    root, lh = both(lambda ctx: root_dev(lib, data, True, ctx))
    assert root == want_root
    untouched = bytes([EE]) * (32 * max(n, 1))
    assert lh == (b''.join(want_lh) if n else untouched)     # n = 0: leaf_hashes given and left alone
    root, lh = both(lambda ctx: root_dev(lib, data, False, ctx))
    assert root == want_root and lh == untouched


# ---------------------------------- 3. a resident tree through device forms only
def tree_info(lib, h):
    n, depth, root = ctypes.c_uint64(0), ctypes.c_uint32(0), np.zeros(32, np.uint8)
    assert lib.pv_merkle_tree_info(h, ctypes.byref(n), ctypes.byref(depth), ctypes.c_void_p(root.ctypes.data)) == 0
    return n.value, depth.value, root.tobytes()


def grow_tree(lib, leaf_hashes, steps, ctx, states=None):
    """a tree with room for 4 leaves, fed from a device tensor step by step -> handle"""
    lh_t = dev_dig(leaf_hashes)
    h = ctypes.c_int32(0)
    assert lib.pv_merkle_tree_create(4, 0, ctypes.byref(h)) == 0, lib.pv_last_error()
    pos = 0
    for j, k in enumerate(steps):
        rc = lib.pv_merkle_tree_extend_hashes_device(h.value, ptr(lh_t, 32 * pos), k, ctx.sp())
        assert rc == 0, lib.pv_last_error()
        pos += k
        if states is not None:
            n, depth, root = tree_info(lib, h.value)
            assert (n, root.hex()) == (states[j]['tree_size'], states[j]['root']), pos
            assert n == pos and depth == (pos - 1).bit_length()
    return h.value


def test_tree_grown_from_a_device_tensor_keeps_the_fixture_states(lib, tree):
    states = mk.compact_fixture()
    assert [s['extend'] for s in states] == STEPS and sum(STEPS) == 1000

    def body(ctx):
        h = grow_tree(lib, tree.lv[0][:1000], STEPS, ctx, states)
        info = tree_info(lib, h)
        assert lib.pv_merkle_tree_free(h) == 0
        return info
    assert both(body) == (1000, 10, tree.root(1000))


@pytest.fixture(scope='module')
def resident(lib, tree):
    """(handle, depth, leaf hashes on the device) of the 1000-leaf tree"""
    h = grow_tree(lib, tree.lv[0][:1000], STEPS, Null())
    yield h, 10, dev_dig(tree.lv[0][:1000])
    assert lib.pv_merkle_tree_free(h) == 0


@pytest.fixture(scope='module')
def twin(host, tree):
    """the header's generation routines over the same 1000 leaves, on the host"""
    t = host.mc_tree_new(b''.join(tree.lv[0][:1000]), 1000)
    assert host.mc_tree_depth(t) == 10
    out, root = np.zeros((11, 32), np.uint8), np.zeros(32, np.uint8)

    def path(m, s):
        n = host.mc_audit_path(t, m, s, out.ctypes.data, root.ctypes.data)
        return n, out[:min(n, 11)].tobytes(), root.tobytes()

    def proof(a, b):
        n = host.mc_cons_proof(t, a, b, out.ctypes.data)
        return n, out[:min(n, 11)].tobytes()
    yield path, proof
    host.mc_tree_free(t)


def paths_dev(lib, h, depth, reqs, ctx):
    """-> (index, size, nodes, lens, roots): request tensors and guarded outputs"""
    k = len(reqs)
    a, b = dev_u64([r[0] for r in reqs]), dev_u64([r[1] for r in reqs])
    nodes, lens, roots = Out(k, (depth + 1) * 32), Out(k, 4), Out(k, 32)
    rc = lib.pv_merkle_audit_paths_device(h, ptr(a), ptr(b), k, nodes.p, lens.p, roots.p, ctx.sp())
    assert rc == 0, lib.pv_last_error()                # refused requests are no error of the call
    return a, b, nodes, lens, roots


def proofs_dev(lib, h, depth, reqs, ctx):
    k = len(reqs)
    a, b = dev_u64([r[0] for r in reqs]), dev_u64([r[1] for r in reqs])
    nodes, lens = Out(k, (depth + 1) * 32), Out(k, 4)
    rc = lib.pv_merkle_consistency_proofs_device(h, ptr(a), ptr(b), k, nodes.p, lens.p, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    return a, b, nodes, lens


def check_generated(reqs, want, lens, nodes, roots=None):
    """want(a, b) -> (nodes, root or None) of a valid request"""
    lens, nodes = words(lens, np.uint32), nodes.reshape(len(reqs), -1, 32)
    seen = 0
    for i, (a, b, valid) in enumerate(reqs):
        if not valid:
            assert lens[i] == md.REFUSED, (i, a, b)
            assert (nodes[i] == EE).all() and (roots is None or (roots[i] == EE).all()), (i, a, b)
            seen += 1
            continue
        path, root = want(a, b)
        assert lens[i] == len(path), (i, a, b)
        assert nodes[i, :len(path)].tobytes() == b''.join(path), (i, a, b)
        if roots is not None:
            assert roots[i].tobytes() == root, (i, a, b)
    return seen


@pytest.mark.parametrize('phase', [0, 1])
@pytest.mark.parametrize('k', CUTS + (1000,))
def test_paths_and_proofs_with_refused_requests_woven_in(lib, resident, tree, twin, k, phase):
    h, depth, _ = resident
    reqs = md.path_requests(1000, k, phase)
    assert len(reqs) == k

    def body(ctx):
        _, _, nodes, lens, roots = paths_dev(lib, h, depth, reqs, ctx)
        return lens.host().tobytes(), nodes.host().tobytes(), roots.host().tobytes()
    lens, nodes, roots = [np.frombuffer(x, np.uint8) for x in both(body)]
    refused = check_generated(reqs, lambda m, s: (tree.audit_path(m, s), tree.root(s)), lens.reshape(k, 4),
                              nodes, roots.reshape(k, 32))
    assert refused == (k + phase) // 2
    for m, s, valid in reqs:
        if valid:
            assert twin[0](m, s) == (len(tree.audit_path(m, s)), b''.join(tree.audit_path(m, s)), tree.root(s))
    reqs = md.proof_requests(1000, k, phase)

    def body(ctx):
        _, _, nodes, lens = proofs_dev(lib, h, depth, reqs, ctx)
        return lens.host().tobytes(), nodes.host().tobytes()
    lens, nodes = [np.frombuffer(x, np.uint8) for x in both(body)]
    refused = check_generated(reqs, lambda a, b: (tree.consistency_proof(a, b), None), lens.reshape(k, 4), nodes)
    assert refused == (k + phase) // 2
    for a, b, valid in reqs:
        if valid:
            assert twin[1](a, b) == (len(tree.consistency_proof(a, b)), b''.join(tree.consistency_proof(a, b)))


# ------------------------------------------------------ 4. the two verifiers
def incl_dev(lib, items, ctx, root_table=None, leaf_data=None):
    """items as gpu_inclusion of test_gpu_merkle_proofs.py -> [(status, computed, stop)]"""
    n = len(items)
    index, size = dev_u64([it[1] for it in items]), dev_u64([it[2] for it in items])
    nodes, poff = pack_proofs([it[3] for it in items])
    if root_table is None:
        roots, ridx, nr = dev_dig([it[4] for it in items]), None, 0
    else:
        roots, ridx, nr = dev_dig(root_table), dev_u32([it[4] for it in items]), len(root_table)
    lh = blob = loff = None
    bp = None
    if leaf_data is None:
        lh = dev_dig([it[0] for it in items])
    else:
        b, o = md.pack(leaf_data)
        blob, bp = dev_blob(b)
        loff = dev_u64(o)
    status, comp, stop = Out(n, 1), Out(n, 32), Out(n, 8)
    rc = lib.pv_merkle_verify_inclusion_device(ptr(lh) if lh is not None else None, bp,
                                               ptr(loff) if loff is not None else None, ptr(index), ptr(size),
                                               ptr(nodes), ptr(poff), ptr(roots),
                                               ptr(ridx) if ridx is not None else None, nr, n, status.p, comp.p,
                                               stop.p, 0, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    st, cp, sp = status.host().reshape(-1), comp.host(), words(stop.host(), np.uint64)
    return [(int(st[j]), cp[j].tobytes(), int(sp[j])) for j in range(n)]


def cons_dev(lib, items, ctx, tables=None):
    """items: (old, new, old root, new root, proof); with tables = (old table,
    new table or None for the same one) the roots are indices"""
    n = len(items)
    old, new = dev_u64([it[0] for it in items]), dev_u64([it[1] for it in items])
    nodes, poff = pack_proofs([it[4] for it in items])
    if tables is None:
        r0, r1, i0, i1, nr = dev_dig([it[2] for it in items]), dev_dig([it[3] for it in items]), None, None, 0
    else:
        r0 = dev_dig(tables[0])
        r1 = r0 if tables[1] is None else dev_dig(tables[1])
        i0, i1, nr = dev_u32([it[2] for it in items]), dev_u32([it[3] for it in items]), len(tables[0])
    status, c0, c1 = Out(n, 1), Out(n, 32), Out(n, 32)
    rc = lib.pv_merkle_verify_consistency_device(ptr(old), ptr(new), ptr(r0), ptr(r1),
                                                 ptr(i0) if i0 is not None else None,
                                                 ptr(i1) if i1 is not None else None, nr, ptr(nodes), ptr(poff), n,
                                                 status.p, c0.p, c1.p, 0, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    st, a, b = status.host().reshape(-1), c0.host(), c1.host()
    return [(int(st[j]), a[j].tobytes(), b[j].tobytes()) for j in range(n)]


def meets(got, want):
    """fixture expectation: None = not recorded by the reference"""
    return all(w is None or w == g for g, w in zip(got, want))


def test_every_inclusion_row_in_device_buffers(lib, nat, host, fx, tree):
    items, want = incl_items(fx, tree)
    assert len(items) >= 550 and {w[0] for w in want} == {mp.OK, mp.BAD_RANGE, mp.TOO_SHORT, mp.TOO_LONG,
                                                          mp.ROOT_MISMATCH}
    assert any(it[2] >= 2 ** 63 for it in items)
    got = both(lambda ctx: incl_dev(lib, items, ctx))
    status, comp, stop = gpu_inclusion(nat, items)                                 # (a) the host form
    assert got == [(int(status[j]), comp[j].tobytes(), int(stop[j])) for j in range(len(items))]
    assert got == [mp.host_inclusion(host, *it) for it in items]                   # (b) the host twin
    for j, w in enumerate(want):                                                   # (c) the fixture
        assert meets(got[j], w), j
    for n in CUTS:
        pick = [(7 * j) % len(items) for j in range(n)]
        assert both(lambda ctx: incl_dev(lib, [items[j] for j in pick], ctx)) == [got[j] for j in pick], n


def test_every_consistency_row_in_device_buffers(lib, nat, host, fx):
    items, want = cons_items(fx)
    assert {w[0] for w in want} == {mp.OK, mp.BAD_RANGE, mp.TOO_SHORT, mp.ROOT_MISMATCH, mp.INCONSISTENT}
    got = both(lambda ctx: cons_dev(lib, items, ctx))
    status, c0, c1 = gpu_consistency(nat, items)
    assert got == [(int(status[j]), c0[j].tobytes(), c1[j].tobytes()) for j in range(len(items))]
    assert got == [mp.host_consistency(host, *it) for it in items]
    for j, w in enumerate(want):
        assert meets(got[j], w), j
    for n in CUTS:
        pick = [(5 * j) % len(items) for j in range(n)]
        assert both(lambda ctx: cons_dev(lib, [items[j] for j in pick], ctx)) == [got[j] for j in pick], n


def test_inclusion_with_a_root_table(lib, host, tree):
    sizes = [70, 513, 1030]
    table = [tree.root(s) for s in sizes]
    items, plain = [], []
    for j in range(200):
        t = j % 3
        s = sizes[t]
        m = (91 * j) % s
        ridx = t if j % 11 else (t + 1) % 3      # every eleventh proof points at a wrong root
        items.append((tree.lv[0][m], m, s, tree.audit_path(m, s), ridx))
        plain.append(items[-1][:4] + (table[ridx],))
    got = both(lambda ctx: incl_dev(lib, items, ctx, root_table=table))
    assert got == [mp.host_inclusion(host, *it) for it in plain]
    assert [g[0] for g in got] == [mp.OK if j % 11 else mp.ROOT_MISMATCH for j in range(200)]
    assert all(g[1] == tree.root(it[2]) for g, it in zip(got, items))


def test_consistency_with_root_tables(lib, host, tree):
    """old_root_idx / new_root_idx: separate tables, and one table as both;
    a wrong root on either side, and on both: the new root's verdict wins"""
    sizes = [1, 2, 70, 512, 513, 1000, 1030]
    table = [tree.root(s) for s in sizes]
    other = [tree.root(s) for s in sizes[::-1]]      # the old-root table of the two-table run, reversed
    nt = len(sizes)
    pairs = [(a, b) for b in range(nt) for a in range(b)]
    items_one, items_two, plain, kinds = [], [], [], []
    for j in range(210):
        a, b = pairs[j % len(pairs)]
        ia, ib = a, b
        kind = j % 5 if j % 5 < 4 else 0          # 0 right, 1 old wrong, 2 new wrong, 3 both wrong
        if kind in (1, 3):
            ia = (a + 1) % nt
        if kind in (2, 3):
            ib = (b + 1) % nt if (b + 1) % nt != a else (b + 2) % nt
        proof = tree.consistency_proof(sizes[a], sizes[b])
        items_one.append((sizes[a], sizes[b], ia, ib, proof))
        items_two.append((sizes[a], sizes[b], nt - 1 - ia, ib, proof))
        plain.append((sizes[a], sizes[b], table[ia], table[ib], proof))
        kinds.append(kind)
    want = [mp.host_consistency(host, *it) for it in plain]
    assert want == [md.ref_consistency(*it) for it in plain]
    by_kind = {k: {w[0] for w, kk in zip(want, kinds) if kk == k} for k in range(4)}
    # a balanced old tree starts the walk from the given old root, so there a wrong old root
    # surfaces as the new root differing
    assert by_kind[0] == {mp.OK} and by_kind[1] == {mp.INCONSISTENT, mp.ROOT_MISMATCH}
    assert by_kind[2] == {mp.ROOT_MISMATCH} and by_kind[3] == {mp.ROOT_MISMATCH}
    assert both(lambda ctx: cons_dev(lib, items_one, ctx, tables=(table, None))) == want
    assert both(lambda ctx: cons_dev(lib, items_two, ctx, tables=(other, table))) == want


def test_leaf_mode_hashes_a_device_blob(lib, host, tree, leaves):
    by_len = {}
    for i, d in enumerate(leaves):
        by_len.setdefault(len(d), i)
    picks = [by_len[k] for k in (0, 1, 55, 56, 4097)]
    items = [(tree.lv[0][m], m, 1030, tree.audit_path(m, 1030), tree.root(1030)) for m in picks]
    # a row whose leaf data is not the leaf of its index, and one checked against another tree's root
    items.append((tree.lv[0][picks[1]], picks[3], 1030, tree.audit_path(picks[3], 1030), tree.root(1030)))
    items.append((tree.lv[0][picks[4]], picks[4], 1030, tree.audit_path(picks[4], 1030), tree.root(1029)))
    data = [leaves[picks[j]] for j in (0, 1, 2, 3, 4, 1, 4)]
    assert [len(d) for d in data] == [0, 1, 55, 56, 4097, 1, 4097]
    got = both(lambda ctx: incl_dev(lib, items, ctx, leaf_data=data))
    assert got == [mp.host_inclusion(host, *it) for it in items]
    assert [g[0] for g in got] == [mp.OK] * 5 + [mp.ROOT_MISMATCH] * 2


def compact(nodes, lens, sel, depth):
    """(k, depth + 1, 32) generated nodes of the requests `sel` -> (packed nodes, proof_off), on the device"""
    ln = lens.index_select(0, sel).to(torch.int64)
    keep = torch.arange(depth + 1, device=DEV)[None, :] < ln[:, None]
    flat = torch.cat([nodes.index_select(0, sel)[keep], torch.zeros((1, 32), dtype=torch.uint8, device=DEV)])
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(ln, 0)])
    return flat.contiguous(), off.contiguous()


def test_generated_paths_and_proofs_verify_without_leaving_the_device(lib, resident):
    h, depth, lh_t = resident

    def body(ctx):
        reqs = md.path_requests(1000, 1000, 0)
        index, size, nodes, lens, roots = paths_dev(lib, h, depth, reqs, ctx)
        ln = lens.rows().view(torch.int32).flatten()
        sel = torch.nonzero(ln != -1).flatten()
        n = sel.numel()
        assert n == 500
        flat, off = compact(nodes.rows().view(1000, depth + 1, 32), ln, sel, depth)
        idx, sz = index.index_select(0, sel), size.index_select(0, sel)
        leaf, rt = lh_t.index_select(0, idx), roots.rows().index_select(0, sel).contiguous()
        status, comp, stop = Out(n, 1), Out(n, 32), Out(n, 8)
        rc = lib.pv_merkle_verify_inclusion_device(ptr(leaf), None, None, ptr(idx), ptr(sz), ptr(flat), ptr(off),
                                                   ptr(rt), None, 0, n, status.p, comp.p, stop.p, 0, ctx.sp())
        assert rc == 0, lib.pv_last_error()
        assert bool((status.rows() == mp.OK).all()) and torch.equal(comp.rows(), rt)
        assert bool((stop.rows() == 0).all()) and status.guards_ok() and comp.guards_ok() and stop.guards_ok()

        reqs = md.proof_requests(1000, 1000, 0)
        first, second, nodes, lens = proofs_dev(lib, h, depth, reqs, ctx)
        ln = lens.rows().view(torch.int32).flatten()
        sel = torch.nonzero(ln != -1).flatten()
        n = sel.numel()
        assert n == 500
        flat, off = compact(nodes.rows().view(1000, depth + 1, 32), ln, sel, depth)
        a, b = first.index_select(0, sel), second.index_select(0, sel)
        # MTH(0, a) and MTH(0, b) from the tree itself (an empty tree's root is never looked at)
        zero = torch.zeros(n, dtype=torch.int64, device=DEV)
        r = []
        for s in (a, b):
            s1 = torch.clamp(s, min=1)
            rn, rl, rr = Out(n, (depth + 1) * 32), Out(n, 4), Out(n, 32)
            rc = lib.pv_merkle_audit_paths_device(h, ptr(zero), ptr(s1), n, rn.p, rl.p, rr.p, ctx.sp())
            assert rc == 0, lib.pv_last_error()
            r.append(rr.rows().contiguous())
        status, c0, c1 = Out(n, 1), Out(n, 32), Out(n, 32)
        rc = lib.pv_merkle_verify_consistency_device(ptr(a), ptr(b), ptr(r[0]), ptr(r[1]), None, None, 0, ptr(flat),
                                                     ptr(off), n, status.p, c0.p, c1.p, 0, ctx.sp())
        assert rc == 0, lib.pv_last_error()
        assert bool((status.rows() == mp.OK).all()) and torch.equal(c0.rows(), r[0]) and torch.equal(c1.rows(), r[1])
        assert status.guards_ok() and c0.guards_ok() and c1.guards_ok()
        return True
    assert both(body)


# ------------------------------- 5. the second trip of the grid-stride kernels
def second_trip_k():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = cus * 32 * 256            # merkle_blocks() of csrc/pv_api_common.h: 32 blocks of 256 per CU
    k = cap + 2 * 256 + 37
    assert k > cap, 'this test no longer reaches a second trip of the proof kernels'
    return k


@pytest.fixture(scope='module')
def small(lib):
    """(handle, LevelTree) of the 5-leaf tree, depth 3"""
    lh = [bytes.fromhex(x) for x in mk.fixture()['leaf_hashes']]
    t5 = md.small_tree(lh)
    h = grow_tree(lib, t5.lv[0], [md.SMALL], Null())
    assert tree_info(lib, h) == (5, 3, t5.root(5))
    yield h, t5
    assert lib.pv_merkle_tree_free(h) == 0


def first_bad(ok_rows):
    """the first request whose row differs, fetched only if there is one"""
    if bool(ok_rows.all()):
        return None
    return int(torch.nonzero(~ok_rows)[0])


def padded_nodes(proofs, rows):
    """class table of generated nodes: `rows` x 32 bytes per class, 0xee where nothing is written"""
    tab = np.full((len(proofs), rows, 32), EE, np.uint8)
    for c, p in enumerate(proofs):
        for j, hsh in enumerate(p or []):
            tab[c, j] = np.frombuffer(hsh, np.uint8)
    return dev(tab)


def check_generation_trip(k, cls, tab_len, tab_nodes, lens, nodes, tab_root=None, roots=None):
    exp_len = tab_len.index_select(0, cls)
    got_len = lens.rows().view(torch.int32).flatten()
    assert first_bad(got_len == exp_len) is None, 'len_out of request {}'.format(first_bad(got_len == exp_len))
    got = nodes.rows().view(k, 4, 32)
    same = (got == tab_nodes.index_select(0, cls)).all(-1)                     # (k, 4): node j as expected
    keep = torch.arange(4, device=DEV)[None, :] < exp_len[:, None]             # refused (-1): nothing kept
    bad = first_bad((same | ~keep).all(-1))
    assert bad is None, 'nodes of request {}'.format(bad)
    refused = exp_len < 0
    assert bool(refused.any()) and bool((got[refused] == EE).all()), 'a refused request wrote nodes'
    if roots is not None:
        bad = first_bad((roots.rows() == tab_root.index_select(0, cls)).all(-1))
        assert bad is None, 'roots_out of request {}'.format(bad)              # 0xee where refused
        assert roots.guards_ok()
    assert lens.guards_ok() and nodes.guards_ok()


def test_second_trip_of_the_path_kernel(lib, small):
    h, t5 = small
    k = second_trip_k()
    pc = md.path_classes(t5)
    ctx = Null()
    cls = torch.arange(k, device=DEV) % len(pc)
    tab_a, tab_b = dev_u64([c[0] for c in pc]), dev_u64([c[1] for c in pc])
    tab_len = dev(np.array([-1 if c[2] is None else len(c[2]) for c in pc], np.int32))
    tab_nodes = padded_nodes([c[2] for c in pc], 4)
    tab_root = dev(np.stack([np.full(32, EE, np.uint8) if c[3] is None else np.frombuffer(c[3], np.uint8)
                             for c in pc]))
    a, b = tab_a.index_select(0, cls), tab_b.index_select(0, cls)
    nodes, lens, roots = Out(k, 128), Out(k, 4), Out(k, 32)
    rc = lib.pv_merkle_audit_paths_device(h, ptr(a), ptr(b), k, nodes.p, lens.p, roots.p, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    check_generation_trip(k, cls, tab_len, tab_nodes, lens, nodes, tab_root, roots)


def test_second_trip_of_the_consistency_proof_kernel(lib, small):
    h, t5 = small
    k = second_trip_k()
    cc = md.proof_classes(t5)
    own = Own()
    with torch.cuda.stream(own.stream):
        cls = torch.arange(k, device=DEV) % len(cc)
        tab_a, tab_b = dev_u64([c[0] for c in cc]), dev_u64([c[1] for c in cc])
        tab_len = dev(np.array([-1 if c[2] is None else len(c[2]) for c in cc], np.int32))
        tab_nodes = padded_nodes([c[2] for c in cc], 4)
        a, b = tab_a.index_select(0, cls), tab_b.index_select(0, cls)
        nodes, lens = Out(k, 128), Out(k, 4)
        rc = lib.pv_merkle_consistency_proofs_device(h, ptr(a), ptr(b), k, nodes.p, lens.p, own.sp())
        assert rc == 0, lib.pv_last_error()
        check_generation_trip(k, cls, tab_len, tab_nodes, lens, nodes)
    own.stream.synchronize()


def expand_proofs(k, cls, proofs):
    """the proofs of the classes, repeated by cls -> (packed nodes, proof_off), built on the device"""
    tab_nodes = dev_dig([hsh for p in proofs for hsh in p])
    tab_len = dev(np.array([len(p) for p in proofs], np.int64))
    tab_off = torch.cumsum(tab_len, 0) - tab_len
    ln = tab_len.index_select(0, cls)
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(ln, 0)])
    req = torch.repeat_interleave(torch.arange(k, device=DEV), ln)
    src = tab_off.index_select(0, cls.index_select(0, req)) + (torch.arange(req.numel(), device=DEV) -
                                                               off.index_select(0, req))
    return tab_nodes.index_select(0, src).contiguous(), off.contiguous()


def test_second_trip_of_the_inclusion_verifier(lib, small):
    _, t5 = small
    k = second_trip_k()
    ic = md.incl_classes(t5)
    assert {w[0] for _, w in ic} == {mp.OK, mp.ROOT_MISMATCH, mp.TOO_SHORT, mp.TOO_LONG, mp.BAD_RANGE}
    ctx = Null()
    cls = torch.arange(k, device=DEV) % len(ic)
    leaf = dev_dig([it[0] for it, _ in ic]).index_select(0, cls)
    index = dev_u64([it[1] for it, _ in ic]).index_select(0, cls)
    size = dev_u64([it[2] for it, _ in ic]).index_select(0, cls)
    roots = dev_dig([it[4] for it, _ in ic]).index_select(0, cls)
    nodes, off = expand_proofs(k, cls, [it[3] for it, _ in ic])
    status, comp, stop = Out(k, 1), Out(k, 32), Out(k, 8)
    rc = lib.pv_merkle_verify_inclusion_device(ptr(leaf), None, None, ptr(index), ptr(size), ptr(nodes), ptr(off),
                                               ptr(roots), None, 0, k, status.p, comp.p, stop.p, 0, ctx.sp())
    assert rc == 0, lib.pv_last_error()
    want = dev(np.array([w[0] for _, w in ic], np.uint8)).index_select(0, cls)
    bad = first_bad(status.rows().flatten() == want)
    assert bad is None, 'status of proof {}'.format(bad)
    bad = first_bad((comp.rows() == dev_dig([w[1] for _, w in ic]).index_select(0, cls)).all(-1))
    assert bad is None, 'computed of proof {}'.format(bad)
    bad = first_bad(stop.rows().view(torch.int64).flatten() == dev_u64([w[2] for _, w in ic]).index_select(0, cls))
    assert bad is None, 'stop_index of proof {}'.format(bad)
    assert status.guards_ok() and comp.guards_ok() and stop.guards_ok()


def test_second_trip_of_the_consistency_verifier(lib, small):
    _, t5 = small
    k = second_trip_k()
    cc = md.cons_classes(t5)
    assert {w[0] for _, w in cc} == {mp.OK, mp.ROOT_MISMATCH, mp.TOO_SHORT, mp.BAD_RANGE, mp.INCONSISTENT}
    own = Own()
    with torch.cuda.stream(own.stream):
        cls = torch.arange(k, device=DEV) % len(cc)
        old = dev_u64([it[0] for it, _ in cc]).index_select(0, cls)
        new = dev_u64([it[1] for it, _ in cc]).index_select(0, cls)
        r0 = dev_dig([it[2] for it, _ in cc]).index_select(0, cls)
        r1 = dev_dig([it[3] for it, _ in cc]).index_select(0, cls)
        nodes, off = expand_proofs(k, cls, [it[4] for it, _ in cc])
        status, c0, c1 = Out(k, 1), Out(k, 32), Out(k, 32)
        rc = lib.pv_merkle_verify_consistency_device(ptr(old), ptr(new), ptr(r0), ptr(r1), None, None, 0, ptr(nodes),
                                                     ptr(off), k, status.p, c0.p, c1.p, 0, own.sp())
        assert rc == 0, lib.pv_last_error()
        want = dev(np.array([w[0] for _, w in cc], np.uint8)).index_select(0, cls)
        bad = first_bad(status.rows().flatten() == want)
        assert bad is None, 'status of pair {}'.format(bad)
        bad = first_bad((c0.rows() == dev_dig([w[1] for _, w in cc]).index_select(0, cls)).all(-1))
        assert bad is None, 'old_computed of pair {}'.format(bad)
        bad = first_bad((c1.rows() == dev_dig([w[2] for _, w in cc]).index_select(0, cls)).all(-1))
        assert bad is None, 'new_computed of pair {}'.format(bad)
        assert status.guards_ok() and c0.guards_ok() and c1.guards_ok()
    own.stream.synchronize()
