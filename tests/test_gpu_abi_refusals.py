"""What the C ABI refuses, and in which words: (entry point, arguments) ->
(return code, exact pv_last_error() text), through plenum_gpu._native.load().

Every row returns before any launch -- a refusal, or a zero count returning
PV_OK -- so the texts and the order of the checks (which refusal wins when
several apply) are pinned without running a kernel.  Arguments are named as in
include/plenum_verify.h; a row starts from a call whose buffers are all valid
(64-byte device tensors or small host arrays, counts of 1) and overrides what
it is about.  The pv_bls_* entry points keep their own device state and error
channel (pv_bls_last_error) and are not part of this table."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

OK, EINVAL, ENODEV, ENOTINIT = 0, -22, -19, -77
NULL_DEV, NULL_HOST = 'null device buffer', 'null buffer'
ALIGN = 'digest buffers must be 16-byte aligned'
COUNTS = ('n', 'k', 'Q', 'n_batches')
DEFAULTS = {'n': 1, 'k': 1, 'Q': 1, 'N': 1, 'P': 1, 'n_batches': 1, 'n_roots': 1, 'n_nodes': 4, 'quorum': 1,
            'iters': 1, 'prefix': -1}


class Mis:
    """a device pointer 4 bytes past a 16-byte boundary"""


def _declarations():
    """{entry point: [(parameter name, its type)]} from the public header"""
    text = open(os.path.join(REPO, 'include', 'plenum_verify.h')).read()
    text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))
    out = {}
    for name, params in re.findall(r'^(?:int|void|const char \*)\s*\**\s*(pv_\w+)\s*\(([^)]*)\)\s*;', text,
                                   re.M | re.S):
        ps = [re.match(r'(.*?)(\w+)$', ' '.join(p.split())) for p in params.split(',')]
        out[name] = [(m.group(2), m.group(1).strip()) for m in ps if m and m.group(1).strip()]
    return out


PARAMS = {k: v for k, v in _declarations().items() if not k.startswith('pv_bls_')}


def has(name, param):
    return any(p == param for p, _ in PARAMS[name])


@pytest.fixture(scope='module')
def ctx():
    """the library, a few 64-byte device tensors and host arrays, and a resident tree of 3 leaves"""
    import torch
    from plenum_gpu import _native
    assert torch.cuda.is_available()
    _native.ensure_init()

    class Ctx:
        lib = _native.load()
        argtypes = {n: a for n, _, a in _native.SIGNATURES}
        tensors = [torch.zeros(64, dtype=torch.uint8, device='cuda:0') for _ in range(6)]
        dev = [t.data_ptr() for t in tensors]
        host_arrays = [np.zeros(64, np.uint64) for _ in range(6)]
        host = [a.ctypes.data for a in host_arrays]
        tree = 0
    assert all(p % 16 == 0 for p in Ctx.dev)
    h = ctypes.c_int32(0)
    assert Ctx.lib.pv_merkle_tree_create(4, 0, ctypes.byref(h)) == OK, Ctx.lib.pv_last_error()
    leaves = np.arange(96, dtype=np.uint8)
    assert Ctx.lib.pv_merkle_tree_extend_hashes(h.value, leaves.ctypes.data, 3) == OK, Ctx.lib.pv_last_error()
    Ctx.tree = h.value
    yield Ctx
    assert Ctx.lib.pv_merkle_tree_free(Ctx.tree) == OK   # the last test re-creates it after a pv_shutdown


def call(ctx, name, over, all_null=False):
    """name(valid arguments, overridden by `over`) -> (rc, pv_last_error text)"""
    unknown = set(over) - {p for p, _ in PARAMS[name]}
    assert not unknown, (name, unknown)
    device_form = has(name, 'device') or name.endswith('_device')
    bufs = itertools.cycle(ctx.dev if device_form else ctx.host)
    vals = []
    for (p, typ), at in zip(PARAMS[name], ctx.argtypes[name]):
        if p in over:
            v = over[p]
            if v is Mis:
                v = ctx.dev[0] + 4
            elif isinstance(v, np.ndarray):
                v = v.ctypes.data
        elif '*' in typ:   # typed pointers (out-parameters of scalars) default to NULL
            v = next(bufs) if at is ctypes.c_void_p and p != 'stream' and not all_null else None
        elif p == 'handle':
            v = ctx.tree
        else:
            v = DEFAULTS.get(p, 0)
        vals.append(v)
    assert len(vals) == len(ctx.argtypes[name]), name
    rc = getattr(ctx.lib, name)(*vals)
    return rc, ctx.lib.pv_last_error().decode()


def check(ctx, rows, **kw):
    """rows of (entry point, overrides, rc, text); the text of a PV_OK row is not looked at"""
    bad = []
    for name, over, rc, text in rows:
        got = call(ctx, name, over, **kw)
        if got[0] != rc or (rc != OK and got[1] != text):
            bad.append((name, {k: v for k, v in over.items() if not isinstance(v, np.ndarray)}, got, (rc, text)))
    assert not bad, bad


def u64(*v):
    return np.array(v, np.uint64)


def u32(*v):
    return np.array(v, np.uint32)


def test_header_and_binding_agree_on_arity(ctx):
    assert len(PARAMS) >= 60
    for name, ps in PARAMS.items():
        assert len(ps) == len(ctx.argtypes[name]), name


def test_uninitialised_device_is_the_first_refusal(ctx):
    names = [n for n in PARAMS if has(n, 'device')]
    assert len(names) >= 30
    h = ctypes.c_int32(0)
    rows = [(n, dict({'device': 99}, **({'handle': ctypes.byref(h)} if n == 'pv_merkle_tree_create' else {})),
             ENOTINIT, 'device 99 not initialised (call pv_init)') for n in names]
    check(ctx, rows)
    check(ctx, rows, all_null=True)


def test_slot_is_checked_before_counts_and_buffers(ctx):
    names = [n for n in PARAMS if has(n, 'slot')]
    assert len(names) == 6
    text = 'slot must be 0 or 1'
    rows = []
    for n in names:
        first_ptr = next(p for p, typ in PARAMS[n] if '*' in typ)
        rows += [(n, {'slot': 2}, EINVAL, text), (n, {'slot': -1}, EINVAL, text),
                 (n, {'slot': 2, first_ptr: None}, EINVAL, text)]
    check(ctx, rows)
    check(ctx, [(n, {'slot': 2}, EINVAL, text) for n in names], all_null=True)


def test_zero_count_with_null_buffers(ctx):
    """PV_OK, except where another check comes first or the form has no empty case"""
    first = {'pv_merkle_root': NULL_HOST, 'pv_merkle_root_device': NULL_DEV,        # an empty tree has a root
             'pv_synth_layout_device': NULL_DEV, 'pv_synth_fill_device': NULL_DEV, 'pv_synth_device': NULL_DEV,
             'pv_tally_votes_device_async': NULL_DEV}                               # `bad` before n_batches
    names = [n for n in PARAMS if any(p in COUNTS and typ == 'uint64_t' for p, typ in PARAMS[n])]
    assert len(names) >= 40
    rows = []
    for n in names:
        over = {p: 0 for p, typ in PARAMS[n] if p in COUNTS and typ == 'uint64_t'}
        rows.append((n, over, EINVAL if n in first else OK, first.get(n)))
    check(ctx, rows, all_null=True)
    check(ctx, [(n, over, rc, text) for n, over, rc, text in rows if n not in first])   # ... and with buffers
    check(ctx, [('pv_tally_votes_device_async', {'n_batches': 0, 'verdict': None}, OK, None),
                # the node count is looked at before the batch count
                ('pv_tally_votes', {'n_batches': 0, 'n_nodes': 0}, EINVAL, 'n_nodes must be in 1..1024'),
                ('pv_tally_votes_device', {'n_batches': 0, 'n_nodes': 1025}, EINVAL, 'n_nodes must be in 1..1024'),
                ('pv_tally_votes_device_async', {'n_batches': 0, 'n_nodes': 0, 'bad': None}, EINVAL,
                 'n_nodes must be in 1..1024'),
                ('pv_tally', {'n_batches': 0, 'n_nodes': 0}, EINVAL, 'n_nodes must be >= 1'),
                ('pv_tally_device', {'n_batches': 0, 'n_nodes': 0}, EINVAL, 'n_nodes must be >= 1'),
                # keys and signatures of the one-call form
                ('pv_verify_keys_device_async', {'k': 0, 'n': 1}, EINVAL, 'signatures without keys'),
                ('pv_verify_keys_device_async', {'wide': 2}, EINVAL, 'wide must be 0 or 1'),
                ('pv_verify_keys_device_async', {'wide': 2, 'k': 0, 'n': 0}, EINVAL, 'wide must be 0 or 1'),
                ('pv_verify_keys_device_async', {'k': 1, 'n': 0, 'pk': None}, EINVAL, NULL_DEV)])


def test_one_null_buffer(ctx):
    dev = [('pv_verify_batch_device', 'pk'), ('pv_verify_batch_device_async', 'bitmap'),
           ('pv_verify_keyed_device', 'ktab'), ('pv_verify_keyed_device_async', 'bitmap'),
           ('pv_verify_keyed_wide_device', 'key_idx'), ('pv_verify_keyed_wide_device_async', 'bitmap'),
           ('pv_keys_prepare_device', 'ktab'), ('pv_keys_prepare_device_async', 'ktab'),
           ('pv_keys_prepare_wide_device', 'pk'), ('pv_keys_prepare_wide_device_async', 'ktab'),
           ('pv_verify_keys_device_async', 'sig'), ('pv_verify_keys_device_async', 'ktab'),
           ('pv_tally_device', 'reached'), ('pv_tally_votes_device', 'votes'),
           ('pv_tally_votes_device_async', 'bad'), ('pv_tally_votes_device_async', 'sender'),
           ('pv_synth_layout_device', 'off'), ('pv_synth_fill_device', 'blob'), ('pv_synth_device', 'off'),
           ('pv_sha256_batch_device', 'digests'), ('pv_merkle_root_device', 'root'),
           ('pv_merkle_verify_inclusion_device', 'index'), ('pv_merkle_verify_consistency_device', 'status'),
           ('pv_sha3_256_batch_device', 'digests'), ('pv_state_proof_verify_device', 'status'),
           ('pv_state_proof_verify_device', 'node_digests')]
    host = [('pv_verify_batch', 'verdict'), ('pv_tally', 'reached'), ('pv_tally_votes', 'votes'),
            ('pv_sign_batch', 'seeds'), ('pv_sha256_batch', 'digests'), ('pv_merkle_root', 'root'),
            ('pv_merkle_verify_inclusion', 'index'), ('pv_merkle_verify_consistency', 'status'),
            ('pv_merkle_tree_extend', 'off'), ('pv_merkle_tree_extend_hashes', 'leaf_hashes'),
            ('pv_merkle_tree_extend_hashes_device', 'leaf_hashes'),
            ('pv_merkle_audit_paths', 'len_out'), ('pv_merkle_audit_paths_device', 'roots_out'),
            ('pv_merkle_consistency_proofs', 'len_out'), ('pv_merkle_consistency_proofs_device', 'nodes_out'),
            ('pv_sha3_256_batch', 'digests'), ('pv_state_proof_verify', 'status'), ('pv_keycache_add', 'pk'),
            ('pv_rlp_split_list', 'item_beg')]
    count = ctypes.c_uint64(0)
    rows = [(n, {p: None}, EINVAL, NULL_DEV) for n, p in dev] + \
           [(n, dict({p: None}, **({'count': ctypes.byref(count), 'cap': 1} if n == 'pv_rlp_split_list' else {})),
             EINVAL, NULL_HOST) for n, p in host]
    # both leaf modes of the inclusion check: hashes given, or hashed from a blob
    rows += [('pv_merkle_verify_inclusion', {'leaf_hashes': None, 'leaf_off': None}, EINVAL, NULL_HOST),
             ('pv_merkle_verify_inclusion', {'leaf_hashes': None, 'status': None}, EINVAL, NULL_HOST),
             ('pv_merkle_verify_inclusion_device', {'leaf_hashes': None, 'leaf_blob': None}, EINVAL, NULL_DEV),
             ('pv_merkle_verify_inclusion_device', {'leaf_hashes': None, 'leaf_off': None}, EINVAL, NULL_DEV),
             ('pv_merkle_verify_inclusion_device', {'leaf_blob': None, 'leaf_off': None, 'stop_index': None}, EINVAL,
              NULL_DEV),
             ('pv_keycache_size', {}, EINVAL, NULL_HOST), ('pv_rlp_split_list', {}, EINVAL, NULL_HOST),
             ('pv_merkle_tree_create', {}, EINVAL, 'null pointer'),
             ('pv_get_tuning', {'t': None}, EINVAL, 'null pointer'),
             ('pv_set_tuning', {'t': None}, EINVAL, 'null pointer')]
    check(ctx, rows)


def test_alignment_of_device_digest_buffers(ctx):
    sp = 'node_digests must be 16-byte aligned, roots and node_blob 4-byte aligned'
    check(ctx, [('pv_merkle_verify_inclusion_device', {'computed': Mis}, EINVAL, ALIGN),
                ('pv_merkle_verify_inclusion_device', {'leaf_hashes': Mis}, EINVAL, ALIGN),
                ('pv_merkle_verify_inclusion_device', {'n_roots': 0}, EINVAL, 'root_idx without roots'),
                ('pv_merkle_verify_inclusion_device', {'n_roots': 0, 'nodes': Mis}, EINVAL, 'root_idx without roots'),
                ('pv_merkle_verify_consistency_device', {'nodes': Mis}, EINVAL, ALIGN),
                ('pv_merkle_verify_consistency_device', {'new_computed': Mis}, EINVAL, ALIGN),
                ('pv_merkle_verify_consistency_device', {'new_root_idx': None, 'nodes': Mis}, EINVAL,
                 'old_root_idx and new_root_idx go together'),
                ('pv_merkle_verify_consistency_device', {'n_roots': 0}, EINVAL, 'root indices without roots'),
                ('pv_merkle_audit_paths_device', {'nodes_out': Mis}, EINVAL, ALIGN),
                ('pv_merkle_audit_paths_device', {'roots_out': Mis}, EINVAL, ALIGN),
                ('pv_merkle_consistency_proofs_device', {'nodes_out': Mis}, EINVAL, ALIGN),
                ('pv_sha3_256_batch_device', {'digests': Mis}, EINVAL, ALIGN),
                ('pv_sha3_256_batch_device', {'blob': ctx.dev[0] + 2}, EINVAL, 'blob must be 4-byte aligned'),
                ('pv_state_proof_verify_device', {'node_digests': Mis}, EINVAL, sp),
                ('pv_state_proof_verify_device', {'roots': ctx.dev[0] + 2}, EINVAL, sp),
                ('pv_state_proof_verify_device', {'P': 0, 'node_digests': Mis}, EINVAL, 'queries without proofs')])


def test_host_forms_check_ranges_before_any_copy(ctx):
    dec = u64(0, 4, 2)   # decreases at position 1
    at1 = ' not monotone at 1'
    check(ctx, [
        ('pv_sha256_batch', {'off': dec, 'n': 2}, EINVAL, 'off' + at1),
        ('pv_sha256_batch', {'off': dec, 'n': 2, 'prefix': 256}, EINVAL, 'prefix must be -1 (none) or a byte value'),
        ('pv_sha256_batch_device', {'prefix': 256}, EINVAL, 'prefix must be -1 (none) or a byte value'),
        ('pv_sha3_256_batch', {'off': dec, 'n': 2}, EINVAL, 'off' + at1),
        ('pv_merkle_root', {'off': dec, 'n': 2}, EINVAL, 'off' + at1),
        ('pv_merkle_tree_extend', {'off': dec, 'k': 2}, EINVAL, 'off' + at1),
        ('pv_merkle_verify_inclusion', {'proof_off': dec, 'n': 2}, EINVAL, 'proof_off' + at1),
        ('pv_merkle_verify_inclusion', {'proof_off': dec, 'n': 2, 'leaf_hashes': None, 'leaf_off': dec}, EINVAL,
         'proof_off' + at1),
        ('pv_merkle_verify_inclusion', {'leaf_hashes': None, 'leaf_off': dec, 'n': 2}, EINVAL, 'leaf_off' + at1),
        ('pv_merkle_verify_inclusion', {'proof_off': u64(0, 1, 2), 'nodes': None, 'n': 2}, EINVAL, NULL_HOST),
        ('pv_merkle_verify_inclusion', {'root_idx': u32(0, 1), 'n_roots': 1, 'n': 2}, EINVAL,
         'root_idx[1] = 1 is not below n_roots 1'),
        ('pv_merkle_verify_consistency', {'proof_off': dec, 'n': 2}, EINVAL, 'proof_off' + at1),
        ('pv_merkle_verify_consistency', {'proof_off': dec, 'n': 2, 'new_root_idx': None}, EINVAL,
         'old_root_idx and new_root_idx go together'),
        ('pv_merkle_verify_consistency', {'old_root_idx': u32(0, 0), 'new_root_idx': u32(0, 1), 'n': 2}, EINVAL,
         'a root index of pair 1 is not below n_roots 1'),
        ('pv_state_proof_verify', {'key_off': dec, 'Q': 2}, EINVAL, 'key_off' + at1),
        ('pv_state_proof_verify', {'key_off': dec, 'val_off': dec, 'Q': 2}, EINVAL, 'key_off' + at1),
        ('pv_state_proof_verify', {'val_off': dec, 'Q': 2}, EINVAL, 'val_off' + at1),
        ('pv_state_proof_verify', {'val_off': dec, 'Q': 2, 'P': 0}, EINVAL, 'queries without proofs'),
        ('pv_state_proof_verify', {'key_off': u64(0, 3), 'key_blob': None}, EINVAL, NULL_HOST),
        ('pv_state_proof_verify', {'node_end': u64(5), 'node_blob_len': 4}, EINVAL, 'node 0 lies outside the blob'),
        ('pv_state_proof_verify', {'proof_first': dec, 'P': 2}, EINVAL, 'proof_first' + at1),
        ('pv_state_proof_verify', {}, EINVAL, 'proof_first ends at 0, not at N = 1'),
        ('pv_state_proof_verify', {'proof_first': u64(0, 1), 'proof_idx': u32(0, 1), 'Q': 2}, EINVAL,
         'proof_idx[1] = 1 is not below P = 1'),
        ('pv_tally_votes', {'batch_off': dec, 'n_batches': 2}, EINVAL, 'batch_off not monotone'),
        ('pv_tally_votes', {'batch_off': u64(0, 1, 2), 'sender': u32(0, 7), 'n_batches': 2}, EINVAL,
         'sender[1] = 7 is >= n_nodes (4)'),
        ('pv_verify_batch', {'flags': 2}, EINVAL, 'unknown flags 0x2'),
        ('pv_verify_batch', {'flags': 2, 'pk': None}, EINVAL, 'unknown flags 0x2'),
        ('pv_verify_batch', {'msg_off': u64(4, 4, 2), 'n': 2}, EINVAL, 'msg_off not monotone'),
        ('pv_verify_batch', {'device_mask': 1 << 31}, ENODEV, 'device_mask 0x80000000 selects no initialised device'),
    ])


def test_resident_tree_requests_and_handles(ctx):
    check(ctx, [
        ('pv_merkle_audit_paths', {'index': u64(0, 3), 'tree_size': u64(3, 3), 'k': 2}, EINVAL,
         'request 1: (3, 3) outside a tree of 3 leaves'),
        ('pv_merkle_audit_paths', {'index': u64(0), 'tree_size': u64(0)}, EINVAL,
         'request 0: (0, 0) outside a tree of 3 leaves'),
        ('pv_merkle_consistency_proofs', {'first': u64(1, 2), 'second': u64(3, 4), 'k': 2}, EINVAL,
         'request 1: (2, 4) outside a tree of 3 leaves'),
        ('pv_merkle_consistency_proofs', {'first': u64(3), 'second': u64(2)}, EINVAL,
         'request 0: (3, 2) outside a tree of 3 leaves'),
        ('pv_merkle_tree_extend_hashes', {'k': (1 << 40) + 1}, EINVAL, 'tree limited to 2^40 leaves'),
        ('pv_merkle_tree_extend', {'k': 1 << 40}, EINVAL, 'tree limited to 2^40 leaves'),
        ('pv_merkle_tree_create', {'handle': ctypes.byref(ctypes.c_int32(0)), 'capacity_hint': (1 << 40) + 1},
         EINVAL, 'capacity_hint above 2^40 leaves'),
    ])
    bad = [('pv_merkle_tree_info', 12345), ('pv_merkle_tree_free', 12345), ('pv_merkle_tree_extend', 0),
           ('pv_merkle_tree_extend_hashes', -1), ('pv_merkle_tree_extend_hashes_device', 12345),
           ('pv_merkle_audit_paths', 0), ('pv_merkle_audit_paths_device', 12345),
           ('pv_merkle_consistency_proofs', 12345), ('pv_merkle_consistency_proofs_device', 0)]
    rows = [(n, {'handle': h}, EINVAL, 'no Merkle tree with handle {}'.format(h)) for n, h in bad]
    check(ctx, rows)
    check(ctx, rows, all_null=True)   # ... before the count and the buffers are looked at


def test_tuning_rlp_and_timing(ctx):
    from plenum_gpu import _native
    size = ctypes.sizeof(_native.Tuning)
    short = _native.Tuning(struct_size=size - 4)
    text = 'struct_size {} != sizeof(pv_tuning) {}'.format(size - 4, size)
    count = ctypes.c_uint64(0)
    beg, end = u64(0, 0, 0, 0), u64(0, 0, 0, 0)
    string = np.frombuffer(b'\x83dog', np.uint8)   # an RLP string, not a list
    check(ctx, [('pv_get_tuning', {'t': ctypes.addressof(short)}, EINVAL, text),
                ('pv_set_tuning', {'t': ctypes.addressof(short)}, EINVAL, text),
                ('pv_rlp_split_list', {'rlp': string, 'len': 4, 'item_beg': beg, 'item_end': end, 'cap': 4,
                                       'count': ctypes.byref(count)}, EINVAL,
                 'not one RLP list of at most 4 items ending at its end'),
                ('pv_rlp_split_list', {'rlp': None, 'len': 4, 'count': ctypes.byref(count)}, EINVAL, NULL_HOST),
                ('pv_time_verify_device', {'iters': 0}, EINVAL, 'iters must be > 0'),
                ('pv_time_verify_device', {'iters': -3, 'pk': None}, EINVAL, 'iters must be > 0'),
                ('pv_time_verify_keyed_device', {'iters': 0}, EINVAL, 'iters must be > 0'),
                ('pv_synth_layout_device', {'mode': 3}, EINVAL, 'unknown synth mode 3'),
                ('pv_synth_layout_device', {'mode': 1, 'mlen_min': 9, 'mlen_max': 8}, EINVAL, 'mlen_max < mlen_min'),
                ('pv_synth_layout_device', {'mode': 2, 'n_nodes': 0}, EINVAL, 'n_nodes must be in 1..1024'),
                ('pv_synth_fill_device', {'mode': 3}, EINVAL, 'unknown synth mode 3'),
                ('pv_synth_fill_device', {'mode': 2, 'n_nodes': 1025}, EINVAL, 'n_nodes must be in 1..1024'),
                ('pv_keycache_add', {'k': 0xffffffff}, EINVAL, 'key cache limited to 2^32 - 2 keys')])


def test_freed_handles_are_refused_and_reused(ctx):
    """Trees and stores created interleaved: a freed id is refused in the pinned words while its
    neighbours keep their contents, the next create of that kind gets the freed id back (the
    lowest free slot) with an empty object, and pv_shutdown + pv_init leaves no id behind."""
    import hashlib
    from plenum_gpu import _native
    lib = ctx.lib
    empty = hashlib.sha256(b'').digest()
    leaves = np.arange(64, dtype=np.uint8)
    node = np.frombuffer(b'\xc6\x85hello', np.uint8)

    def tree_info(h):
        n, depth, root = ctypes.c_uint64(77), ctypes.c_uint32(77), np.zeros(32, np.uint8)
        rc = lib.pv_merkle_tree_info(h, ctypes.byref(n), ctypes.byref(depth), root.ctypes.data)
        return (rc, lib.pv_last_error().decode()) if rc else (n.value, depth.value, root.tobytes())

    def store_info(s):
        v = [ctypes.c_uint64(77) for _ in range(4)]
        rc = lib.pv_state_store_info(s, *[ctypes.byref(x) for x in v])
        return (rc, lib.pv_last_error().decode()) if rc else tuple(x.value for x in v[:3])

    def create():
        h, s = ctypes.c_int32(0), ctypes.c_int32(0)
        assert lib.pv_merkle_tree_create(1, 0, ctypes.byref(h)) == OK, lib.pv_last_error()
        assert lib.pv_state_store_create(1, 1, 0, ctypes.byref(s)) == OK, lib.pv_last_error()
        return h.value, s.value

    def no_tree(h):
        return EINVAL, 'no Merkle tree with handle {}'.format(h)

    def no_store(s):
        return EINVAL, 'no state store with id {}'.format(s)

    try:
        (t1, s1), (t2, s2), (t3, s3) = create(), create(), create()
        assert t1 < t2 < t3 and s1 < s2 < s3
        assert lib.pv_merkle_tree_extend_hashes(t2, leaves.ctypes.data, 2) == OK, lib.pv_last_error()
        added = ctypes.c_uint64(0)
        assert lib.pv_state_store_add(s2, node.ctypes.data, u64(0, node.size).ctypes.data, 1, None,
                                      ctypes.byref(added)) == OK, lib.pv_last_error()
        assert tree_info(t2) == (2, 1, hashlib.sha256(b'\x01' + leaves.tobytes()).digest())
        assert added.value == 1 and store_info(s2) == (1, 1, node.size)
        assert lib.pv_merkle_tree_free(t2) == OK and lib.pv_state_store_free(s2) == OK
        assert tree_info(t2) == no_tree(t2) and store_info(s2) == no_store(s2)
        for t, s in ((t1, s1), (t3, s3)):
            assert tree_info(t) == (0, 0, empty) and store_info(s) == (0, 0, 0)
        assert tree_info(ctx.tree)[:2] == (3, 2)
        assert create() == (t2, s2)
        assert tree_info(t2) == (0, 0, empty) and store_info(s2) == (0, 0, 0)
        _native.shutdown()
        _native.ensure_init()
        for t, s in ((t1, s1), (t2, s2), (t3, s3)):
            assert tree_info(t) == no_tree(t) and store_info(s) == no_store(s)
        assert tree_info(ctx.tree) == no_tree(ctx.tree)
    finally:   # the module's tree, for whatever runs after this test
        _native.ensure_init()
        h = ctypes.c_int32(0)
        assert lib.pv_merkle_tree_create(4, 0, ctypes.byref(h)) == OK, lib.pv_last_error()
        assert lib.pv_merkle_tree_extend_hashes(h.value, np.arange(96, dtype=np.uint8).ctypes.data, 3) == OK
        ctx.tree = h.value
