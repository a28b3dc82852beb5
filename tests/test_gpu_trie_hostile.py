"""The hostile-node table (tests/_trie_hostile.py) through the device entry points of the five state
walks -- pv_state_proof_verify, prove, pv_state_update, pv_state_apply and reachable / prune -- on
stores of the row's two nodes: every output equals the host twin's.  Each row is bytes the kernels
bound-check and answer with a status."""
import re

import numpy as np
import pytest

import _state_prune as pr
import _state_proofs as sp
import _trie_hostile as th

pytestmark = pytest.mark.gpu

ROWS = {r.name: r for r in th.ROWS}


@pytest.fixture(scope='module')
def mod():
    import torch
    from plenum_gpu import _native, state_store
    assert torch.cuda.is_available()
    _native.ensure_init()
    return state_store


def test_verify_every_row_in_one_call(mod):
    """one proof per row, the queries of the host test: statuses equal the host build's"""
    from plenum_gpu import _native as nat
    blob, beg, end, first, roots, pidx, keys, vals = b'', [], [], [0], [], [], [], []
    for p, row in enumerate(th.ROWS):
        for n in row.nodes:
            beg.append(len(blob))
            blob += n
            end.append(len(blob))
        first.append(len(beg))
        roots.append(row.root)
        proved = [th.prove_twin(row)[0].value(q) for q in range(len(th.PROVE_KEYS))]
        for _, key, val in th.verify_queries(row, proved):
            pidx.append(p)
            keys.append(key)
            vals.append(val)
    pk = object.__new__(sp.Packed)
    pk.blob_len, pk.blob = len(blob), np.frombuffer(blob + b'\0' * 16, np.uint8).copy()
    pk.beg, pk.end, pk.first = np.array(beg, np.uint64), np.array(end, np.uint64), np.array(first, np.uint64)
    pk.roots, pk.pidx = np.frombuffer(b''.join(roots), np.uint8).copy(), np.array(pidx, np.uint32)
    (pk.keys, pk.koff), (pk.vals, pk.voff) = sp._pack(keys), sp._pack(vals)
    pk.N, pk.P, pk.Q = len(beg), len(roots), len(pidx)
    want = sp.host_statuses(pk)
    got = np.full(pk.Q, 0xee, np.uint8)
    rc = nat.load().pv_state_proof_verify(sp.ptr(pk.blob), pk.blob_len, sp.ptr(pk.beg), sp.ptr(pk.end),
                                          sp.ptr(pk.first), sp.ptr(pk.roots), sp.ptr(pk.pidx), sp.ptr(pk.keys),
                                          sp.ptr(pk.koff), sp.ptr(pk.vals), sp.ptr(pk.voff), pk.N, pk.P, pk.Q,
                                          sp.ptr(got))
    assert rc == 0, nat.load().pv_last_error()
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert {th.OK, th.VALUE_MISMATCH, th.NODE_MISSING, th.MALFORMED} <= set(got.tolist())


def _merge_gpu(mod, store_id, row, batch, entry):
    """-> (PV_SP_* status, new root or None, emitted nodes' bytes) of one device update / apply, nothing inserted"""
    from plenum_gpu import _native as nat
    try:
        r = mod._update_gpu(store_id, row.root, batch, insert=False, want_nodes=True, entry=entry)
    except nat.PlenumGpuError as e:
        return int(re.search(r'\(status (\d)\)', str(e)).group(1)), None, b''
    return th.OK, r[0], r[3].tobytes()


@pytest.mark.parametrize('name', list(ROWS))
def test_store_walks_equal_the_host_twins(mod, name):
    row = ROWS[name]
    with mod.GpuStateStore(node_hint=1) as st:
        assert st.add_nodes(row.nodes) == 2
        batches, roots, ridx, keys, _ = th.prove_scenario(row)
        want = th.prove_twin(row)[0]
        assert want.same(st.prove(roots, ridx, keys), ids=False) is None
        for batch in th.UPDATE_BATCHES:
            b = th.update_twin(row, batch)
            assert _merge_gpu(mod, st._id, row, batch, 'pv_state_update') == th.built_status(b) + (b.blob.tobytes(),)
        for batch in th.UPDATE_BATCHES + th.REMOVAL_BATCHES:
            b = th.apply_twin(row, batch)
            assert _merge_gpu(mod, st._id, row, batch, 'pv_state_apply') == th.built_status(b) + (b.blob.tobytes(),)
        assert st.info()['n_nodes'] == 2                     # nothing was inserted
        with pr.HostStore(row.nodes) as hs:
            for gpu, host in ((st.reachable([row.root], want_digests=True), hs.prune([row.root], apply=False)),
                              (st.prune([row.root], want_digests=True), hs.prune([row.root]))):
                assert host['rc'] == pr.PR_OK
                for k in ('n_kept', 'bytes_kept', 'n_missing', 'root_status', 'digests'):
                    assert gpu[k] == host[k], k
            assert st.info() == hs.info()
        assert want.same(st.prove(roots, ridx, keys), ids=False) is None     # the pruned store answers as before
