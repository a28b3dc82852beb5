"""plenum_gpu — MI355X batch Ed25519 verification and quorum tally for
Plenum's request-authentication hot path.

Host-side mirror of the reference interfaces on this path (same class names,
arguments, return values and exceptions), each with a batch entry point that
runs on HIP kernels through the C-ABI library libplenum_verify.so:

  nacl_wrappers   VerifyKey / SigningKey / Signer / Verifier (+ verify_batch)
                  stp_core/crypto/nacl_wrappers.py
  verifier        Verifier / DidVerifier (+ verify_batch)       plenum/common/verifier.py
  client_authn    ClientAuthNr / NaclAuthNr / SimpleAuthNr / CoreAuthMixin /
                  CoreAuthNr (+ verify_batch, authenticate_batch)
                  plenum/server/client_authn.py
  req_authenticator  ReqAuthenticator (+ verify_batch)       plenum/server/req_authenticator.py
  quorums, models Quorums / Commits / Prepares (+ tally_batches)
                  plenum/server/quorums.py, plenum/server/models.py
  merkle          GpuTreeHasher, sha256_batch, merkle_root      ledger/tree_hasher.py
  merkle_proofs   GpuMerkleVerifier (+ *_batch), GpuMerkleTree
                  ledger/merkle_verifier.py, ledger/compact_merkle_tree.py
  ledger_tree     GpuLedgerTree: the ledger's write cycle on the resident tree
                  (appendTxns / commitTxns / discardTxns, hash store, catch-up)
                  plenum/common/ledger.py, ledger/compact_merkle_tree.py
  state_proofs    GpuStateVerifier (+ verify_state_proofs_batch), sha3_256_batch
                  state/pruning_state.py, state/trie/pruning_trie.py
  state_store     GpuStateStore: a device-resident trie node store,
                  generate_state_proof (+ generate_state_proofs_batch), build_state,
                  state_root_batch, get_batch (reads)
                  state/pruning_state.py, state/trie/pruning_trie.py
  pruning_state   GpuPruningState: the State interface over the store (set / remove /
                  headHash / commit / revertToHead / get)           state/pruning_state.py
  serialization, base58, exceptions, constants   the data formats either side

device.py holds the device-resident (torch tensor) entry points; _native.py is
the ctypes binding.  Nothing here verifies on the CPU.
"""
__version__ = '0.1.0'

# exported from merkle_proofs, imported on first use (the package import stays light)
_MERKLE_PROOFS = ('GpuMerkleVerifier', 'GpuMerkleTree', 'STH')
_LEDGER_TREE = ('GpuLedgerTree',)
_STATE_PROOFS = ('GpuStateVerifier', 'verify_state_proofs_batch', 'sha3_256_batch')
_STATE_STORE = ('GpuStateStore', 'state_root_batch')
_PRUNING_STATE = ('GpuPruningState',)
__all__ = list(_MERKLE_PROOFS + _LEDGER_TREE + _STATE_PROOFS + _STATE_STORE + _PRUNING_STATE)


def __getattr__(name):
    if name in _MERKLE_PROOFS:
        from . import merkle_proofs
        return getattr(merkle_proofs, name)
    if name in _LEDGER_TREE:
        from . import ledger_tree
        return getattr(ledger_tree, name)
    if name in _STATE_PROOFS:
        from . import state_proofs
        return getattr(state_proofs, name)
    if name in _STATE_STORE:
        from . import state_store
        return getattr(state_store, name)
    if name in _PRUNING_STATE:
        from . import pruning_state
        return getattr(pruning_state, name)
    raise AttributeError('module {!r} has no attribute {!r}'.format(__name__, name))
