"""GpuPruningState: the reference's State interface (state/pruning_state.py) over a resident trie
node store, a drop-in where a node constructs PruningState.

The store (plenum_gpu.state_store.GpuStateStore) offers the kernels' view: roots in, roots out.  The
reference's users hold a PruningState instead: `set` / `remove` per request, `headHash` after a 3PC
batch, `commit(rootHash)` when the batch is ordered, `revertToHead` when it is not, and
`get(key, isCommitted)` throughout.  This class keeps that bookkeeping -- the head, the committed
head, the chain of uncommitted heads and the read-your-own-uncommitted-writes rule -- so that no
integrator has to write it again.

* `set` / `remove` stage into an ordered pending map, the last occurrence of a key winning; nothing
  runs on the device.  `headHash` flushes the map through ONE `apply_batch` at the current head and
  appends the new head to the chain of uncommitted heads (the reference updates its trie per call).
* `get(key, isCommitted=False)` looks in the pending map first (a staged set gives its value, a
  staged removal None) and reads the rest at the current head; a committed read goes to
  committedHeadHash.  `get_batch` does the same for many keys with one device call.
* `commit` takes the reference's argument forms (:87-98) and does not move the head: committing
  batch 1 while batches 2 and 3 are uncommitted is the normal case.
* `revertToHead(headHash)` drops the pending map, moves the head and truncates the chain.
* `prune(extra_roots)` keeps the committed head, the head, the chain and the extras
  (GpuStateStore.prune): what the reference does with reference counts.

Differences from the reference, all deliberate:
  - an empty value raises ValueError in `set` (as apply_batch does; the reference would store
    rlp([b'']), which reads back as b'');
  - `revertToHead` to a root the store does not hold raises KeyError and changes nothing (the
    reference raises the KeyError from inside replace_root_hash, after it has touched the old root);
  - `as_dict`, `get_all_leaves_for_root_hash` and `generate_state_proof_for_keys_with_prefix` raise
    NotImplementedError: subtree traversal stays out of scope (the prefix-proof pull request was not
    merged; see the scope list of plenum_gpu/state_store.py);
  - a proof lists its nodes terminal node first, root last (state_store.py).

The store is duck-typed: anything with apply_batch(root, items), get_batch(items, decode),
generate_state_proof(key, root, serialize, get_value) and prune(keep_roots).  The CPU tests drive
this class over the Python mirrors (apply_host / get_host) that way.
"""
import hashlib
import string
from binascii import unhexlify

from .state_proofs import BLANK_NODE, BLANK_ROOT, GpuStateVerifier

_TRAVERSAL = ('{} is a subtree traversal, which this state does not offer: whole-state and prefix reads '
              'were left out of the resident store (plenum_gpu/state_store.py, "Out of scope")')


def _bytes(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def _is_hex(val):
    """state/util/utils.py:104-117"""
    if isinstance(val, (bytes, bytearray)):
        try:
            val = bytes(val).decode()
        except ValueError:
            return False
    return isinstance(val, str) and all(c in string.hexdigits for c in val)


class GpuPruningState:
    def __init__(self, store=None, device=0, root=BLANK_ROOT):
        """store: a GpuStateStore (or anything with its four methods; None: a new store on `device`,
        closed by close()); root: the committed head to start from, which the store must hold"""
        self._own = store is None
        if store is None:
            from .state_store import GpuStateStore
            store = GpuStateStore(device)
        self._store = store
        self._committed = self._root_hash(root)
        self._head = self._committed
        self._chain = []      # heads of the uncommitted batches, oldest first
        self._pending = {}    # key -> raw value, or None for a removal; insertion-ordered

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _root_hash(root):
        from .state_store import root_hash_of
        return root_hash_of(root)

    def _open(self):
        if self._store is None:
            raise ValueError('the state is closed')
        return self._store

    def _holds(self, root):
        """whether the store holds the root node of `root` (a read of the empty key fetches it alone)"""
        if root == BLANK_ROOT:
            return True
        try:
            self._open().get_batch([(root, b'')], decode=False)
        except KeyError:
            return False
        except ValueError:
            pass
        return True

    # ------------------------------------------------------------------ writes
    def set(self, key, value):
        """PruningState.set (:60-61), staged; ValueError for an empty value"""
        value = _bytes(value)
        if not value:
            raise ValueError('an empty value is no value; remove(key) removes a key')
        key = _bytes(key)
        self._pending.pop(key, None)      # the last occurrence wins, and keeps the last position
        self._pending[key] = value

    def remove(self, key):
        """PruningState.remove (:84-85), staged"""
        key = _bytes(key)
        self._pending.pop(key, None)
        self._pending[key] = None

    @property
    def headHash(self):
        """the root after every staged set and removal: one apply_batch at the current head"""
        if self._pending:
            new = self._open().apply_batch(self._head, list(self._pending.items()))
            self._pending = {}
            self._head = new
            self._chain.append(new)
        return self._head

    @property
    def committedHeadHash(self):
        return self._committed

    def commit(self, rootHash=None, rootNode=None):
        """PruningState.commit (:87-98): a decoded root node, a hex str, hex bytes, raw bytes, or
        nothing (headHash, which flushes).  The head stays where it is."""
        if rootNode:
            rootHash = self._root_hash(rootNode)
        elif rootHash and _is_hex(rootHash):
            rootHash = unhexlify(_bytes(rootHash))
        elif rootHash:
            rootHash = bytes(rootHash)
        else:
            rootHash = self.headHash
        self._committed = rootHash
        if rootHash in self._chain:       # the batches up to it are no longer uncommitted
            del self._chain[:self._chain.index(rootHash) + 1]

    def revertToHead(self, headHash=None):
        """PruningState.revertToHead (:100-102): the staged work is dropped and the head moves to
        headHash; KeyError, and nothing changes, for a root the store does not hold"""
        root = self._root_hash(headHash)
        if not self._holds(root):
            raise KeyError('revertToHead: the root {} is not in the store'.format(root.hex()))
        self._pending = {}
        self._head = root
        if root in self._chain:
            del self._chain[self._chain.index(root) + 1:]
        else:
            self._chain = []

    # ------------------------------------------------------------------ reads
    def get_batch(self, keys, isCommitted=True):
        """get() for many keys: the decoded values, None for an absent key; one device call"""
        keys = [_bytes(k) for k in keys]
        if isCommitted:
            return self._open().get_batch([(self._committed, k) for k in keys])
        out, rest = [None] * len(keys), []
        for q, k in enumerate(keys):
            if k in self._pending:
                out[q] = self._pending[k]
            else:
                rest.append(q)
        if rest:
            for q, v in zip(rest, self._open().get_batch([(self._head, keys[q]) for q in rest])):
                out[q] = v
        return out

    def get(self, key, isCommitted=True):
        """PruningState.get (:63-70)"""
        return self.get_batch([key], isCommitted)[0]

    def get_batch_sha256(self, preimages, isCommitted=True):
        """get_batch for keys that are sha256(preimage), as the domain state keys a NYM
        (nym_to_state_key, plenum/server/request_handlers/utils.py:38-39): the preimages are hashed
        on the device (pv_sha256_batch_device) into the key buffer the read walks, as
        apply_batch_sha256 does for writes.  Needs a GpuStateStore."""
        preimages = [_bytes(p) for p in preimages]
        store = self._open()
        if isCommitted or not self._pending:
            return store.get_batch_sha256(self._committed if isCommitted else self._head, preimages)
        out, rest = [None] * len(preimages), []
        for q, p in enumerate(preimages):       # the staged keys are few: matched on the host
            k = hashlib.sha256(p).digest()
            if k in self._pending:
                out[q] = self._pending[k]
            else:
                rest.append(q)
        if rest:
            for q, v in zip(rest, store.get_batch_sha256(self._head, [preimages[q] for q in rest])):
                out[q] = v
        return out

    def get_for_root_hash(self, root_hash, key):
        """PruningState.get_for_root_hash (:72-77); KeyError when the root or a node on the path is
        not in the store"""
        return self._open().get_batch([(self._root_hash(root_hash), _bytes(key))])[0]

    def get_head_by_hash(self, root_hash):
        """the decoded root node; BLANK_NODE for the blank root (:52-59)"""
        root = self._root_hash(root_hash)
        if root == BLANK_ROOT:
            return BLANK_NODE
        return self._open().generate_state_proof(b'', root, serialize=False)[-1]

    @property
    def head(self):
        return self.get_head_by_hash(self.headHash)

    @property
    def committedHead(self):
        return self.get_head_by_hash(self._committed)

    # ------------------------------------------------------------------ proofs
    def generate_state_proof(self, key, root=None, serialize=False, get_value=False):
        """PruningState.generate_state_proof (:105-106); root=None is the head
        (state/trie/pruning_trie.py:1088)"""
        root = self.headHash if root is None else self._root_hash(root)
        return self._open().generate_state_proof(_bytes(key), root, serialize=serialize, get_value=get_value)

    verify_state_proof = staticmethod(GpuStateVerifier.verify_state_proof)
    verify_state_proof_multi = staticmethod(GpuStateVerifier.verify_state_proof_multi)

    def generate_state_proof_for_keys_with_prefix(self, key_prfx, root=None, serialize=False, get_value=False):
        raise NotImplementedError(_TRAVERSAL.format('generate_state_proof_for_keys_with_prefix'))

    def get_all_leaves_for_root_hash(self, root_hash):
        raise NotImplementedError(_TRAVERSAL.format('get_all_leaves_for_root_hash'))

    @property
    def as_dict(self):
        raise NotImplementedError(_TRAVERSAL.format('as_dict'))

    # ------------------------------------------------------------------ housekeeping
    def prune(self, extra_roots=()):
        """drop every node that neither the committed head, the head, an uncommitted head nor one of
        `extra_roots` reaches (GpuStateStore.prune) -> its dict"""
        keep = list(dict.fromkeys([self._committed, self._head] + self._chain +
                                  [self._root_hash(r) for r in extra_roots]))
        return self._open().prune(keep)

    @property
    def uncommittedHeads(self):
        """the heads of the uncommitted batches, oldest first"""
        return list(self._chain)

    @property
    def isEmpty(self):
        return self._committed == BLANK_ROOT

    @property
    def closed(self):
        return self._store is None

    def close(self):
        store, self._store = self._store, None
        if store is not None and self._own:
            store.close()
