/*
 * plenum_verify.h — C ABI of the MI355X batch signature-verification and
 * vote-tally engine (libplenum_verify.so).
 *
 * Drop-in boundary for Plenum's request-authentication hot path.  Each entry
 * point names the reference interface it replaces:
 *
 *   pv_verify_batch  replaces N calls of libnacl.crypto_sign_open(sig||msg, pk)
 *                    made by stp_core/crypto/nacl_wrappers.py:86-108
 *                    (VerifyKey.verify) via Verifier.verify (:232-242) and
 *                    plenum/common/verifier.py:53-54 (DidVerifier.verify).
 *                    Native side of that call: libsodium 1.0.18
 *                    int crypto_sign_open(unsigned char *m, unsigned long long *mlen_p,
 *                                         const unsigned char *sm, unsigned long long smlen,
 *                                         const unsigned char *pk);
 *                    (/opt/conda/include/sodium/crypto_sign.h:67).  Verdicts are
 *                    bit-exact with crypto_sign_ed25519_verify_detached on
 *                    (sig[0:64], msg).  The sig||msg framing (smlen < 64 rejects,
 *                    a non-64-byte decoded signature shifts bytes into M) is the
 *                    caller's job, exactly as in the reference;
 *                    the Python glue (plenum_gpu.nacl_wrappers) does it.
 *   pv_tally         replaces the per-3PC-batch voter-set count of
 *                    plenum/server/models.py:16-114 (Commits/Prepares.addVote +
 *                    hasQuorum) with quorum values from plenum/server/quorums.py:15-39:
 *                    the SURVEY.md §8(b) contract (node-indexed voter bitmaps);
 *   pv_tally_votes   the same predicate built from per-message verdicts and sender
 *                    indices (the voter set is formed on the GPU; also the PROPAGATE
 *                    f+1 count of plenum/server/propagator.py:38-46).
 *   pv_sign_batch    batch counterpart of SigningKey(seed) + sign
 *                    (stp_core/crypto/nacl_wrappers.py:130-176; crypto_sign_seed_keypair
 *                    + crypto_sign_detached).  Used to generate fixtures/bench data.
 *
 * Conventions:
 *   - All host buffers are owned by the caller; nothing is retained after return.
 *   - Return 0 on success, a negative errno-style code on failure; no exceptions
 *     cross the ABI.  pv_last_error() describes the last failure (thread-local).
 *   - Calls are synchronous and thread-compatible (one caller thread at a time per
 *     device set), matching the single Looper thread (stp_core/loop/looper.py:64).
 *   - A verdict is a pure function of (pk, sig64, M).
 *   - msg_off has n+1 entries; message i is msg_blob[msg_off[i] : msg_off[i+1]].
 *
 * Device-pointer variants (*_device) take device pointers on `device` and an
 * optional hipStream_t (NULL = a library-owned stream) and return after the
 * work is enqueued AND complete (they synchronise the stream).  The message
 * blob passed to a device variant must have >= 16 readable bytes after the last
 * message (the hash kernel reads aligned words).
 */
#ifndef PLENUM_VERIFY_H
#define PLENUM_VERIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PV_OK 0
#define PV_EINVAL (-22)   /* bad argument */
#define PV_ENODEV (-19)   /* no usable GPU in device_mask */
#define PV_ENOMEM (-12)   /* device allocation failed */
#define PV_EIO (-5)       /* HIP runtime / kernel failure */
#define PV_ENOTINIT (-77) /* pv_init not called */

/* flags for pv_verify_batch */
#define PV_FLAG_NONE 0u
/* Deduplicate verifying keys on the host and prepare each distinct key once
 * (decompressed -A and its cached multiples) when at least half of a shard's
 * signatures repeat a key (node COMMIT votes, many requests per client DID).
 * Verdicts are identical; only the work changes. */
#define PV_FLAG_DEDUP_KEYS 1u

/* words per prepared key (pv_keys_prepare_device): an 8-way comb of -A —
 * affine multiples k * 2^(32 q) * (-A), k = 0..8, q = 0..7, 32 words each —
 * + status word + padding to a multiple of 32 words (each key starts on a
 * 128-byte line, so no 128-byte entry straddles two cache lines) */
#define PV_KEY_WORDS 2336u

/* Initialise the engine on the GPUs in device_mask (bit d = HIP device d;
 * 0 = all visible devices).  Idempotent.  Builds the base-point tables
 * (radix 256, 132 KB; radix 2^16 chunk tables k * 2^(32 q) * B, 33.5 MB per
 * device). */
int pv_init(uint32_t device_mask);

/* Release every device resource.  Safe to call when not initialised. */
void pv_shutdown(void);

/* TEST ONLY (not part of the node-facing interface): pv_init(0) with k (2..8)
 * engine devices that all run on HIP device 0, so the multi-device paths of
 * pv_verify_batch (a worker thread per device, shard offsets, error
 * aggregation) run on a one-GPU box (tests/test_gpu_multidev.py).  Requires
 * that no device is initialised (PV_EINVAL otherwise); pv_shutdown ends it. */
int pv_test_init_dup(uint32_t k);

/* TEST ONLY: the spin budget (ns, default 20,000,000) a zero-copy small call
 * polls its completion word for before it falls back to hipStreamSynchronize;
 * 0 sends every such call through the fallback (tests/test_gpu_keycache.py).
 * PV_EINVAL for ns < 0. */
int pv_test_set_spin_ns(int64_t ns);

/* Human-readable description of the last error on this thread ("" if none). */
const char *pv_last_error(void);

/* Number of devices the engine is using (after pv_init), else 0. */
int pv_device_count(void);

/* Verify n signatures held in HOST memory.
 *   pk      n x 32 bytes
 *   sig     n x 64 bytes (R || S; the first 64 bytes of sig||msg)
 *   msg_blob, msg_off  messages (see conventions)
 *   verdict n bytes out, 1 = valid, 0 = invalid
 * The batch is split into contiguous shards over the devices in device_mask
 * (0 = every initialised device), each driven by its own host thread; a shard
 * runs as a pipeline of about 8 chunks: host threads gather chunk c into a
 * page-locked slot, its H2D runs on a copy stream, and its kernels run on one
 * of two compute streams (chunk c+1's grid fills chunk c's tail).  msg_off must
 * be non-decreasing (checked chunk by chunk before any kernel reads it:
 * PV_EINVAL).  Synchronous: returns after every verdict is in `verdict`. */
int pv_verify_batch(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off,
                    uint64_t n, uint8_t *verdict, uint32_t device_mask, uint32_t flags);

/* Same with DEVICE pointers on `device`.  msg_off entries are offsets into
 * msg_blob.  bitmap (may be NULL) receives ceil(n/64) 64-bit words: bit i%64 of
 * word i/64 = verdict i (the layout all-gathered across ranks). */
int pv_verify_batch_device(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off,
                           uint64_t n, uint8_t *verdict, uint64_t *bitmap, int device, void *stream);

/* Enqueue-only forms for pipelined device callers: the work is queued on
 * `stream` (NULL = the library stream of `slot`) with verify workspace `slot`
 * (0 or 1) and the call returns without waiting; the caller synchronises its
 * stream.  Two batches in flight at once must use different slots and
 * different output buffers (verdict, bitmap; for keys, ktab); work reusing a
 * slot must be ordered after that slot's previous batch (same stream, or an
 * event).  Inputs must be ready on `stream` (the caller orders its own writes).
 * A caller alternating two streams and two slots over consecutive batches lets
 * batch k + 1's hash stage run while batch k's curve grid drains.  bitmap is
 * required here. */
int pv_verify_batch_device_async(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob,
                                 const uint64_t *msg_off, uint64_t n, uint8_t *verdict, uint64_t *bitmap, int device,
                                 void *stream, int slot);
int pv_verify_keyed_device_async(const uint32_t *ktab, const uint32_t *key_idx, const uint8_t *pk, const uint8_t *sig,
                                 const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n, uint8_t *verdict,
                                 uint64_t *bitmap, int device, void *stream, int slot);
int pv_keys_prepare_device_async(const uint8_t *pk, uint64_t k, uint32_t *ktab, int device, void *stream, int slot);

/* Verifying-key cache on the device.  pv_keys_prepare_device fills ktab
 * (k x PV_KEY_WORDS words) for the k 32-byte keys in pk; a key that libsodium
 * would refuse (non-canonical, small order, not on the curve) is marked so and
 * every signature under it is rejected.  The table is an 8-way comb, so a
 * keyed verification needs 28 doublings instead of 253.  pv_verify_keyed_device verifies n
 * signatures whose key is pk[key_idx[i]] (the same pk array the table was built
 * from: the hash still covers the key's bytes) — same verdicts as
 * pv_verify_batch_device on the gathered keys, without re-decompressing a key
 * per signature.  Replaces the per-call VerifyKey(key) construction of
 * stp_core/crypto/nacl_wrappers.py:71-81 for repeated keys. */
int pv_keys_prepare_device(const uint8_t *pk, uint64_t k, uint32_t *ktab, int device, void *stream);

int pv_verify_keyed_device(const uint32_t *ktab, const uint32_t *key_idx, const uint8_t *pk, const uint8_t *sig,
                           const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n, uint8_t *verdict,
                           uint64_t *bitmap, int device, void *stream);

/* Persistent verifying-key cache of host-buffer calls.  pv_keycache_add
 * prepares the comb tables of the k 32-byte keys in pk on every initialised
 * device (and on devices initialised later) and keeps them until
 * pv_keycache_clear / pv_shutdown; keys already cached are skipped.  A
 * pv_verify_batch shard of a Looper-pass size (<= the latency size) then looks
 * up every signature's key on the host: signatures under cached keys run the
 * keyed latency kernel (no decompression of A; the hashed key bytes are still
 * the caller's), the rest the generic one, in the same call.  Verdicts are
 * identical with or without the cache -- a key libsodium refuses is cached as
 * refused.  Fill it from the keys a node already knows: node keys, the client
 * DIDs of SimpleAuthNr.addIdr / getVerkey's NYM state lookups
 * (plenum/server/client_authn.py:145-168), replacing the per-call VerifyKey(key) of
 * stp_core/crypto/nacl_wrappers.py:71-81.  At most 2^32 - 2 keys. */
int pv_keycache_add(const uint8_t *pk, uint64_t k);
int pv_keycache_clear(void);
int pv_keycache_size(uint64_t *count);

/* Wide prepared keys (node keys): the same comb with radix-256 windows --
 * affine multiples k * 2^(32 q) * (-A), k = 0..128, q = 0..7 (129 entries of
 * 32 words per table) + status + padding, PV_KEY_WORDS_WIDE words (132 KB) per
 * key.  A verify then needs 24 doublings and 32 key adds instead of 28 and 64;
 * the preparation costs ~16x the default format's, so it pays for keys that
 * sign many messages per preparation (a pool's node keys, C3).  Same verdicts.
 * Preparation runs 128 lanes per key (16 slices of each of the 8 tables) and
 * holds 160 KB of device scratch per key while it runs (128 lanes x 320 words,
 * owned by the device context, grown to the largest k seen).  Async forms as
 * pv_*_device_async (slot 0 or 1, enqueue only). */
#define PV_KEY_WORDS_WIDE 33056u
int pv_keys_prepare_wide_device(const uint8_t *pk, uint64_t k, uint32_t *ktab, int device, void *stream);
int pv_keys_prepare_wide_device_async(const uint8_t *pk, uint64_t k, uint32_t *ktab, int device, void *stream,
                                      int slot);
int pv_verify_keyed_wide_device(const uint32_t *ktab, const uint32_t *key_idx, const uint8_t *pk, const uint8_t *sig,
                                const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n, uint8_t *verdict,
                                uint64_t *bitmap, int device, void *stream);
int pv_verify_keyed_wide_device_async(const uint32_t *ktab, const uint32_t *key_idx, const uint8_t *pk,
                                      const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n,
                                      uint8_t *verdict, uint64_t *bitmap, int device, void *stream, int slot);

/* Key preparation + keyed verification of one batch in one enqueue-only call
 * (slot / stream rules as pv_*_device_async): the k keys in pk are prepared
 * into ktab (wide = 0: the PV_KEY_WORDS format, 1: PV_KEY_WORDS_WIDE).  A key
 * grid of less than one wave per SIMD (e.g. a pool's 25 node keys in the wide
 * format) runs on the slot's own side stream, forked from `stream`, WHILE the
 * signatures' SHA-512 stage runs on `stream` (it reads only the key bytes
 * pk[key_idx[i]]), and the keyed curve kernel waits for both; a larger key
 * grid fills the GPU itself and runs before the hash stage on `stream`.  Same
 * verdicts and tables as
 * pv_keys_prepare[_wide]_device_async followed by
 * pv_verify_keyed[_wide]_device_async on the same stream, which run the two
 * stages one after the other.  n = 0 only prepares the keys.  As for every
 * keyed call, each key_idx[i] must be < k: the kernels do not bound-check it. */
int pv_verify_keys_device_async(const uint8_t *pk, uint64_t k, uint32_t *ktab, const uint32_t *key_idx,
                                const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n,
                                uint8_t *verdict, uint64_t *bitmap, uint32_t wide, int device, void *stream, int slot);

/* SHA-256 / Merkle tree hashing.
 *   pv_sha256_batch[_device]  digests[i] (32 bytes) = SHA-256(prefix || M_i); prefix -1 = none,
 *                             0..255 = that single byte.  Replaces the per-request
 *                             sha256(...).hexdigest() of Request.key / payload_digest
 *                             (plenum/common/request.py:82-90).
 *   pv_merkle_root[_device]   RFC 6962 Merkle Tree Hash of the leaves M_0..M_{n-1}, bit-identical
 *                             to ledger/tree_hasher.py TreeHasher.hash_full_tree (:55-86; leaf =
 *                             SHA-256(0x00 || M), node = SHA-256(0x01 || l || r), n = 0 ->
 *                             SHA-256("")); leaf_hashes (n x 32, may be NULL) receives the leaf
 *                             digests (TreeHasher.hash_leaf, :21-24).
 * Device variants: root is a 32-byte DEVICE buffer; the blob needs >= 16 readable bytes after
 * the last message. */
int pv_sha256_batch(const uint8_t *blob, const uint64_t *off, uint64_t n, int32_t prefix, uint8_t *digests);
int pv_sha256_batch_device(const uint8_t *blob, const uint64_t *off, uint64_t n, int32_t prefix, uint8_t *digests,
                           int device, void *stream);
int pv_merkle_root(const uint8_t *blob, const uint64_t *off, uint64_t n, uint8_t *root, uint8_t *leaf_hashes);
int pv_merkle_root_device(const uint8_t *blob, const uint64_t *off, uint64_t n, uint8_t *leaf_hashes, uint8_t *root,
                          int device, void *stream);

/* Merkle audit paths and consistency proofs, batched (one proof per GPU lane).
 * All digests are 32 bytes; indices and sizes are 64-bit.  Proof nodes of a
 * batch lie in one array `nodes`; proof i is nodes[proof_off[i] .. proof_off[i+1])
 * (proof_off: n + 1 entries, counted in nodes, monotone).
 *
 * Per-proof status (status[i], one byte each): */
#define PV_MP_OK 0
#define PV_MP_BAD_RANGE 1      /* index >= tree_size, or old_size > new_size (the reference's ValueError) */
#define PV_MP_TOO_SHORT 2      /* ProofError: proof too short */
#define PV_MP_TOO_LONG 3       /* ProofError: proof too long (inclusion only) */
#define PV_MP_ROOT_MISMATCH 4  /* ProofError: computed root (consistency: the new root) differs */
#define PV_MP_INCONSISTENT 5   /* ConsistencyError: the old root differs, or equal sizes with different roots */
/* len_out[i] of a request the *_device generation entries refuse */
#define PV_MP_LEN_REFUSED 0xffffffffu

/*   pv_merkle_verify_inclusion[_device]
 *       MerkleVerifier.verify_leaf_hash_inclusion / verify_leaf_inclusion
 *       (ledger/merkle_verifier.py:155-266) for n proofs.  Leaves: leaf_hashes (n x 32), or,
 *       when leaf_hashes is NULL, the leaf data leaf_blob / leaf_off (n + 1 offsets), hashed
 *       on the GPU as SHA-256(0x00 || leaf) first.  Proof i's root is roots[i], or
 *       roots[root_idx[i]] of a table of n_roots roots when root_idx is not NULL.
 *       Out: status[i]; computed[i] = the root the walk reached; stop_index[i] = the node
 *       index a too-short walk stopped at (the reference's message prints it), else 0.
 *   pv_merkle_verify_consistency[_device]
 *       MerkleVerifier.verify_tree_consistency (:47-153) for n (old_size, new_size) pairs,
 *       the same order of decisions: equal sizes compare roots; old_size == 0 passes; "new
 *       root differs" wins over "old root differs"; extra nodes are accepted.  Roots as
 *       above (old_root_idx / new_root_idx both NULL or both given; then old_roots and
 *       new_roots are tables of n_roots entries and may be the same table).
 *       Out: status[i], old_computed[i], new_computed[i] (the given roots when the proof is
 *       not walked).
 * Host forms check proof_off, leaf_off and the root indices (PV_EINVAL).  Device forms take
 * DEVICE buffers, 16-byte aligned digests, each root index < n_roots (not checked), and a
 * leaf blob with >= 16 readable bytes after the last leaf. */
int pv_merkle_verify_inclusion(const uint8_t *leaf_hashes, const uint8_t *leaf_blob, const uint64_t *leaf_off,
                               const uint64_t *index, const uint64_t *tree_size, const uint8_t *nodes,
                               const uint64_t *proof_off, const uint8_t *roots, const uint32_t *root_idx,
                               uint64_t n_roots, uint64_t n, uint8_t *status, uint8_t *computed,
                               uint64_t *stop_index);
int pv_merkle_verify_inclusion_device(const uint8_t *leaf_hashes, const uint8_t *leaf_blob, const uint64_t *leaf_off,
                                      const uint64_t *index, const uint64_t *tree_size, const uint8_t *nodes,
                                      const uint64_t *proof_off, const uint8_t *roots, const uint32_t *root_idx,
                                      uint64_t n_roots, uint64_t n, uint8_t *status, uint8_t *computed,
                                      uint64_t *stop_index, int device, void *stream);
int pv_merkle_verify_consistency(const uint64_t *old_size, const uint64_t *new_size, const uint8_t *old_roots,
                                 const uint8_t *new_roots, const uint32_t *old_root_idx, const uint32_t *new_root_idx,
                                 uint64_t n_roots, const uint8_t *nodes, const uint64_t *proof_off, uint64_t n,
                                 uint8_t *status, uint8_t *old_computed, uint8_t *new_computed);
int pv_merkle_verify_consistency_device(const uint64_t *old_size, const uint64_t *new_size, const uint8_t *old_roots,
                                        const uint8_t *new_roots, const uint32_t *old_root_idx,
                                        const uint32_t *new_root_idx, uint64_t n_roots, const uint8_t *nodes,
                                        const uint64_t *proof_off, uint64_t n, uint8_t *status, uint8_t *old_computed,
                                        uint8_t *new_computed, int device, void *stream);

/* Device-resident Merkle tree with every level kept: the read side of
 * CompactMerkleTree (ledger/compact_merkle_tree.py:197-249) for batches.
 *   pv_merkle_tree_create        an empty tree on `device` (capacity_hint leaves allocated up
 *                                front; capacity doubles on overflow); *handle > 0
 *   pv_merkle_tree_extend        append k leaves (HOST blob / off, hashed as SHA-256(0x00 || leaf));
 *                                CompactMerkleTree.extend / append
 *   pv_merkle_tree_extend_hashes[_device]  append k leaf hashes (k x 32, HOST / DEVICE memory)
 *   pv_merkle_tree_info          *n leaves, *depth levels above them, root = MTH(0, n)
 *                                (CompactMerkleTree.root_hash; SHA-256("") for n = 0)
 *   pv_merkle_tree_free          release it (pv_shutdown releases every tree)
 *   pv_merkle_audit_paths[_device]
 *       CompactMerkleTree.inclusion_proof(index[i], tree_size[i]) and merkle_tree_hash(0,
 *       tree_size[i]) (what Ledger.merkleInfo / auditProof read, ledger/ledger.py:196-217) for k
 *       requests.  Request i's path is nodes_out[i * (depth + 1) * 32 ...], len_out[i] nodes,
 *       bottom-up; roots_out[i] = MTH(0, tree_size[i]).
 *   pv_merkle_consistency_proofs[_device]
 *       CompactMerkleTree.consistency_proof(first[i], second[i]) (seeder_service.py:85,103),
 *       same output layout; empty for first == 0 and first == second.
 * A request with index >= tree_size, tree_size == 0, tree_size > n, first > second or
 * second > n is never clamped: the host forms return PV_EINVAL before any launch; the device
 * forms (request arrays in DEVICE memory) write len_out[i] = PV_MP_LEN_REFUSED and nothing
 * else for it.  A freed or foreign handle is PV_EINVAL. */
int pv_merkle_tree_create(uint64_t capacity_hint, int device, int32_t *handle);
int pv_merkle_tree_extend(int32_t handle, const uint8_t *blob, const uint64_t *off, uint64_t k);
int pv_merkle_tree_extend_hashes(int32_t handle, const uint8_t *leaf_hashes, uint64_t k);
int pv_merkle_tree_extend_hashes_device(int32_t handle, const uint8_t *leaf_hashes, uint64_t k, void *stream);
int pv_merkle_tree_info(int32_t handle, uint64_t *n, uint32_t *depth, uint8_t *root);
int pv_merkle_tree_free(int32_t handle);
int pv_merkle_audit_paths(int32_t handle, const uint64_t *index, const uint64_t *tree_size, uint64_t k,
                          uint8_t *nodes_out, uint32_t *len_out, uint8_t *roots_out);
int pv_merkle_audit_paths_device(int32_t handle, const uint64_t *index, const uint64_t *tree_size, uint64_t k,
                                 uint8_t *nodes_out, uint32_t *len_out, uint8_t *roots_out, void *stream);
int pv_merkle_consistency_proofs(int32_t handle, const uint64_t *first, const uint64_t *second, uint64_t k,
                                 uint8_t *nodes_out, uint32_t *len_out);
int pv_merkle_consistency_proofs_device(int32_t handle, const uint64_t *first, const uint64_t *second, uint64_t k,
                                        uint8_t *nodes_out, uint32_t *len_out, void *stream);

/* The ledger write cycle on the resident tree: with these a ledger needs no host-side
 * CompactMerkleTree.  A tree holds `committed` <= n leaves; leaves [committed, n) are staged.
 * pv_merkle_tree_extend* appends and commits as before and is PV_EINVAL while leaves are staged;
 * pv_merkle_tree_info and the proof calls keep reading all n leaves (the committed view is
 * tree_size <= committed).  Every call is synchronous and ordered on the tree's stream.
 *   pv_merkle_tree_stage / _stage_hashes / _stage_hashes_device
 *       append k staged leaves (HOST blob / off; k x 32 leaf hashes in HOST / DEVICE memory);
 *       root_out (HOST, may be NULL) = MTH(0, n) afterwards: Ledger.appendTxns ->
 *       uncommittedRootHash, treeWithAppliedTxns (plenum/common/ledger.py:38-57, 129-143).
 *       k <= 1024 rebuilds the right edge in one launch of one workgroup.  k == 0 is PV_OK and
 *       writes nothing, root_out included (pv_merkle_tree_discard(handle, 0, root) reads the root).
 *   pv_merkle_tree_commit        committed += count, no device work: Ledger.commitTxns
 *                                (plenum/common/ledger.py:75-100); count > n - committed is PV_EINVAL
 *   pv_merkle_tree_discard       drop the last `count` staged leaves and repair the right edge in
 *                                one launch: Ledger.discardTxns / reset_uncommitted
 *                                (plenum/common/ledger.py:102-148).  root_out (may be NULL) = the
 *                                new root, SHA-256("") for an empty tree.  count > n - committed is
 *                                PV_EINVAL (the reference's LogicError) and changes nothing.
 *   pv_merkle_tree_sizes         *committed and *total (= n)
 *   pv_merkle_tree_frontier      CompactMerkleTree.hashes (ledger/compact_merkle_tree.py:77-79, what
 *                                save / load / __copy__ carry, :47-63) of the prefix of tree_size <= n
 *                                leaves: *count_out = popcount(tree_size) full-subtree roots, largest
 *                                first, in hashes_out (room for 64 x 32 bytes; NULL: the count only)
 *   pv_merkle_tree_hash_store[_device]
 *       what the hash store receives while leaves first + 1 .. last (sequence numbers, last <= n)
 *       are appended one by one (CompactMerkleTree._push_subtree, ledger/compact_merkle_tree.py:
 *       95-136; HashStore.writeLeaf / writeNode): leaf_out = their (last - first) leaf hashes,
 *       node_out = the completed nodes in writeNode order, *n_nodes = (last - popcount(last)) -
 *       (first - popcount(first)) of them.  Leaf e completes ctz(e) nodes, height h = 1 .. ctz(e),
 *       1-based store position (e - 1) - popcount(e - 1) + h (HashStore.getNodePosition(e, h)).
 *       Either output may be NULL.  node_cap < *n_nodes is PV_EINVAL with the need in *n_nodes and
 *       nothing written.  The _device form writes DEVICE buffers (16-byte aligned) on `stream`.
 *   pv_merkle_tree_check_nodes   the same range and order compared with node_hashes (HOST):
 *                                *n_bad = differing nodes, *first_bad = the smallest differing index
 *                                or UINT64_MAX.  The content check that
 *                                Ledger.recoverTreeFromHashStore / CompactMerkleTree.verify_consistency
 *                                (ledger/compact_merkle_tree.py:280-289: counts only) lack. */
int pv_merkle_tree_stage(int32_t handle, const uint8_t *blob, const uint64_t *off, uint64_t k, uint8_t *root_out);
int pv_merkle_tree_stage_hashes(int32_t handle, const uint8_t *leaf_hashes, uint64_t k, uint8_t *root_out);
int pv_merkle_tree_stage_hashes_device(int32_t handle, const uint8_t *leaf_hashes, uint64_t k, uint8_t *root_out,
                                       void *stream);
int pv_merkle_tree_commit(int32_t handle, uint64_t count);
int pv_merkle_tree_discard(int32_t handle, uint64_t count, uint8_t *root_out);
int pv_merkle_tree_sizes(int32_t handle, uint64_t *committed, uint64_t *total);
int pv_merkle_tree_frontier(int32_t handle, uint64_t tree_size, uint8_t *hashes_out, uint32_t *count_out);
int pv_merkle_tree_hash_store(int32_t handle, uint64_t first, uint64_t last, uint8_t *leaf_out, uint8_t *node_out,
                              uint64_t node_cap, uint64_t *n_nodes);
int pv_merkle_tree_hash_store_device(int32_t handle, uint64_t first, uint64_t last, uint8_t *leaf_out,
                                     uint8_t *node_out, uint64_t node_cap, uint64_t *n_nodes, void *stream);
int pv_merkle_tree_check_nodes(int32_t handle, uint64_t first, uint64_t last, const uint8_t *node_hashes,
                               uint64_t *n_bad, uint64_t *first_bad);

/* SHA3-256 and Patricia-trie state proofs, batched: the third check of a read reply
 * (plenum/server/request_handlers/handler_interfaces/read_request_handler.py:39-59).
 *   pv_sha3_256_batch[_device]
 *       digests[i] (32 bytes) = SHA3-256(M_i), M_i = blob[off[i] .. off[i+1]): the trie's
 *       hashlib.sha3_256 (state/util/utils.py:7-8,156-157).
 *   pv_rlp_split_list   (host only, no GPU)
 *       The top-level items of the RLP list rlp[0 .. len), in place: item k is
 *       rlp[item_beg[k] .. item_end[k]) with its own header.  This is how the nodes of a
 *       serialized proof (Trie.serialize_proof = rlp(list of nodes),
 *       state/trie/pruning_trie.py:1164-1170) are found without copying them.  *count = the
 *       number of items.  PV_EINVAL when the input is not one list whose items end exactly at
 *       its end, or when it holds more than cap items.  Lengths decode as in
 *       state/util/fast_rlp.py:47-71 (lenient), every one checked against the enclosing end.
 *   pv_state_proof_verify[_device]
 *       Trie.verify_spv_proof / verify_spv_proof_multi (pruning_trie.py:1100-1162; what
 *       PruningState.verify_state_proof[_multi], state/pruning_state.py:113-128, call after
 *       encode_kv_for_verification) for Q queries over P proofs.  The N nodes of all proofs are
 *       byte ranges node_blob[node_beg[j] .. node_end[j]), each one RLP list; proof p owns nodes
 *       proof_first[p] .. proof_first[p+1] - 1 (P + 1 entries, monotone, the last == N) and is
 *       trusted up to roots[p] (32 bytes).  Query i checks that proof proof_idx[i] ties key i
 *       (key_blob / key_off) to the ENCODED value i (val_blob / val_off; empty = None = absent).
 *       Every node is hashed once (k_sha3_256), however many queries name its proof; then one
 *       lane per query walks the trie.  status[i] is one of PV_SP_*; the reference's verdict is
 *       status[i] == PV_SP_OK (for _multi: all of its queries).
 *       Host form: PV_EINVAL before any launch (status untouched) for non-monotone key_off /
 *       val_off, node_beg[j] > node_end[j] or node_end[j] > node_blob_len, a proof_first that is
 *       not monotone or does not end at N, or proof_idx[i] >= P.  Q == 0 launches nothing.
 *       Device form: DEVICE buffers, not checked; node_blob 4-byte aligned with >= 16 readable
 *       bytes after the last node; roots 4-byte aligned; node_digests (N x 32, 16-byte
 *       aligned) receives the node digests.
 * pv_sha3_256_batch_device: DEVICE buffers; blob 4-byte aligned (checked) with >= 16 readable
 * bytes after the last message (a lane loads whole aligned 16-byte groups); digests 16-byte
 * aligned (checked).
 * Two deliberate differences from the reference: a node that is not well-formed RLP of a trie
 * node (reachable from a trusted root only through a SHA3 preimage) gives PV_SP_MALFORMED by
 * rule, never an out-of-bounds read, whatever exception pyrlp would raise; and splitting a
 * serialized proof is the caller's step, so an undecodable one is the caller's False. */
#define PV_SP_OK 0
#define PV_SP_VALUE_MISMATCH 1 /* the trie holds another value, or none, for the key */
#define PV_SP_NODE_MISSING 2   /* the root or a referenced node is not among the proof's nodes */
#define PV_SP_MALFORMED 3      /* a node on the path is not a well-formed trie node */
int pv_sha3_256_batch(const uint8_t *blob, const uint64_t *off, uint64_t n, uint8_t *digests);
int pv_sha3_256_batch_device(const uint8_t *blob, const uint64_t *off, uint64_t n, uint8_t *digests, int device,
                             void *stream);
int pv_rlp_split_list(const uint8_t *rlp, uint64_t len, uint64_t *item_beg, uint64_t *item_end, uint64_t cap,
                      uint64_t *count);
int pv_state_proof_verify(const uint8_t *node_blob, uint64_t node_blob_len, const uint64_t *node_beg,
                          const uint64_t *node_end, const uint64_t *proof_first, const uint8_t *roots,
                          const uint32_t *proof_idx, const uint8_t *key_blob, const uint64_t *key_off,
                          const uint8_t *val_blob, const uint64_t *val_off, uint64_t N, uint64_t P, uint64_t Q,
                          uint8_t *status);
int pv_state_proof_verify_device(const uint8_t *node_blob, const uint64_t *node_beg, const uint64_t *node_end,
                                 const uint64_t *proof_first, const uint8_t *roots, const uint32_t *proof_idx,
                                 const uint8_t *key_blob, const uint64_t *key_off, const uint8_t *val_blob,
                                 const uint64_t *val_off, uint64_t N, uint64_t P, uint64_t Q, uint8_t *status,
                                 uint8_t *node_digests, int device, void *stream);

/* Resident trie node store: batched state-proof GENERATION, the serving side of the check above.
 * The reference's trie database is content-addressed and append-only -- a node lives under
 * sha3(rlp(node)) and never changes (state/trie/pruning_trie.py:346-353) -- and
 * Trie.generate_state_proof (:1043-1050, :1075-1098; PruningState.generate_state_proof,
 * state/pruning_state.py:105-106) is Trie._get (:376-407) from a root plus a record of every node
 * fetched by hash, with the root appended.  So the store only grows between two
 * pv_state_store_prune calls, and a proof at any committed
 * root, current or historical, is a walk over hash lookups.  One call replaces one
 * generate_state_proof(key, root, serialize=True, get_value=True) per reply of
 * ReadRequestHandler._get_value_from_state
 * (plenum/server/request_handlers/handler_interfaces/read_request_handler.py:33-61).
 *   pv_state_store_create   an empty store on `device` (room for node_hint nodes and byte_hint
 *                           bytes up front; every buffer doubles on overflow); *store_out > 0
 *   pv_state_store_add[_device]
 *       what the host trie's _encode_node (:334-344: _db.inc_refcount(sha3(rlp(node)), rlp(node)))
 *       adds on commit: n_new node RLPs, node i = node_blob[node_off[i] .. node_off[i+1]) (n_new + 1
 *       offsets).  The nodes are appended to the store's blob, hashed in place (k_sha3_256) and
 *       inserted into a digest-keyed hash table.  A node whose digest the store already holds --
 *       from an earlier call or earlier in this one -- is flagged and gets no second table slot;
 *       its bytes stay in the blob as dead bytes.  digests (may be NULL; n_new x 32) receives the
 *       new nodes' SHA3-256; *n_added (may be NULL) the number of nodes new to the store.
 *       Host form: PV_EINVAL before any launch unless node_off is strictly increasing (an empty
 *       node is refused).  Device form: DEVICE buffers, not checked; a node whose range is
 *       empty, reversed or ends past node_off[n_new] is stored as an empty node, which no walk
 *       reads.  At most 2^32 - 2 nodes are accepted (ids are 32-bit; the table stops at 2^31
 *       slots, which a store reaches at 2^30 nodes: PV_ENOMEM).
 *   pv_state_store_info     nodes added, nodes with a table slot (n_nodes - n_unique = duplicates
 *                           kept as dead bytes), bytes, table slots (a power of two >= 2 n_nodes)
 *   pv_state_store_free     release it (pv_shutdown releases every store)
 *   pv_state_store_prove    HOST buffers.  Query q: key q (key_blob / key_off) at root
 *       roots[root_idx[q]] (32 bytes each; root_idx NULL: root q).  Writes, per query,
 *         status      PV_SP_OK: the walk ended; val_len == 0 means the key is proven absent.
 *                     PV_SP_NODE_MISSING: the root or a referenced node is not in the store (the
 *                     reference's KeyError, which the read handler turns into (None, None)).
 *                     PV_SP_MALFORMED.  PV_SP_PATH_TOO_LONG: more hashed nodes than max_nodes;
 *                     node_count is the true count, so the caller can retry.
 *         node_count  hashed nodes fetched (inline nodes are walked in place and are no proof
 *                     nodes, as spv_grabbing, pruning_trie.py:233-243, runs only on db fetches, :351-352)
 *         proof_off   n_queries + 1 offsets into proof_blob; proof q is the serialized proof
 *                     (Trie.serialize_proof, :1164-1170) of an OK query, empty otherwise
 *         val_rel, val_len   the value (rlp([v]) as the trie stores it, what get_value=True
 *                     returns) lies at proof_blob[proof_off[q] + val_rel[q] ..], val_len[q] bytes
 *       With proof_blob == NULL this is the sizing call: everything but the bytes is written.
 *       With proof_cap < proof_off[n_queries]: PV_EINVAL before the pack launch, the text names
 *       both numbers, and proof_off and the per-query outputs are already written.
 *       PV_EINVAL before any launch: key_off not monotone, root_idx[q] >= n_roots, max_nodes == 0.
 *   pv_state_store_walk_device / pv_state_store_pack_device
 *       the two halves with DEVICE buffers, read by the kernels only: the walk writes node_ids
 *       (n_queries x max_nodes; query q's ids at q * max_nodes, root first) and proof_len; the
 *       caller scans proof_len into proof_off (n_queries + 1, proof_off[0] = 0) and the pack
 *       writes proof_blob (proof_off[n_queries] bytes).  A query whose root_idx is >= n_roots
 *       is PV_SP_MALFORMED; a proof whose ids do not add up to proof_off[q+1] - proof_off[q]
 *       bytes is not written.
 * A store's calls are synchronous and ordered on their stream (NULL = the library's).
 * Two deliberate differences from the reference.  Node order: a proof is the list of the nodes in
 * REVERSE walk order, terminal node first, root last; root last is the one ordering property
 * _generate_state_proof has (pf.append(root), and the NOTE at :1102), the rest of the reference's
 * order is Python set order.  Blank root: the proof is the empty list, the one byte 0xc0, which
 * is what verify accepts; the reference would serialize [b''].
 * Out of scope: generate_state_proof_for_keys_with_prefix (a subtree traversal).  (Building a trie
 * from a batch: pv_state_build; sets onto a committed root: pv_state_update; sets and removals:
 * pv_state_apply; dropping the nodes no kept root reaches: pv_state_store_prune.) */
#define PV_SP_PATH_TOO_LONG 4
int pv_state_store_create(uint64_t node_hint, uint64_t byte_hint, int device, int32_t *store_out);
int pv_state_store_add(int32_t store, const uint8_t *node_blob, const uint64_t *node_off, uint64_t n_new,
                       uint8_t *digests, uint64_t *n_added);
int pv_state_store_add_device(int32_t store, const uint8_t *node_blob, const uint64_t *node_off, uint64_t n_new,
                              uint8_t *digests, void *stream);
int pv_state_store_info(int32_t store, uint64_t *n_nodes, uint64_t *n_unique, uint64_t *n_bytes, uint64_t *n_slots);
int pv_state_store_free(int32_t store);
int pv_state_store_prove(int32_t store, const uint8_t *roots, const uint32_t *root_idx, uint64_t n_roots,
                         const uint8_t *key_blob, const uint64_t *key_off, uint64_t n_queries, uint32_t max_nodes,
                         uint8_t *status, uint32_t *node_count, uint64_t *proof_off, uint64_t *val_rel,
                         uint64_t *val_len, uint8_t *proof_blob, uint64_t proof_cap);
int pv_state_store_walk_device(int32_t store, const uint8_t *roots, const uint32_t *root_idx, uint64_t n_roots,
                               const uint8_t *key_blob, const uint64_t *key_off, uint64_t n_queries,
                               uint32_t max_nodes, uint8_t *status, uint32_t *node_count, uint32_t *node_ids,
                               uint64_t *proof_len, uint64_t *val_rel, uint64_t *val_len, void *stream);
int pv_state_store_pack_device(int32_t store, const uint32_t *node_ids, const uint32_t *node_count,
                               uint32_t max_nodes, const uint64_t *proof_off, uint64_t n_queries,
                               uint8_t *proof_blob, void *stream);

/* Reads from the store (csrc/pv_trie_get.h): PruningState.get / get_for_root_hash
 * (state/pruning_state.py:63-77) for a batch of keys at any roots the store holds -- the walk of
 * pv_state_store_prove without the record of the nodes, so that a value of about a hundred bytes
 * leaves the device and not the ~2 KB of proof around it.
 *   pv_state_store_get      HOST buffers.  Query q: key q (key_blob / key_off) at root
 *       roots[root_idx[q]] (32 bytes each; root_idx NULL: root q).  Writes, per query,
 *         status   PV_SP_OK: the walk ended.  PV_SP_NODE_MISSING: the root or a referenced node is
 *                  not in the store (the reference's KeyError).  PV_SP_MALFORMED: a node on the
 *                  path is no trie node or, with decode, the stored value is not of the accepted
 *                  form.  There is no max_nodes and no PV_SP_PATH_TOO_LONG.
 *         found    1: the key has a value; 0: absent, or a status other than PV_SP_OK.  A blank
 *                  root is PV_SP_OK with found = 0 and no lookup.
 *         val_off  n_queries + 1 offsets into val_blob; value q is val_blob[val_off[q] ..
 *                  val_off[q + 1]), empty unless found.  decode = 0: the value as the trie stores
 *                  it, rlp([v]) (what get_value=True of a proof returns).  decode = 1: the payload
 *                  PruningState.get_decoded returns, rlp_decode(value)[0] (:162-163).  found = 1
 *                  with an empty value (a stored rlp([b''])) is a present key, not an absent one.
 *       Accepted by decode: the stored value is one RLP list (short or long header) whose length
 *       is the rest of the value and whose first item is a string (a byte below 0x80, a short
 *       string, a long string); lengths are read leniently (no canonical-form check) and checked
 *       against the value's range before use.  A bare string, an empty list, a first item that is
 *       a list and any length that overruns are PV_SP_MALFORMED with found = 0.
 *       With val_blob == NULL this is the sizing call: everything but the bytes is written.
 *       With val_cap < val_off[n_queries]: PV_EINVAL before the copy launch, the text names both
 *       numbers, and val_off and the per-query outputs are already written.
 *       PV_EINVAL before any launch: key_off not monotone, root_idx[q] >= n_roots, decode not 0 or 1.
 *   pv_state_store_get_device   the same with DEVICE buffers, read by the kernels only (key_off
 *       and root_idx are not checked: a query whose root_idx is >= n_roots is PV_SP_MALFORMED);
 *       val_off is scanned on the device and its last entry read back for the val_cap check.
 *       roots 4-byte aligned.  Synchronous on `stream` (NULL = the library's). */
int pv_state_store_get(int32_t store, const uint8_t *roots, const uint32_t *root_idx, uint64_t n_roots,
                       const uint8_t *key_blob, const uint64_t *key_off, uint64_t n_queries, int32_t decode,
                       uint8_t *status, uint8_t *found, uint64_t *val_off, uint8_t *val_blob, uint64_t val_cap);
int pv_state_store_get_device(int32_t store, const uint8_t *roots, const uint32_t *root_idx, uint64_t n_roots,
                              const uint8_t *key_blob, const uint64_t *key_off, uint64_t n_queries, int32_t decode,
                              uint8_t *status, uint8_t *found, uint64_t *val_off, uint8_t *val_blob,
                              uint64_t val_cap, void *stream);

/* Pruning the store (csrc/pv_trie_prune.h): keep exactly the nodes reachable from the roots the
 * caller names, drop the rest and give the memory back.  It replaces what the reference's pruning
 * state does on commit and revertToHead (state/pruning_state.py:87-102): reference counts on every
 * node (state/db/refcount_db.py), a death row of nodes whose count fell to zero and an epoch ttl
 * after which they are deleted (state/trie/pruning_trie.py:208-230, 681).  The difference from the
 * reference: no counts, no death row and no ttl -- reachability from NAMED roots.  A node calls it
 * with committedHeadHash, the heads of its uncommitted batches and every root it still serves to
 * readers; whatever else the store held (earlier roots, reverted batches, the duplicates
 * pv_state_apply re-emits) is gone afterwards.
 *   keep_roots    HOST memory, n_roots x 32 bytes.
 *   root_status   (may be NULL; n_roots bytes, written in both modes) PV_SP_OK, or
 *                 PV_SP_NODE_MISSING for a non-blank root the store does not hold.  The blank root
 *                 is PV_SP_OK and reaches nothing.
 *   apply == 0    the sizing and reporting call: every output is written, the store is untouched.
 *   apply != 0    the store is compacted.
 *   n_kept, bytes_kept, n_missing, kept_digests   each may be NULL.  n_missing counts the 32-byte
 *                 child references of kept nodes that the store does not hold (a store filled from
 *                 proofs is partial by design; a walk that needs such a node answered
 *                 PV_SP_NODE_MISSING before and still does).  kept_digests has digest_cap entries of
 *                 32 bytes and receives the kept nodes' digests in new-id order.
 * The kept set is the closure of "a node some walk of pv_state_store_prove from a kept root can
 * fetch by hash": the children of a branch's items 0 .. 15 and of an extension's item 1, through
 * inline nodes; a 32-byte leaf value or branch value is never followed, and a node that is no trie
 * node is kept when referenced and contributes no children.  So for every kept root r and key k
 * pv_state_store_prove(r, k) returns the same status, node_count, value and proof bytes as before,
 * and pv_state_apply / pv_state_update onto a kept root return the same root and nodes.
 * After apply != 0: the kept nodes are renumbered in ascending order of their old ids (a stable
 * compaction: the result depends on the store's content and the roots alone); duplicate ids and
 * their dead bytes are gone, n_nodes == n_unique == n_kept and n_bytes == bytes_kept; the table is
 * rebuilt at the smallest power of two >= max(64, 2 n_kept); the node and byte capacities shrink to
 * the next power of two that holds the kept data.  NODE IDS HANDED OUT EARLIER
 * (pv_state_store_walk_device) ARE INVALID.  The new buffers are built beside the old ones and
 * swapped in at the end: a failure leaves the store as it was.  Synchronous and ordered like every
 * other store call.
 * Refusals, each before any change to the store: PV_EINVAL for an unknown store, n_roots == 0 (free
 * the store instead), keep_roots == NULL, kept_digests with digest_cap < n_kept (the text starts
 * "digest capacity too small" and *n_kept holds the need), with apply != 0 any root that is
 * PV_SP_NODE_MISSING (a mistyped root must not empty a store; the text names its index and
 * root_status is written), and inline nodes nested more than 7 deep under a stored node (a
 * well-formed trie nests 3 deep; only junk added with pv_state_store_add goes deeper).
 * PV_ENOTINIT without pv_init; PV_ENOMEM when the fresh buffers cannot be allocated.
 *   pv_state_store_prune (state/pruning_state.py:87-102; pruning_trie.py:681; refcount_db.py) */
int pv_state_store_prune(int32_t store, const uint8_t *keep_roots, uint64_t n_roots, int apply,
                         uint8_t *root_status, uint64_t *n_kept, uint64_t *bytes_kept, uint64_t *n_missing,
                         uint8_t *kept_digests, uint64_t digest_cap);

/* Time the phases of one applied prune (pv_state_store_prune with apply != 0, same refusals, the
 * store is compacted) with HIP events on the store's stream, as pv_time_verify_device times the
 * verify kernels: *ms_mark = the seed kernel and the level loop with its count read-backs,
 * *ms_compact = the keep flags, the two scans, the allocation of the fresh buffers and the copy,
 * *ms_rehash = clearing and refilling the fresh table.  For tools/bench_state_prune.py. */
int pv_time_state_store_prune(int32_t store, const uint8_t *keep_roots, uint64_t n_roots, uint64_t *n_kept,
                              uint64_t *bytes_kept, float *ms_mark, float *ms_compact, float *ms_rehash);

/* Batch construction of a state trie (csrc/pv_trie_build.h): the write side of the store above.
 * The reference computes a state root with one PruningState.set per key and reads headHash
 * (state/pruning_state.py:60-61, 136; Trie.update, state/trie/pruning_trie.py:1006-1027).  A
 * Merkle-Patricia root depends on the final key/value set alone, so any sequence of sets is one
 * batch computation over the sorted distinct keys.
 *   Input    n keys (key_blob / key_off) and n values (val_blob / val_off); a value is the bytes
 *            the trie stores, rlp([v]) from PruningState.set, and is not empty.
 *   Output   root (32 bytes, HOST memory in both forms); *n_nodes and *n_bytes (HOST, may be
 *            NULL): the nodes the reference stores under their hash -- RLP of >= 32 bytes, and the
 *            root node whatever its length (_encode_node(..., is_root=True), :334-344) -- and
 *            their bytes.  Optional, all or some: node_blob (n_bytes), node_off (n_nodes + 1,
 *            node_off[0] = 0), digests (n_nodes x 32).  Node order is fixed by the keys alone
 *            (position i of the sorted keys owns, in this order, the extension above the branch
 *            whose leftmost split is before key i, that branch, and the leaf of key i); two
 *            byte-identical nodes are both emitted.  n == 0, the empty state: PV_OK, root
 *            receives SHA3-256(0x80), *n_nodes and *n_bytes 0, node_off[0] = 0 -- each if it is
 *            given (all may be NULL); no kernel of the build runs, nothing is inserted and the
 *            store and the input buffers are not looked at.
 *   Capacities   blob_cap bytes for node_blob; node_cap nodes for node_off (node_cap + 1 entries)
 *            and digests (node_cap x 32).  A capacity counts only for the outputs it sizes that
 *            are given (the digests alone need no blob_cap).  If one is too small: PV_EINVAL,
 *            the text starts with
 *            "node capacity too small", *n_nodes / *n_bytes hold what is needed, no node is
 *            written and none is inserted, so the caller can retry.
 *   store    -1, or a store on the same device: the nodes are appended and inserted with the
 *            digests the build computed (no second hash).
 *   pv_state_build (state/pruning_state.py:60-61; pruning_trie.py:1006-1027)
 *            HOST buffers, keys in any order; of equal keys the last occurrence wins, as a
 *            sequence of sets gives.  PV_EINVAL before any launch: null pointers with n > 0,
 *            offsets not monotone, an empty value, an unknown store.
 *   pv_state_build_device (state/pruning_state.py:60-61; pruning_trie.py:1006-1027)
 *            DEVICE buffers (node outputs too).  The keys must be strictly increasing bytewise,
 *            a proper prefix first; a pair out of order or equal is refused with a text naming
 *            the first offending index (so are an empty value and decreasing offsets), nothing
 *            is written and nothing is inserted.  key_blob and val_blob are 4-byte aligned with
 *            16 readable bytes after the last item; digests 16-byte aligned.
 * At most 2^28 keys per call, keys of at most 2^20 bytes, values of at most 2^30 bytes.
 * The empty key is a key like any other (the reference accepts it).  Differences from the
 * reference: it also keeps the intermediate nodes of every update, here only the nodes reachable
 * from the final root exist.  Sets onto an existing root: pv_state_update below; sets and
 * removals: pv_state_apply. */
int pv_state_build(const uint8_t *key_blob, const uint64_t *key_off, const uint8_t *val_blob, const uint64_t *val_off,
                   uint64_t n, int32_t store, uint8_t *root, uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob,
                   uint64_t blob_cap, uint64_t *node_off, uint64_t node_cap, uint8_t *digests);
int pv_state_build_device(const uint8_t *key_blob, const uint64_t *key_off, const uint8_t *val_blob,
                          const uint64_t *val_off, uint64_t n, int32_t store, uint8_t *root, uint64_t *n_nodes,
                          uint64_t *n_bytes, uint8_t *node_blob, uint64_t blob_cap, uint64_t *node_off,
                          uint64_t node_cap, uint8_t *digests, int device, void *stream);

/* Sets applied to a committed root (csrc/pv_trie_update.h): the per-3PC-batch update.  The
 * reference takes the state at a committed root, applies one PruningState.set per request of
 * the batch and reads the new headHash (state/pruning_state.py:60-61, 136; Trie.update,
 * state/trie/pruning_trie.py:1006-1027).  Here the batch is one call: one lane per batch key
 * walks the old trie in `store` from old_root and carries, as it is, the reference of every
 * child no batch key enters; the carried values and references and the new values make one
 * sorted list, and the build above runs over it.  No host trie and no other key of the state is
 * needed, and every earlier root stays provable: an update only adds to the store.
 *   Input    store: where the old trie is read.  old_root (32 bytes, HOST memory in both forms).
 *            Keys and values as pv_state_build[_device].
 *   insert   != 0: the emitted nodes are appended to `store` with the digests the build computed.
 *            0: compute only, so a sizing call followed by a retry never inserts twice.
 *   Output   new_root (32 bytes, HOST in both forms), *n_nodes, *n_bytes, node_blob, node_off,
 *            digests and the two capacities as pv_state_build, the "node capacity too small"
 *            refusal included.  The nodes are exactly what the build over the merged list emits,
 *            in its fixed order: every re-encoded node on a touched path, the root last changed
 *            included; nodes inside untouched subtrees are never emitted.  A re-encoded node the
 *            store already holds (an overwrite with the same value) is emitted and flagged a
 *            duplicate by the store.  n == 0: PV_OK, new_root = old_root, sizes 0 and
 *            node_off[0] = 0 -- each if it is given (all may be NULL); no kernel of the update
 *            runs and, as with the empty build, the store is not looked at.
 *            old_root = SHA3-256(0x80), the blank root: the result of pv_state_build, and the
 *            store is not read.
 *   Refusals   PV_EINVAL before any launch: an unknown store, null pointers with n > 0, offsets
 *            not monotone, an empty value, misaligned device blobs; PV_ENOTINIT without pv_init.
 *            The device form refuses unsorted or equal keys, an empty value and decreasing
 *            offsets with pv_state_build_device's texts.  If the walk of a batch key meets a node
 *            that is not in the store (old_root included) or is not a well-formed trie node, the
 *            whole call is refused: PV_EINVAL, the text names the first such key and its PV_SP_*
 *            status, nothing is written and nothing is inserted.  More than 2^28 merged items
 *            (batch keys plus carried values and references, at most 17 per node on a key's
 *            path) are refused.
 *   pv_state_update (state/pruning_state.py:60-61; pruning_trie.py:1006-1027)
 *            HOST buffers, keys in any order, the last of equal keys wins.
 *   pv_state_update_device (state/pruning_state.py:60-61; pruning_trie.py:1006-1027)
 *            DEVICE buffers (node outputs too), keys strictly increasing, on the store's device.
 * Calls are synchronous and ordered on the store's stream (NULL = the library's).  Sets only: an
 * empty value is refused; removals go through pv_state_apply below.  The nodes an update leaves
 * unreachable go with pv_state_store_prune. */
int pv_state_update(int32_t store, const uint8_t *old_root, const uint8_t *key_blob, const uint64_t *key_off,
                    const uint8_t *val_blob, const uint64_t *val_off, uint64_t n, int insert, uint8_t *new_root,
                    uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob, uint64_t blob_cap, uint64_t *node_off,
                    uint64_t node_cap, uint8_t *digests);
int pv_state_update_device(int32_t store, const uint8_t *old_root, const uint8_t *key_blob, const uint64_t *key_off,
                           const uint8_t *val_blob, const uint64_t *val_off, uint64_t n, int insert,
                           uint8_t *new_root, uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob,
                           uint64_t blob_cap, uint64_t *node_off, uint64_t node_cap, uint8_t *digests, void *stream);

/* Sets and removals applied to a committed root: pv_state_update with the third mutating call of
 * the State interface, PruningState.remove (state/pruning_state.py:84-85; Trie.delete,
 * state/trie/pruning_trie.py:683-848).  A pair with an EMPTY value removes its key (no set has an
 * empty value: rlp([v]) has at least one byte); removing a key the state does not hold changes
 * nothing.  The lane of a removed key walks and carries as a set's lane does, emits no value, and
 * opens every child reference it carries from a branch on its path: a leaf child is carried as its
 * path and value, an extension child as its path and child reference, a branch child as it is.  So
 * a branch left with one entry collapses in the build over the merged list: a leaf or extension
 * child merges its path with the slot nibble and any extension above, a branch child goes under a
 * new or lengthened extension, a branch left with only its value becomes a leaf.
 *   Arguments, outputs, capacities, insert, the sizing-call contract, n == 0 and the refusals are
 *   those of pv_state_update[_device], except that an empty value is a removal, not a refusal.
 *   The host form takes val_blob == NULL when no pair of the batch has a value byte.
 *   No item left (every key of the state removed): new_root = SHA3-256(0x80), the blank root, zero
 *   nodes, no build launch.  old_root the blank root: the removals are dropped and the rest is
 *   pv_state_build.  A batch without removals gives the outputs of pv_state_update byte for byte.
 *   Difference from the reference: it decodes the sibling of a removed key only when a collapse
 *   happens; here a removal needs every node referenced from the branches on its path to be in
 *   `store` (PV_EINVAL naming the key and PV_SP_NODE_MISSING otherwise; PV_SP_MALFORMED for a
 *   referenced node that is no trie node).  A store that holds a whole state always has them; a
 *   store filled from proofs alone may refuse a removal the reference would apply.
 *   pv_state_apply (state/pruning_state.py:60-61, 84-85; pruning_trie.py:683-848, 1006-1027)
 *            HOST buffers, keys in any order, the last of equal keys wins: a later removal beats
 *            an earlier set and the other way round.
 *   pv_state_apply_device (state/pruning_state.py:60-61, 84-85; pruning_trie.py:683-848, 1006-1027)
 *            DEVICE buffers (node outputs too), keys strictly increasing, on the store's device.
 * The store grows with every batch; pv_state_store_prune drops the nodes no kept root reaches. */
int pv_state_apply(int32_t store, const uint8_t *old_root, const uint8_t *key_blob, const uint64_t *key_off,
                   const uint8_t *val_blob, const uint64_t *val_off, uint64_t n, int insert, uint8_t *new_root,
                   uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob, uint64_t blob_cap, uint64_t *node_off,
                   uint64_t node_cap, uint8_t *digests);
int pv_state_apply_device(int32_t store, const uint8_t *old_root, const uint8_t *key_blob, const uint64_t *key_off,
                          const uint8_t *val_blob, const uint64_t *val_off, uint64_t n, int insert, uint8_t *new_root,
                          uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob, uint64_t blob_cap,
                          uint64_t *node_off, uint64_t node_cap, uint8_t *digests, void *stream);

/* State keys sorted on the device (csrc/pv_trie_sort.h), for keys that are produced there: the
 * domain-state key of a NYM is sha256(nym) (plenum/server/request_handlers/utils.py:38-39,
 * nym_handler.py:112), which pv_sha256_batch_device writes in request order.
 *   Order: bytewise, a proper prefix first (the order the *_device forms above require).  Of equal
 *   keys the occurrence with the highest index stays: the last of equal keys wins, as in the host
 *   forms.  No input buffer is written and no value byte is read.
 *   Cost: one round of radix passes per 8 bytes that two distinct keys share (1 round for random
 *   32-byte keys).  Keys above 1024 bytes are refused (PV_EINVAL naming the first such key): the
 *   host forms pv_state_build / pv_state_update / pv_state_apply sort keys of any length.
 *   key_blob 4-byte aligned; keys may start at any byte; no byte past a key is read.
 *   pv_state_sort_device
 *            perm     DEVICE, n words out: perm[k] = the index of the k-th kept key, k < *n_kept;
 *                     the rest is not written
 *            n_kept   HOST out: the number of distinct keys
 *            Refused by the first kernel with nothing written: key_off decreasing, a key above
 *            1024 bytes.  n == 0: PV_OK, *n_kept = 0, nothing else is looked at.
 *   pv_state_build_unsorted_device    the arguments of pv_state_build_device
 *   pv_state_apply_unsorted_device    the arguments of pv_state_apply_device
 *            The pairs in any order: the sort, a gather of the kept pairs into compact blobs, then
 *            the code of the sorted form over them.  Every output, the sizing-call contract, insert
 *            and n == 0 are those of the sorted form over the sorted distinct pairs, byte for byte;
 *            in apply a later removal beats an earlier set and the other way round.  A batch
 *            without removals gives pv_state_update_device's outputs.  The refusals before any
 *            launch are the sorted form's; the first kernel refuses decreasing offsets, a key above
 *            1024 bytes and a value that is above 2^30 bytes or (build) empty, naming the input
 *            index, with nothing written and nothing inserted.
 *            PV_EIO "device sort: a bug in the sort ...": the build's own order check refused the
 *            sorted keys.  It is not retried. */
int pv_state_sort_device(const uint8_t *key_blob, const uint64_t *key_off, uint64_t n, uint32_t *perm,
                         uint64_t *n_kept, int device, void *stream);
int pv_state_build_unsorted_device(const uint8_t *key_blob, const uint64_t *key_off, const uint8_t *val_blob,
                                   const uint64_t *val_off, uint64_t n, int32_t store, uint8_t *root,
                                   uint64_t *n_nodes, uint64_t *n_bytes, uint8_t *node_blob, uint64_t blob_cap,
                                   uint64_t *node_off, uint64_t node_cap, uint8_t *digests, int device,
                                   void *stream);
int pv_state_apply_unsorted_device(int32_t store, const uint8_t *old_root, const uint8_t *key_blob,
                                   const uint64_t *key_off, const uint8_t *val_blob, const uint64_t *val_off,
                                   uint64_t n, int insert, uint8_t *new_root, uint64_t *n_nodes, uint64_t *n_bytes,
                                   uint8_t *node_blob, uint64_t blob_cap, uint64_t *node_off, uint64_t node_cap,
                                   uint8_t *digests, void *stream);

/* Measurement only (tools/bench_state_sort.py): the first two steps of the fused forms over DEVICE
 * pairs, the sort and the gather into the compact temporaries, each timed with HIP events on the
 * call's stream; empty values are admitted, nothing is built.  HOST outputs: the kept count, the
 * rounds the sort ran and the two times in milliseconds. */
int pv_time_state_sort_device(const uint8_t *key_blob, const uint64_t *key_off, const uint8_t *val_blob,
                              const uint64_t *val_off, uint64_t n, int device, void *stream, uint64_t *n_kept,
                              uint32_t *rounds, float *ms_sort, float *ms_gather);

/* Per-batch quorum tally, SURVEY.md §8(b) form (HOST memory).
 *   verdict_bits  n_batches x W words, W = ceil(n_nodes / 32): bit j of word w of
 *                 batch b = node 32 w + j cast a valid vote in batch b (a voter SET:
 *                 a node's repeated votes are one bit, plenum/server/models.py:24-28)
 *   dup_mask      same shape, may be NULL: nodes whose votes must not count
 *                 (e.g. a sender the caller already counted elsewhere)
 *   reached       n_batches out: popcount(verdict_bits & ~dup_mask) >= quorum
 * Bits of nodes >= n_nodes are ignored. */
int pv_tally(const uint32_t *verdict_bits, const uint32_t *dup_mask, uint64_t n_batches, uint32_t n_nodes,
             uint32_t quorum, uint8_t *reached);

/* DEVICE buffers; votes (may be NULL) receives the per-batch counts. */
int pv_tally_device(const uint32_t *verdict_bits, const uint32_t *dup_mask, uint64_t n_batches, uint32_t n_nodes,
                    uint32_t quorum, uint8_t *reached, uint32_t *votes, int device, void *stream);

/* Per-batch quorum tally from per-message verdicts (HOST memory).
 *   verdict    n_msgs bytes (1 = vote counts)
 *   sender     n_msgs node indices (< n_nodes <= 1024; an index >= n_nodes is
 *              PV_EINVAL, never a silently dropped vote)
 *   batch_off  n_batches + 1 offsets into verdict/sender
 *   votes      n_batches out: distinct valid senders per batch
 *   reached    n_batches out: votes >= quorum
 * Duplicate senders count once (a voter SET, plenum/server/models.py:24-28). */
int pv_tally_votes(const uint8_t *verdict, const uint32_t *sender, const uint64_t *batch_off, uint64_t n_batches,
                   uint32_t n_nodes, uint32_t quorum, uint32_t *votes, uint8_t *reached);

int pv_tally_votes_device(const uint8_t *verdict, const uint32_t *sender, const uint64_t *batch_off,
                          uint64_t n_batches, uint32_t n_nodes, uint32_t quorum, uint32_t *votes, uint8_t *reached,
                          int device, void *stream);
/* Enqueue-only form for pipelined callers: the kernel ORs 1 into the DEVICE
 * word *bad when a sender index is >= n_nodes (the caller zeroes it and checks
 * it once its stream is synchronised -- such a vote is never counted). */
int pv_tally_votes_device_async(const uint8_t *verdict, const uint32_t *sender, const uint64_t *batch_off,
                                uint64_t n_batches, uint32_t n_nodes, uint32_t quorum, uint32_t *votes,
                                uint8_t *reached, uint32_t *bad, int device, void *stream);

/* Batch keygen + sign (HOST memory): pk_out[i], sig_out[i] for seed i over
 * message i.  Deterministic (RFC 8032 / crypto_sign_detached). */
int pv_sign_batch(const uint8_t *seeds, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n,
                  uint8_t *pk_out, uint8_t *sig_out);

int pv_sign_batch_device(const uint8_t *seeds, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n,
                         uint8_t *pk_out, uint8_t *sig_out, int device, void *stream);

/* Deterministic synthetic workload on the device (bench/tests; spec in
 * plenum_gpu/synth.py).  Two phases so that the caller can
 * size the message blob:
 *   pv_synth_layout_device  off[0..n] <- exclusive prefix sum of the message
 *                           lengths (off[n] = blob bytes)
 *   pv_synth_fill_device    messages, seeds, tamper flags (and for COMMIT the
 *                           sender node of every vote), then keygen + sign, then
 *                           the spec's single-bit tampering.
 * Modes: FIXED (C2: len = mlen_min), RANGE (C4: len uniform in [mlen_min,
 * mlen_max]), COMMIT (C3: signature i is node slot i % n_nodes's COMMIT vote
 * in 3PC batch i / n_nodes; M = "instId:0|op:COMMIT|ppSeqNo:<b+1>|viewNo:0").
 * key_mod (FIXED/RANGE): key index = i % key_mod (0 = distinct keys).
 * Buffers are device buffers the caller allocated: off (n+1), blob (off[n] + 16),
 * seeds (n*32), pk (n*32), sig (n*64), tamper (n), sender (n or NULL). */
#define PV_SYNTH_FIXED 0u
#define PV_SYNTH_RANGE 1u
#define PV_SYNTH_COMMIT 2u

int pv_synth_layout_device(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t mlen_min,
                           uint32_t mlen_max, uint32_t n_nodes, uint64_t *off, int device, void *stream);

int pv_synth_fill_device(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t key_mod,
                         uint32_t n_nodes, const uint64_t *off, uint8_t *blob, uint8_t *seeds, uint8_t *pk,
                         uint8_t *sig, uint8_t *tamper, uint32_t *sender, int device, void *stream);

/* FIXED-mode convenience (C2): layout + fill in one call; blob holds n*mlen + 16. */
int pv_synth_device(uint32_t cfg, uint64_t first, uint64_t n, uint32_t key_mod, uint32_t mlen, uint64_t *off,
                    uint8_t *blob, uint8_t *seeds, uint8_t *pk, uint8_t *sig, uint8_t *tamper, int device,
                    void *stream);

/* Time the verify kernels alone over `iters` launches on device-resident
 * inputs using HIP events on the launch stream; returns per-kernel average
 * milliseconds (hash, curve).  "hash" = k_hash plus, on the half-size path, the
 * scalar stage k_lattice; "curve" = the single curve kernel launch. */
int pv_time_verify_device(const uint8_t *pk, const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off,
                          uint64_t n, uint8_t *verdict, uint64_t *bitmap, int device, void *stream, int iters,
                          float *ms_hash, float *ms_curve);

/* ------------------------------------------------------------------------
 * Schedule tuning.  pv_init reads NO environment: a node runs the defaults
 * below unless its code calls pv_set_tuning.  None of these knobs changes a
 * verdict (tests/test_gpu_verify.py and test_gpu_device.py run the fixtures
 * through every setting); they exist for A/B timing (tools/) and tests.
 *
 *   curve_mode      curve stage of generic (non-keyed) batches:
 *     PV_CURVE_HALF     (default) half-size scalars: Euclid on (8L, h) gives
 *                       c == d h (mod 8L) with |c|, d < 2^131, d odd, and the
 *                       verdict is  s'B + c(-A) + d(-R) == O  (s' = dS mod L): the
 *                       same accept/reject as libsodium's encode(SB - hA) == R for
 *                       every input (derivation in indy-plenum_amd/csrc/pv_lattice.h);
 *                       the ~0.2 % of signatures whose h has no such (c, d) get the
 *                       full-length verdict in the same launch;
 *     PV_CURVE_FULL     every signature through the full-length verdict;
 *     PV_CURVE_GROUPED  the full-length kernel, 8 signatures per lane sharing one
 *                       inversion.
 *   lat_max         generic batches of at most this many signatures (per device
 *                   call / host-buffer shard) run the latency kernel: 8 lanes per
 *                   signature (lane-pair split, each side's point over a lane
 *                   QUAD, one coordinate per lane, DPP exchanges), so small
 *                   batches finish ~2x sooner.  Default 32768 (the measured
 *                   crossover with the throughput path is 32k-64k); 0 disables;
 *                   at most 2^20.
 *   lat_keyed_max   keyed batches (prepared keys, the key cache) of at most this
 *                   many signatures run the keyed latency kernel (the key's comb
 *                   over two lane quads per signature).  Default 8192; 0 disables.
 *   lat_kernel      PV_LAT_QUAD (default) or PV_LAT_PAIR (the lane-pair kernel, A/B).
 *   small_zc_max    host calls of at most this many signatures read their inputs
 *                   from, and write verdicts to, mapped page-locked memory (no
 *                   copies).  Default 2048; 0 = always copy.
 *   host_fused      host-buffer chunks of generic batches: 1 (default) = one
 *                   fused launch per chunk + one lane-quad pass over the deferred
 *                   records; 0 = hash, lattice, curve launches per chunk.
 *   host_staging    PV_STAGING_PINNED (default): each chunk is gathered by up to
 *                   host_copy_threads host threads into one of two page-locked
 *                   slots per device (at most host_pin_max_mb each) and DMA'd from
 *                   there; PV_STAGING_PAGEABLE: the caller's buffers go straight
 *                   to hipMemcpyAsync.  Switching to pageable releases the slots.
 *   host_chunks     a shard runs as leading ramp chunks (host_ramp, 2 host_ramp,
 *                   ... signatures below a regular chunk; host_ramp 0 = one first
 *                   chunk of host_first_pct % of a regular one) and then about
 *                   host_chunks equal chunks of >= 32768 signatures.
 *                   Defaults 8 (1..256), ramp 32768 (0 or 1024..2^20),
 *                   first_pct 50 (10..100), copy threads 8 (1..64), pin 512 MB
 *                   (16..4096).
 *   host_trace      1 = per-chunk host timings of pv_verify_batch on stderr.
 *   bls_quad_max    BLS calls (pv_bls_verify_*) of at most this many checks run
 *                   one check per lane quad (latency), larger ones one per lane
 *                   pair (throughput).  Default 32768 (0..2^20).
 *   bls_oct_max     BLS calls of at most this many checks run one check per lane
 *                   octet (the shortest chain; takes precedence over
 *                   bls_quad_max).  Default 4096 (0..2^20).
 *   reserved        must be 0.
 * (The test-only duplicate engine devices are not a tuning field: see
 * pv_test_init_dup below.)
 * pv_get_tuning fills *t with the current values (struct_size must be set to
 * sizeof(pv_tuning) by the caller); pv_set_tuning validates every field
 * (PV_EINVAL and nothing changes if one is out of range), keeps them for later
 * pv_init calls and applies them to every initialised device.
 * ---------------------------------------------------------------------- */
#define PV_CURVE_HALF 0u
#define PV_CURVE_FULL 1u
#define PV_CURVE_GROUPED 2u
#define PV_LAT_QUAD 0u
#define PV_LAT_PAIR 1u
#define PV_STAGING_PINNED 0u
#define PV_STAGING_PAGEABLE 1u
typedef struct pv_tuning {
  uint32_t struct_size;       /* sizeof(pv_tuning) */
  uint32_t curve_mode;
  uint64_t lat_max;
  uint64_t lat_keyed_max;
  uint64_t small_zc_max;
  uint32_t lat_kernel;
  uint32_t host_fused;
  uint32_t host_staging;
  uint32_t host_chunks;
  uint32_t host_first_pct;
  uint32_t host_copy_threads;
  uint64_t host_ramp;
  uint32_t host_pin_max_mb;
  uint32_t host_trace;
  uint32_t bls_quad_max;
  uint32_t bls_oct_max;
  uint32_t reserved;
} pv_tuning;
int pv_get_tuning(pv_tuning *t);
int pv_set_tuning(const pv_tuning *t);

/* mode (may be NULL) = the curve_mode of `device`; deferred (may be NULL) =
 * signatures of the last generic batch on this device that took the
 * full-length verdict (0 if none ran). */
int pv_curve_stats(int device, uint32_t *mode, uint64_t *deferred);

/* Live kernel timing of the verify calls themselves (bench.py's timed region):
 * enable = 1 resets and starts recording HIP events around the hash and curve
 * stages of every verify launch on `device` (on the launch stream, without
 * waiting for them: async launches stay in flight); enable = 0 stops, waits
 * for the recorded events and returns the summed milliseconds and the number
 * of launches. */
int pv_kernel_timing(int device, int enable, float *hash_ms, float *curve_ms, uint64_t *launches);

/* The SHA-512 part of the live "hash" interval: summed milliseconds from the
 * start of each timed verify launch to the end of its k_hash (the pre-checks +
 * SHA-512(R||A||M), without the half-size path's k_lattice), since the last
 * pv_kernel_timing(device, 1, ...).  bench.py's hash roofline. */
int pv_kernel_timing_sha(int device, float *sha_ms);

/* pv_time_verify_device for keyed batches. */
int pv_time_verify_keyed_device(const uint32_t *ktab, const uint32_t *key_idx, const uint8_t *pk, const uint8_t *sig,
                                const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n, uint8_t *verdict,
                                uint64_t *bitmap, int device, void *stream, int iters, float *ms_hash,
                                float *ms_curve);




/* ------------------------------------------------------------------------
 * BLS COMMIT check
 *
 *   pv_bls_verify_batch  replaces n calls of
 *                        BlsCryptoVerifierIndyCrypto.verify_sig(signature, message, bls_pk)
 *                        (crypto/bls/indy_crypto/bls_crypto_indy_crypto.py:73-82), made by
 *                        BlsBftReplicaPlenum._validate_signature for every COMMIT
 *                        (plenum/bls/bls_bft_replica_plenum.py:55-75, 194-213), i.e.
 *                        python-ursa 0.1.1 Bls.verify(sig, msg, vk, gen):
 *                        e(sigma, g) == e(H(msg), vk) over Milagro AMCL BN254.
 *   pv_bls_set_keys      the fixed G2 arguments of those checks: the group generator
 *                        (BlsGroupParamsLoaderIndyCrypto, bls_crypto_indy_crypto.py:15-20)
 *                        and the nodes' keys (bls_key_register.get_key_by_name);
 *                        replaces IndyCryptoBlsUtils.bls_from_str(v, VerKey) (:38-52)
 *                        + the pairing's G2 precomputation.
 *   pv_bls_sign_batch[_device], pv_bls_pubkeys
 *                        batch counterparts of Bls.sign / VerKey.new (data generation).
 *
 * PARITY UNPINNED: ursa / AMCL are not in the reference and not installed; the
 * reference holds no BLS vector.  Encodings (128-byte representations):
 *   sigma  0x04|x|y (uncompressed) or 0x02/0x03|x (compressed), big-endian, rest
 *          ignored; x or y >= p, another prefix, or a point off y^2 = x^3 + 2 is
 *          the point at infinity O (AMCL ECP::frombytes).  A representation that
 *          is not 128 bytes fails to decode: verdict 0 (sig_len).
 *   keys   x.a|x.b|y.a|y.b, big-endian, each taken mod p (ECP2::frombytes);
 *          off the twist y^2 = x^3 + 2/(1+i) = O.
 *   H(m)   SHA-256(m) as a big-endian integer mod p, try-and-increment on x,
 *          y = (x^3+2)^((p+1)/4) (ursa PointG1::from_hash / AMCL ECP::new_big).
 *   e(O, .) = e(., O) = 1: sigma = O or key = O verify iff both are O.
 * Errors of these entry points are reported by pv_bls_last_error().
 * ---------------------------------------------------------------------- */
#define PV_BLS_KEY_OK 0u          /* a point of order r on the twist */
#define PV_BLS_KEY_INFINITY 1u    /* off the twist: decodes to O */
#define PV_BLS_KEY_NOT_IN_G2 2u   /* on the twist outside the order-r subgroup: verdicts are 0 */

/* Prepare the generator (128 B) and k keys (k x 128 B) on HIP device `device`:
 * decode, subgroup check, the 70 optimal-ate lines of each point (kept on the
 * device; replaces the previous key set).  status (k bytes, may be NULL) gets
 * PV_BLS_KEY_*.  PV_EINVAL if the generator is not PV_BLS_KEY_OK. */
int pv_bls_set_keys(const uint8_t *gen, const uint8_t *pks, uint64_t k, uint8_t *status, int device);

/* Append k keys (k x 128 B) to the key set of pv_bls_set_keys on `device`
 * WITHOUT re-preparing the keys already there: one k_bls_lines launch over the
 * k new points (a node key added by a NODE txn, bls_key_register).  Their key
 * indices are *first .. *first + k - 1 (first may be NULL); status as in
 * pv_bls_set_keys.  PV_ENOTINIT without a set; PV_EINVAL past 65535 keys (the
 * set is left as it was on any error). */
int pv_bls_add_keys(const uint8_t *pks, uint64_t k, uint8_t *status, uint64_t *first, int device);

/* The key set on `device`: keys in it and the points k_bls_lines has prepared
 * for it so far (cumulative over pv_bls_set_keys / pv_bls_add_keys). */
int pv_bls_keyset_info(int device, uint64_t *nkeys, uint64_t *points_prepared);

/* n checks from HOST memory: check j = (sig[j] 128 B, message msg_idx[j] of
 * msg_blob/msg_off (n_msgs messages, msg_off has n_msgs+1 entries), key
 * key_idx[j] of the current key set) -> verdict[j] (1 = Bls.verify true).
 * sig_len (may be NULL): the decoded representation lengths; != 128 -> 0.
 * Every message is hashed once; checks are grouped by key on the device. */
int pv_bls_verify_batch(const uint8_t *sig, const uint64_t *sig_len, const uint8_t *msg_blob, const uint64_t *msg_off,
                        uint64_t n_msgs, const uint32_t *msg_idx, const uint32_t *key_idx, uint64_t n,
                        uint8_t *verdict, int device);
/* Same with DEVICE pointers (msg_blob needs >= 16 readable bytes past the last
 * message); synchronous on `stream` (NULL = library stream).  Indices are not
 * checked on the host here: a check whose key_idx is >= the key count or whose
 * msg_idx is >= n_msgs is skipped by the kernels and gets verdict 0. */
int pv_bls_verify_batch_device(const uint8_t *sig, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n_msgs,
                               const uint32_t *msg_idx, const uint32_t *key_idx, uint64_t n, uint8_t *verdict,
                               int device, void *stream);
/* sig[j] = sk[key_idx[j]] * H(message msg_idx[j]) (uncompressed 128 B); sks: k x 32 B big-endian */
int pv_bls_sign_batch(const uint8_t *sks, uint64_t k, const uint8_t *msg_blob, const uint64_t *msg_off,
                      uint64_t n_msgs, const uint32_t *msg_idx, const uint32_t *key_idx, uint64_t n, uint8_t *sig,
                      int device);
int pv_bls_sign_batch_device(const uint8_t *sks, const uint8_t *msg_blob, const uint64_t *msg_off, uint64_t n_msgs,
                             const uint32_t *msg_idx, const uint32_t *key_idx, uint64_t n, uint8_t *sig, int device,
                             void *stream);
/* n multi-signature checks from HOST memory; replaces n calls of
 *   BlsCryptoVerifierIndyCrypto.verify_multi_sig(signature, message, pks)
 *   (crypto/bls/indy_crypto/bls_crypto_indy_crypto.py:84-97), made once per
 *   ledger of every PRE-PREPARE by BlsBftReplicaPlenum._validate_multi_sig
 *   (plenum/bls/bls_bft_replica_plenum.py:43-50, 212-225), i.e. python-ursa
 *   Bls.verify_multi_sig: e(sigma, g) == e(H(msg), sum of the keys).
 * Check j: sig[j] (128 B; sig_len as in pv_bls_verify_batch), message
 * msg_idx[j] of msg_blob/msg_off, keys pks[pk_off[j] .. pk_off[j+1]) (128 B each,
 * decoded as keys are; an empty set sums to O).  The sum is prepared like a key
 * (PV_BLS_KEY_NOT_IN_G2 -> verdict 0) together with the generator `gen`; the key
 * set of pv_bls_set_keys is not touched.  At most 65535 checks per call. */
int pv_bls_verify_multi_batch(const uint8_t *gen, const uint8_t *sig, const uint64_t *sig_len, const uint8_t *msg_blob,
                              const uint64_t *msg_off, uint64_t n_msgs, const uint32_t *msg_idx, const uint8_t *pks,
                              const uint64_t *pk_off, uint64_t n, uint8_t *verdict, int device);
/* m multi-signatures; replaces m calls of
 *   BlsCryptoVerifierIndyCrypto.create_multi_sig(signatures) (:99-102), made by
 *   BlsBftReplicaPlenum._calculate_single_multi_sig (bls_bft_replica_plenum.py:278-288),
 *   i.e. python-ursa MultiSignature.new: the sum of the signatures' G1 points.
 * Set j = sigs[set_off[j] .. set_off[j+1]) (128 B each, decoded as sigma is);
 * out[j] = the sum's 128-byte representation: 0x04|x|y, zero-padded; the point
 * at infinity as 0x04|0|1 (AMCL's affine (0, 1) of O). */
int pv_bls_aggregate_sigs(const uint8_t *sigs, const uint64_t *set_off, uint64_t m, uint8_t *out, int device);
/* pks[i] = sks[i] * gen (k keys, 128 B each) */
int pv_bls_pubkeys(const uint8_t *gen, const uint8_t *sks, uint64_t k, uint8_t *pks, int device);
/* HIP-event durations of the last verify call on `device`: message hashing and the check kernel */
int pv_bls_kernel_ms(int device, float *hash_ms, float *verify_ms);
const char *pv_bls_last_error(void);
void pv_bls_shutdown(void);

#ifdef __cplusplus
}
#endif

#endif /* PLENUM_VERIFY_H */
