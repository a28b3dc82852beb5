// Internal launch interface between the C-ABI layer (pv_api*.cpp) and the HIP
// kernels (pv_kernels.hip).  All pointers are device pointers on the current
// device; every launch is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pv {

// base-point table: 129 niels entries (k*B, k = 0..128), 32 words each
constexpr int BTAB_ENTRIES = 129;
constexpr int BTAB_WORDS = 32;
constexpr int BTAB_CHUNKS = 8;     // tables for 2^(32 q) B, q = 0..7 (comb kernel of prepared keys)
// per-lane scratch: A table (9 cached entries k*(-A), 40 words each) + the
// CURVE_K points awaiting the shared inversion (40 words each)
#ifndef PV_CURVE_K
#define PV_CURVE_K 8
#endif
constexpr int ATAB_WORDS = 9 * 40 + PV_CURVE_K * 40;
constexpr int CURVE_BLOCK = 256;
constexpr int HASH_BLOCK = 256;

struct DeviceCaps {
  int cu_count;
  int curve_blocks;  // persistent grid for the curve kernel
};

hipError_t launch_btable_init(uint32_t* btab, hipStream_t s);

// resident curve-kernel blocks per CU (occupancy query)
hipError_t curve_occupancy(int* blocks_per_cu, bool keyed = false);

// pre[i] = 1 iff S canonical, R/A not small order, A canonical;
// dig[i] (16 words) = SHA-512(R||A||M) when pre[i] (reduced mod L by the curve
// kernel).  Persistent grid of `blocks` blocks; `counter` is an 8-byte device
// word the launch resets (work queue).
hipError_t hash_occupancy(int* blocks_per_cu);
// kidx (may be NULL): signature i's key is pk[kidx[i]] (keyed batches)
// pre != null: k_precheck writes the pre-check verdicts first and k_hash skips
// the rejected signatures; pre == null: every signature is hashed (the
// half-size path checks in launch_lattice)
hipError_t launch_hash(const uint8_t* pk, const uint8_t* sig, const uint8_t* blob, const uint64_t* off, uint64_t n,
                       unsigned long long* counter, uint32_t* dig, uint8_t* pre, int blocks, hipStream_t s,
                       const uint32_t* kidx = nullptr);

// verdict[i] in {0,1}; bitmap[i/64] bit i%64 (bitmap must hold ceil(n/64) words);
// h = the hash kernel's digests (16 words per signature)
// ktab/kidx (may be NULL): keyed mode, signature i uses prepared key kidx[i]
hipError_t launch_curve(const uint8_t* pk, const uint8_t* sig, const uint32_t* h, const uint8_t* pre,
                        const uint32_t* btab, uint32_t* scratch, uint64_t scratch_lanes, uint8_t* verdict,
                        uint64_t* bitmap, uint64_t n, int blocks, hipStream_t s, const uint32_t* ktab = nullptr,
                        const uint32_t* kidx = nullptr, const uint32_t* bw = nullptr,
                        unsigned long long* tasks = nullptr,    // wave task queue counter (zeroed here)
                        bool wide = false);                     // ktab in the wide (radix-256) key format

// Half-size scalar path (generic batches, pv_lattice.h):
//   launch_lattice   pre-checks (-> pre) and h mod L -> (c, d, s') records
//                    (HSREC_WORDS words per signature), deferred indices ->
//                    dlist / *dcount; also
//                    zeroes *tasks and the bitmap (ceil(n/64) words) the curve
//                    kernel ORs into.  n < 2^32.
//   launch_curve_half  verdicts + bitmap; per-lane scratch HALF_SCRATCH_WORDS
//                    (tables of +-A and -R).
constexpr int HSREC_WORDS = 20;
constexpr int HALF_SCRATCH_WORDS = 2 * 9 * 40;
hipError_t curve_half_occupancy(int* blocks_per_cu);
// latency mode for small batches: lane pairs per signature, per-lane scratch
// ATAB_LAT_WORDS (one 9-entry table)
constexpr int ATAB_LAT_WORDS = 9 * 40;
hipError_t launch_curve_lat(const uint8_t* pk, const uint8_t* sig, const uint32_t* dig, const uint32_t* rec,
                            const uint32_t* btab, const uint32_t* bw, uint32_t* scratch, uint64_t scratch_lanes,
                            uint8_t* verdict, uint64_t* bitmap, uint64_t n, hipStream_t s);
// latency mode in one launch: pre-checks + hash + scalar stage (one wave) and
// the lane-quad curve stage (another) per block of 8 signatures; *dcount +=
// the deferred records (caller zeroes it); the bitmap needs no zeroing
hipError_t launch_verify_quad(const uint8_t* pk, const uint8_t* sig, const uint8_t* blob, const uint64_t* off, uint64_t n,
                              const uint32_t* bw, uint8_t* verdict, uint64_t* bitmap, unsigned long long* dcount,
                              bool force_full, hipStream_t s);
// host-buffer chunks: the whole half-size verify of a chunk in one persistent
// launch (pre-checks + hash + lattice + curve per 64-signature task; rec =
// HSREC_WORDS per signature, scratch as launch_curve_half); deferred records
// are appended to dlist as base + i (*dcount, zeroed by the caller) and left
// for launch_verify_quad_list, which verifies the listed indices (count read
// on the device; max_count bounds the grid) with the lane-quad kernel
hipError_t launch_chunk_half(const uint8_t* pk, const uint8_t* sig, const uint8_t* blob, const uint64_t* off,
                             uint64_t n, uint32_t* rec, const uint32_t* bw, uint32_t* scratch, uint64_t scratch_lanes,
                             uint8_t* verdict, uint32_t* dlist, unsigned long long* dcount, uint64_t base,
                             unsigned long long* tasks, int blocks, bool force_full, hipStream_t s);
hipError_t launch_verify_quad_list(const uint8_t* pk, const uint8_t* sig, const uint8_t* blob, const uint64_t* off,
                                   const uint32_t* list, const unsigned long long* lcount, uint64_t max_count,
                                   int blocks, const uint32_t* bw, uint8_t* verdict, bool force_full, hipStream_t s);
hipError_t launch_lattice(const uint8_t* pk, const uint8_t* sig, const uint32_t* dig, uint8_t* pre, uint64_t n,
                          uint32_t* rec, uint32_t* dlist, unsigned long long* dcount, unsigned long long* tasks,
                          uint64_t* bitmap, bool force_full, hipStream_t s);
// btab: the radix-256 base-point tables (deferred full-length tasks); bw:
// BWTAB_WORDS words, the radix-2^16 chunk tables k * 2^(32 q) * B, q = 0..7
// (launch_bw_init; chunks 0 and 4 serve the half-size path, all eight the
// keyed comb)
constexpr int BWTAB_ENTRIES = (1 << 15) + 1;
constexpr uint64_t BWTAB_WORDS = 8ull * BWTAB_ENTRIES * BTAB_WORDS;
hipError_t launch_bw_init(uint32_t* bw, hipStream_t s);
hipError_t launch_curve_half(const uint8_t* pk, const uint8_t* sig, const uint32_t* dig, const uint32_t* rec,
                             const uint32_t* btab, const uint32_t* bw, uint32_t* scratch, uint64_t scratch_lanes,
                             uint8_t* verdict, uint64_t* bitmap, uint64_t n, const uint32_t* dlist,
                             const unsigned long long* dcount, unsigned long long* tasks, int blocks, hipStream_t s);

// prepared keys: KEYTAB_WORDS words per key (8 comb tables of affine multiples
// k * 2^(32 q) * (-A) + status); KEYTAB_SCRATCH words of scratch per key
constexpr int KEYTAB_WORDS = 8 * 9 * 32 + 32;
constexpr int KEYTAB_SCRATCH = 64 * 40;   // projective entries + prefix products (lane-interleaved per 64 keys)
hipError_t launch_keys(const uint8_t* pk, uint64_t k, uint32_t* ktab, uint32_t* scr, hipStream_t s);
// wide key format (radix-256 comb, node keys): KEYTAB_WIDE_WORDS words per key,
// KEYTAB_WIDE_SCRATCH words of scratch per lane (KEYTAB_WIDE_LANES lanes per
// key: 16 per table, lane-interleaved per 64)
constexpr int KEYTAB_WIDE_WORDS = 8 * 129 * 32 + 32;
constexpr int KEYTAB_WIDE_LANES = 128;
constexpr int KEYTAB_WIDE_SCRATCH = 8 * 40;
hipError_t launch_keys_wide(const uint8_t* pk, uint64_t k, uint32_t* ktab, uint32_t* scr, hipStream_t s);
// latency mode for prepared keys (k_verify_quad_keyed): the whole verify of n
// signatures in one launch, signature e's key = ktab entry kidx[i] with i =
// list ? list[e] : e; the hashed key bytes are pk + 32 * (pk_by_key ? kidx[i] : i).
// Verdicts go to verdict[i]; bitmap (ceil(n/64) words, needs no zeroing) only
// without a list (may be NULL then too).  flag (host-mapped) / done (a device
// counter at 0): the last block writes seq to *flag when every verdict is out
// and re-arms *done (both NULL: no completion word)
hipError_t launch_verify_quad_keyed(const uint8_t* pk, bool pk_by_key, const uint8_t* sig, const uint8_t* blob,
                                    const uint64_t* off, uint64_t n, const uint32_t* list, const uint32_t* ktab,
                                    const uint32_t* kidx, const uint32_t* bw, uint8_t* verdict, uint64_t* bitmap,
                                    hipStream_t s, uint32_t* done = nullptr, uint32_t* flag = nullptr,
                                    uint32_t seq = 0);

// completion signal of a zero-copy host call: *flag = seq (system scope, after
// every earlier kernel of the stream), polled by the host instead of a stream
// synchronize (run_small)
hipError_t launch_signal(uint32_t* flag, uint32_t seq, hipStream_t s);

// keygen + sign: pk[i], sig[i] for seed[i] over M_i
hipError_t launch_sign(const uint8_t* seeds, const uint8_t* blob, const uint64_t* off, uint64_t n,
                       const uint32_t* btab, uint8_t* pk_out, uint8_t* sig_out, hipStream_t s);

// per-batch quorum tally over per-message verdicts + sender indices (*bad |= 1
// when a sender index is >= n_nodes), and over node-indexed voter bitmaps
hipError_t launch_tally(const uint8_t* verdict, const uint32_t* sender, const uint64_t* batch_off,
                        uint64_t n_batches, uint32_t n_nodes, uint32_t quorum, uint32_t* votes,
                        uint8_t* reached, uint32_t* bad, hipStream_t s);
hipError_t launch_tally_bits(const uint32_t* bits, const uint32_t* dup, uint64_t n_batches, uint32_t n_nodes,
                             uint32_t quorum, uint32_t* votes, uint8_t* reached, hipStream_t s);

// SHA-256 / Merkle: out (n x 8 words) = SHA-256(prefix || M_i)
// (plen 0 or 1 prefix bytes); one Merkle level m -> ceil(m/2) nodes
hipError_t sha256_occupancy(int* blocks_per_cu);
hipError_t launch_sha256(const uint8_t* blob, const uint64_t* off, uint64_t n, uint32_t plen, uint32_t prefix,
                         unsigned long long* counter, uint32_t* out, int blocks, hipStream_t s);
hipError_t launch_merkle_level(const uint32_t* in, uint64_t m, uint32_t* out, hipStream_t s);
// the remaining levels of m (2 <= m <= MERKLE_TAIL) nodes in one workgroup -> root
constexpr int MERKLE_TAIL = 256;
hipError_t launch_merkle_tail(const uint32_t* in, uint64_t m, uint32_t* root, hipStream_t s);

// Merkle audit paths / consistency proofs (pv_merkle_proof.h), one proof or
// request per lane; digests are 8 words each and 16-byte aligned, proof_off
// (n + 1 entries) counts nodes, max_blocks caps the grid-stride grid.
//   verify_incl  leaf (n x 8) + index / tree_size + nodes -> status, computed, stop_index;
//                proof i's root is roots[root_idx ? root_idx[i] : i]
//   verify_cons  the same for (old_size, new_size) pairs and their two roots
//   level_keep   parents first_out .. ceil(m/2) - 1 of one level (resident tree)
//   paths / cons_proofs  lv = device table of level pointers of a tree of n
//                leaves and `depth` levels above them; request i writes at most
//                depth + 1 nodes at stride depth + 1, its length (MP_LEN_REFUSED
//                for a request outside the tree) and, for paths, MTH(0, s)
hipError_t launch_merkle_verify_incl(const uint32_t* leaf, const uint64_t* index, const uint64_t* tree_size,
                                     const uint32_t* nodes, const uint64_t* proof_off, const uint32_t* roots,
                                     const uint32_t* root_idx, uint64_t n, uint8_t* status, uint32_t* computed,
                                     uint64_t* stop_index, int max_blocks, hipStream_t s);
hipError_t launch_merkle_verify_cons(const uint64_t* old_size, const uint64_t* new_size, const uint32_t* old_roots,
                                     const uint32_t* new_roots, const uint32_t* old_idx, const uint32_t* new_idx,
                                     const uint32_t* nodes, const uint64_t* proof_off, uint64_t n, uint8_t* status,
                                     uint32_t* old_computed, uint32_t* new_computed, int max_blocks, hipStream_t s);
hipError_t launch_merkle_level_keep(const uint32_t* in, uint64_t first_out, uint64_t m, uint32_t* out, hipStream_t s);
hipError_t launch_merkle_paths(const uint32_t* const* lv, uint64_t n, uint32_t depth, const uint64_t* index,
                               const uint64_t* tree_size, uint64_t k, uint32_t* nodes_out, uint32_t* len_out,
                               uint32_t* roots_out, int max_blocks, hipStream_t s);
hipError_t launch_merkle_cons_proofs(const uint32_t* const* lv, uint64_t n, uint32_t depth, const uint64_t* first,
                                     const uint64_t* second, uint64_t k, uint32_t* nodes_out, uint32_t* len_out,
                                     int max_blocks, hipStream_t s);

// The ledger write cycle over a resident tree (pv_merkle_ledger.h).
//   edge       every ancestor of the leaves [f0, n_new), f0 < n_new <= f0 + MERKLE_EDGE_MAX, in one
//              launch of one workgroup; levels[0 .. n_levels) are HOST-side copies of the level
//              pointers, level l with room for the nodes of n_new leaves
//   hs_gather  leaf hashes and writeNode-ordered nodes of the leaves (first, last]; either output may be null
//   hs_check   the same nodes compared with `nodes`: res[0] += differing, res[1] = min(res[1], first differing)
//   frontier   CompactMerkleTree.hashes of the prefix of `size` leaves, largest subtree first
constexpr uint32_t MERKLE_EDGE_MAX = 1024;
hipError_t launch_merkle_edge(uint32_t* const* levels, uint32_t n_levels, uint64_t f0, uint64_t n_new, hipStream_t s);
hipError_t launch_merkle_hs_gather(const uint32_t* const* lv, uint64_t first, uint64_t last, uint32_t* leaf_out,
                                   uint32_t* node_out, int max_blocks, hipStream_t s);
hipError_t launch_merkle_hs_check(const uint32_t* const* lv, uint64_t first, uint64_t last, const uint32_t* nodes,
                                  unsigned long long* res, int max_blocks, hipStream_t s);
hipError_t launch_merkle_frontier(const uint32_t* const* lv, uint64_t size, uint32_t* out, hipStream_t s);

// SHA3-256 / Patricia-trie state proofs (pv_sha3.h, pv_trie_proof.h).
//   sha3_256     out (n x 8 words, 16-byte aligned) = SHA3-256(blob[beg[i] .. end[i])); the
//                work queue of launch_sha256 (`counter` reset by the launch); the blob needs
//                >= 16 readable bytes after the last message
//   trie_verify  one query per lane: proof proof_idx[i] = nodes proof_first[p] ..
//                proof_first[p + 1] - 1 with digests node_dig, root roots[p] (8 words), key and
//                expected encoded value -> status[i] (SP_*)
hipError_t sha3_occupancy(int* blocks_per_cu);
hipError_t launch_sha3_256(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, uint64_t n,
                           unsigned long long* counter, uint32_t* out, int blocks, hipStream_t s);
hipError_t launch_trie_verify(const uint8_t* node_blob, const uint64_t* node_beg, const uint64_t* node_end,
                              const uint32_t* node_dig, const uint64_t* proof_first, const uint32_t* roots,
                              uint64_t n_proofs, const uint32_t* proof_idx, const uint8_t* key_blob,
                              const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off, uint64_t n,
                              uint8_t* status, int max_blocks, hipStream_t s);

// Resident trie node store and state-proof generation (pv_trie_store.h); all device memory.
//   trie_store_layout  node first + i = blob[base + (node_off[i] - node_off[0]) ..
//                      base + (node_off[i + 1] - node_off[0])); a range that is empty, reversed or
//                      ends past `total` becomes the empty range at base (never read, walks as
//                      malformed)
//   trie_store_insert  one lane per new node id first .. first + n_new - 1 (hashed already);
//                      *unique += the nodes whose digest the table did not hold; dup[] flags the rest
//   trie_store_rehash  ids 0 .. n - 1 that are not flagged, into an empty table
//   trie_prove         one query per lane: root roots[root_idx ? root_idx[q] : q], key q ->
//                      status, node_count, node_ids[q * max_nodes ..], proof_len, val_rel, val_len
//   trie_proof_pack    one wave per proof: list header at proof_off[q], then the nodes' bytes in
//                      reverse walk order; a proof whose ids do not add up to
//                      proof_off[q + 1] - proof_off[q] bytes is not written
hipError_t launch_trie_store_layout(const uint64_t* node_off, uint64_t n_new, uint64_t base, uint64_t total,
                                    uint64_t* beg, uint64_t* end, uint64_t first, int max_blocks, hipStream_t s);
hipError_t launch_trie_store_insert(uint32_t* table, uint32_t slots, const uint32_t* dig, uint8_t* dup,
                                    uint32_t first, uint32_t n_new, unsigned int* unique, int max_blocks,
                                    hipStream_t s);
hipError_t launch_trie_store_rehash(uint32_t* table, uint32_t slots, const uint32_t* dig, uint8_t* dup, uint32_t n,
                                    int max_blocks, hipStream_t s);
hipError_t launch_trie_prove(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                             const uint32_t* table, uint32_t slots, uint32_t n_nodes, const uint32_t* roots,
                             const uint32_t* root_idx, uint64_t n_roots, const uint8_t* key_blob,
                             const uint64_t* key_off, uint64_t n_queries, uint32_t max_nodes, uint8_t* status,
                             uint32_t* node_count, uint32_t* node_ids, uint64_t* proof_len, uint64_t* val_rel,
                             uint64_t* val_len, int max_blocks, hipStream_t s);
hipError_t launch_trie_proof_pack(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, uint32_t n_nodes,
                                  const uint32_t* node_ids, const uint32_t* node_count, uint32_t max_nodes,
                                  const uint64_t* proof_off, uint64_t n_queries, uint8_t* proof_blob, int max_blocks,
                                  hipStream_t s);

// Reads from the resident store (pv_trie_get.h); all device memory.
//   trie_get       one query per lane: status, found, src[q] (where the value lies in the store's
//                  blob) and val_off[q] <- the value's length, val_off[n_queries] <- 0; the caller
//                  scans val_off (n_queries + 1) in place
//   trie_get_copy  TG_GROUP lanes per value: val_blob[val_off[q] ..] <- the value's bytes
hipError_t launch_trie_get(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                           const uint32_t* table, uint32_t slots, uint32_t n_nodes, const uint32_t* roots,
                           const uint32_t* root_idx, uint64_t n_roots, const uint8_t* key_blob,
                           const uint64_t* key_off, uint64_t n_queries, bool decode, uint8_t* status, uint8_t* found,
                           uint64_t* src, uint64_t* val_off, int max_blocks, hipStream_t s);
hipError_t launch_trie_get_copy(const uint8_t* blob, const uint64_t* src, const uint64_t* val_off, uint64_t n_queries,
                                uint8_t* val_blob, int max_blocks, hipStream_t s);

// Pruning the resident store (pv_trie_prune.h); all device memory.
//   trie_prune_seed   one lane per kept root: status[i], the root's node marked and enqueued
//   trie_prune_level  one lane per queue entry head .. tail - 1: tp_expand (children marked, the
//                     newly marked ones appended at c.counts[TP_TAIL])
//   trie_prune_flags  keep[i] / len[i], i = 0 .. n (0 at n): what the two exclusive scans take
//   trie_prune_copy   one wave per old id: a marked one to new id keep[i] at byte off[i] (scanned);
//                     nblob == nullptr: the digests alone
struct TpCtx;
hipError_t launch_trie_prune_seed(const TpCtx& c, const uint32_t* roots, uint64_t n_roots, uint8_t* status,
                                  int max_blocks, hipStream_t s);
hipError_t launch_trie_prune_level(const TpCtx& c, uint64_t head, uint64_t tail, int max_blocks, hipStream_t s);
hipError_t launch_trie_prune_flags(const uint32_t* bits, const uint64_t* beg, const uint64_t* end, uint64_t n,
                                   uint64_t* keep, uint64_t* len, int max_blocks, hipStream_t s);
hipError_t launch_trie_prune_copy(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                                  const uint32_t* bits, const uint64_t* keep, const uint64_t* off, uint64_t n,
                                  uint8_t* nblob, uint64_t* nbeg, uint64_t* nend, uint32_t* ndig, int max_blocks,
                                  hipStream_t s);

// Batch trie build (pv_trie_build.h); all device memory.  One item per lane of the routine
// named: tb_lcp_one over positions 0 .. n (stats[0] <- max h by atomicMax, stats[1 .. 3] <- the
// first index refused for order / value / offsets by atomicMin), tb_min_one over the `size`
// entries of tree level lv, tb_struct_one over the keys (*root_e <- the root's entity),
// tb_size_one / tb_emit_one over the entities of level lv.
struct TbCtx;
hipError_t launch_trie_build_lcp(const TbCtx& c, uint32_t* stats, int max_blocks, hipStream_t s);
hipError_t launch_trie_build_min(const TbCtx& c, uint32_t lv, uint64_t size, int max_blocks, hipStream_t s);
hipError_t launch_trie_build_struct(const TbCtx& c, uint32_t* root_e, int max_blocks, hipStream_t s);
hipError_t launch_trie_build_size(const TbCtx& c, uint32_t lv, int max_blocks, hipStream_t s);
hipError_t launch_trie_build_emit(const TbCtx& c, uint32_t lv, int max_blocks, hipStream_t s);

// Sets onto a committed root (pv_trie_update.h); all device memory.  tu_walk over the batch
// keys, one key per lane: count mode (status[j], cnt / pbytes / vbytes [j]), then, after the
// three scans, write mode (the merged items).
struct TuCtx;
hipError_t launch_trie_update_count(const TuCtx& c, int max_blocks, hipStream_t s);
hipError_t launch_trie_update_emit(const TuCtx& c, int max_blocks, hipStream_t s);

// Sets and removals onto a committed root: the same two passes with tu_walk_t<true>, in which the
// lane of an empty value is a removal (it emits no value and opens the children it carries).
hipError_t launch_trie_apply_count(const TuCtx& c, int max_blocks, hipStream_t s);
hipError_t launch_trie_apply_emit(const TuCtx& c, int max_blocks, hipStream_t s);

// sorting state keys (pv_trie_sort.h): the first kernel's checks, one LSD pass, the flag pass,
// perm, and the gather of the kept pairs into compact blobs
struct TsRec;
uint64_t trie_sort_blocks(uint64_t n);
hipError_t launch_trie_sort_init(const uint8_t* key_blob, const uint64_t* key_off, const uint64_t* val_off,
                                 bool empty_ok, uint64_t n, TsRec* rec, uint32_t* stats, int max_blocks,
                                 hipStream_t s);
hipError_t launch_trie_sort_round(const uint8_t* key_blob, const uint64_t* key_off, const TsRec* in, const uint64_t* x,
                                  uint64_t n, uint32_t r, TsRec* out, int max_blocks, hipStream_t s);
hipError_t launch_trie_sort_pass(const TsRec* in, uint64_t n, uint32_t p, uint64_t* table, uint64_t* sums, TsRec* out,
                                 hipStream_t s);
hipError_t launch_trie_sort_flags(const TsRec* rec, uint64_t n, uint64_t* x, int max_blocks, hipStream_t s);
hipError_t launch_trie_sort_finish(const TsRec* rec, const uint64_t* x, uint64_t n, uint32_t* perm, int max_blocks,
                                   hipStream_t s);
hipError_t launch_trie_sort_lens(const uint32_t* perm, uint64_t m, uint64_t n, const uint64_t* key_off,
                                 const uint64_t* val_off, uint64_t* klen, uint64_t* vlen, int max_blocks,
                                 hipStream_t s);
hipError_t launch_trie_sort_copy(const uint32_t* perm, uint64_t m, uint64_t n, const uint8_t* key_blob,
                                 const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                                 const uint64_t* out_koff, const uint64_t* out_voff, uint8_t* out_keys,
                                 uint8_t* out_vals, int max_blocks, hipStream_t s);

// deterministic synthetic workload; spec in plenum_gpu/synth.py.
// mode 0 FIXED (len = mlen_min), 1 RANGE (len uniform in [mlen_min, mlen_max]),
// 2 COMMIT (C3 3PC batches of n_nodes votes).
// off (n+1) <- exclusive prefix sum of message lengths; sums = scan_sums_words(n+1) words
uint64_t scan_sums_words(uint64_t m);
hipError_t launch_exclusive_scan(uint64_t* x, uint64_t m, uint64_t* sums, hipStream_t s);
hipError_t launch_synth_layout(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t mlen_min,
                               uint32_t mlen_max, uint32_t n_nodes, uint64_t* off, uint64_t* sums, hipStream_t s);
hipError_t launch_synth(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t key_mod, uint32_t n_nodes,
                        uint8_t* seeds_out, uint8_t* tamper_out, uint32_t* sender_out, hipStream_t s);
hipError_t launch_synth_fill(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t n_nodes,
                             const uint64_t* off, uint8_t* blob, hipStream_t s);
hipError_t launch_tamper(uint64_t first, uint64_t n, const uint8_t* tamper, const uint64_t* off, uint8_t* blob,
                         uint8_t* sig, hipStream_t s);

}  // namespace pv
