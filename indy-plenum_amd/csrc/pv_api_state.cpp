// The state-proof part of include/plenum_verify.h: pv_sha3_256_batch*,
// pv_rlp_split_list, pv_state_proof_verify*, and the resident trie node store
// (pv_state_store_*: add, walk / pack / prove, prune).
#include "pv_api_common.h"
#include "pv_trie_proof.h"
#include "pv_trie_store.h"
#include "pv_trie_prune.h"

using namespace pvapi;

static_assert(pv::SP_OK == PV_SP_OK && pv::SP_VALUE_MISMATCH == PV_SP_VALUE_MISMATCH &&
                  pv::SP_NODE_MISSING == PV_SP_NODE_MISSING && pv::SP_MALFORMED == PV_SP_MALFORMED,
              "public state-proof status codes");

extern "C" {

// ------------------------------------------------ SHA3-256 / state proofs
int pv_sha3_256_batch_device(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* digests, int device,
                             void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!blob || !off || !digests) return fail(PV_EINVAL, "null device buffer");
  if (misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(blob) & 3u) return fail(PV_EINVAL, "blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_sha3_256(blob, off, off + 1, n, en.d->counter.p, w32(digests), en.d->sha3_blocks, en.s));
  return en.finish();
}

int pv_sha3_256_batch(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* digests) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!off || !digests || (!blob && off[n] != off[0])) return fail(PV_EINVAL, "null buffer");
  Ragged msgs(off, n);
  if (const int rc = msgs.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure(n * 8));
  if (const int rc = msgs.stage(blob, d, d.stream)) return rc;
  HIP_OK(pv::launch_sha3_256(d.blob.p, d.off.p, d.off.p + 1, n, d.counter.p, d.mk0.p, d.sha3_blocks, d.stream));
  HIP_OK(hipMemcpyAsync(digests, d.mk0.p, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_rlp_split_list(const uint8_t* rlp, uint64_t len, uint64_t* item_beg, uint64_t* item_end, uint64_t cap,
                      uint64_t* count) {
  if (!count || (len && !rlp) || (cap && (!item_beg || !item_end))) return fail(PV_EINVAL, "null buffer");
  if (!pv::rlp_split_list(rlp, len, item_beg, item_end, cap, count))
    return fail(PV_EINVAL, "not one RLP list of at most %llu items ending at its end", (unsigned long long)cap);
  return PV_OK;
}

int pv_state_proof_verify_device(const uint8_t* node_blob, const uint64_t* node_beg, const uint64_t* node_end,
                                 const uint64_t* proof_first, const uint8_t* roots, const uint32_t* proof_idx,
                                 const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                                 const uint64_t* val_off, uint64_t N, uint64_t P, uint64_t Q, uint8_t* status,
                                 uint8_t* node_digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (Q == 0) return PV_OK;
  if (!proof_first || !roots || !proof_idx || !key_off || !val_off || !status ||
      (N && (!node_blob || !node_beg || !node_end || !node_digests)))
    return fail(PV_EINVAL, "null device buffer");
  if (P == 0) return fail(PV_EINVAL, "queries without proofs");
  if (misaligned16(node_digests) || (reinterpret_cast<uintptr_t>(roots) & 3u) ||
      (reinterpret_cast<uintptr_t>(node_blob) & 3u))
    return fail(PV_EINVAL, "node_digests must be 16-byte aligned, roots and node_blob 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  HIP_OK(pv::launch_sha3_256(node_blob, node_beg, node_end, N, d->counter.p, w32(node_digests), d->sha3_blocks, s));
  HIP_OK(pv::launch_trie_verify(node_blob, node_beg, node_end, w32(node_digests), proof_first, w32(roots), P,
                                proof_idx, key_blob, key_off, val_blob, val_off, Q, status, merkle_blocks(*d), s));
  return en.finish();
}

int pv_state_proof_verify(const uint8_t* node_blob, uint64_t node_blob_len, const uint64_t* node_beg,
                          const uint64_t* node_end, const uint64_t* proof_first, const uint8_t* roots,
                          const uint32_t* proof_idx, const uint8_t* key_blob, const uint64_t* key_off,
                          const uint8_t* val_blob, const uint64_t* val_off, uint64_t N, uint64_t P, uint64_t Q,
                          uint8_t* status) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (Q == 0) return PV_OK;
  if (!proof_first || !roots || !proof_idx || !key_off || !val_off || !status ||
      (N && (!node_beg || !node_end)) || (node_blob_len && !node_blob))
    return fail(PV_EINVAL, "null buffer");
  if (P == 0) return fail(PV_EINVAL, "queries without proofs");
  Ragged keys(key_off, Q), vals(val_off, Q);
  if (const int rc = keys.check("key_off")) return rc;
  if (const int rc = vals.check("val_off")) return rc;
  if ((keys.len && !key_blob) || (vals.len && !val_blob)) return fail(PV_EINVAL, "null buffer");
  for (uint64_t j = 0; j < N; ++j)
    if (node_beg[j] > node_end[j] || node_end[j] > node_blob_len)
      return fail(PV_EINVAL, "node %llu lies outside the blob", (unsigned long long)j);
  if (const int rc = offsets_ok(proof_first, P, "proof_first")) return rc;
  if (proof_first[P] != N)
    return fail(PV_EINVAL, "proof_first ends at %llu, not at N = %llu", (unsigned long long)proof_first[P],
                (unsigned long long)N);
  for (uint64_t i = 0; i < Q; ++i)
    if (proof_idx[i] >= P)
      return fail(PV_EINVAL, "proof_idx[%llu] = %u is not below P = %llu", (unsigned long long)i, proof_idx[i],
                  (unsigned long long)P);
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dblob, droots, dkeys, dvals, dstatus, ddig;
  TmpBuf<uint64_t> dbeg, dend, dfirst, dkoff, dvoff;
  TmpBuf<uint32_t> dpidx;
  StreamDrain tail{s};
  HIP_OK(dblob.alloc(node_blob_len + 16));
  if (const int rc = upload_padded(dblob.p, node_blob, node_blob_len, s)) return rc;
  HIP_OK(dbeg.put(node_beg, N, s));
  HIP_OK(dend.put(node_end, N, s));
  HIP_OK(dfirst.put(proof_first, P + 1, s));
  HIP_OK(droots.put(roots, P * 32, s));
  HIP_OK(dpidx.put(proof_idx, Q, s));
  HIP_OK(dkeys.put(keys.len ? key_blob + keys.b0 : nullptr, keys.len, s));
  HIP_OK(dkoff.put(keys.rebased(), Q + 1, s));
  HIP_OK(dvals.put(vals.len ? val_blob + vals.b0 : nullptr, vals.len, s));
  HIP_OK(dvoff.put(vals.rebased(), Q + 1, s));
  HIP_OK(dstatus.alloc(Q));
  HIP_OK(ddig.alloc(N * 32));
  HIP_OK(pv::launch_sha3_256(dblob.p, dbeg.p, dend.p, N, d.counter.p, w32(ddig.p), d.sha3_blocks, s));
  HIP_OK(pv::launch_trie_verify(dblob.p, dbeg.p, dend.p, w32(ddig.p), dfirst.p, w32(droots.p), P, dpidx.p, dkeys.p,
                                dkoff.p, dvals.p, dvoff.p, Q, dstatus.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, Q, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

}  // extern "C"

// --------------------------------- resident trie node store / proof generation
static void store_drop(StateStore& st) {
  void* bufs[] = {st.blob, st.beg, st.end, st.dig, st.dup, st.table, st.unique};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
}
HandleTable<StateStore> pvapi::g_stores{store_drop, "state store", "id"};
void pvapi::release_stores() { g_stores.release_all(); }

// the store holds at least `nodes` nodes and `bytes` bytes of them afterwards
int pvapi::store_reserve(StateStore& st, uint64_t nodes, uint64_t bytes, hipStream_t s) {
  if (const int rc = grow_device(&st.blob, &st.cap_bytes, bytes, st.n_bytes, 16, 1, s)) return rc;
  if (nodes <= st.cap_nodes && st.beg) return PV_OK;
  // the four per-node arrays grow in step: same start, same doubling
  uint64_t c0 = st.cap_nodes, c1 = st.cap_nodes, c2 = st.cap_nodes, cd = st.cap_nodes * 8;
  if (const int rc = grow_device(&st.beg, &c0, nodes, st.n_nodes, 0, 1, s)) return rc;
  if (const int rc = grow_device(&st.end, &c1, nodes, st.n_nodes, 0, 1, s)) return rc;
  if (const int rc = grow_device(&st.dup, &c2, nodes, st.n_nodes, 0, 1, s)) return rc;
  if (const int rc = grow_device(&st.dig, &cd, c0 * 8, st.n_nodes * 8, 0, 1, s)) return rc;
  st.cap_nodes = c0;
  return PV_OK;
}

// a table of `slots` slots holding every node that has one; launched before an
// insert that would push the nodes above slots / 2
int pvapi::store_rehash(StateStore& st, uint32_t slots, const Device& d, hipStream_t s) {
  uint32_t* nt = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&nt), (size_t)slots * 4));
  hipError_t e = hipMemsetAsync(nt, 0, (size_t)slots * 4, s);
  if (e == hipSuccess)
    e = pv::launch_trie_store_rehash(nt, slots, st.dig, st.dup, (uint32_t)st.n_nodes, merkle_blocks(d), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(nt);
    HIP_OK(e);
  }
  if (st.table) (void)hipFree(st.table);
  st.table = nt;
  st.slots = slots;
  return PV_OK;
}

namespace {

// pv_state_store_add[_device]: host = the arrays are host memory and checked here
int store_add(int32_t id, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new, uint8_t* digests,
              uint64_t* n_added, bool host, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, id, &st)) return rc;
  if (n_added) *n_added = 0;
  if (n_new == 0) return PV_OK;
  if (!node_blob || !node_off) return fail(PV_EINVAL, host ? "null buffer" : "null device buffer");
  if (n_new > pv::TS_MAX_NODES || st->n_nodes + n_new > pv::TS_MAX_NODES)
    return fail(PV_EINVAL, "state store limited to 2^32 - 2 nodes");
  if (host)
    for (uint64_t i = 0; i < n_new; ++i)
      if (node_off[i + 1] <= node_off[i])
        return fail(PV_EINVAL, "node_off not strictly increasing at %llu (an empty node)", (unsigned long long)i);
  if (const int rc = en.begin(stream)) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  uint64_t ends[2] = {0, 0};   // node_off[0], node_off[n_new]
  if (host) {
    ends[0] = node_off[0];
    ends[1] = node_off[n_new];
  } else {   // the two ends size the copy; the offsets between them are read by the kernel only
    HIP_OK(hipMemcpyAsync(&ends[0], node_off, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&ends[1], node_off + n_new, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (ends[1] < ends[0]) return fail(PV_EINVAL, "node_off ends below its start");
  }
  const uint64_t total = ends[1] - ends[0];
  if (total > (1ull << 40)) return fail(PV_EINVAL, "more than 2^40 bytes of nodes in one call");
  const uint64_t nodes = st->n_nodes + n_new;
  if (const int rc = store_reserve(*st, nodes, st->n_bytes + total, s)) return rc;
  TmpBuf<uint64_t> doff;
  StreamDrain tail{s};
  const uint64_t* poff = node_off;
  if (host) {
    HIP_OK(doff.put(node_off, n_new + 1, s));
    poff = doff.p;
  }
  if (total)
    HIP_OK(hipMemcpyAsync(st->blob + st->n_bytes, node_blob + ends[0], total,
                          host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(st->blob + st->n_bytes + total, 0, 16, s));
  HIP_OK(hipMemsetAsync(st->dup + st->n_nodes, 0, n_new, s));
  HIP_OK(pv::launch_trie_store_layout(poff, n_new, st->n_bytes, total, st->beg, st->end, st->n_nodes,
                                      merkle_blocks(d), s));
  HIP_OK(pv::launch_sha3_256(st->blob, st->beg + st->n_nodes, st->end + st->n_nodes, n_new, d.counter.p,
                             st->dig + 8 * st->n_nodes, d.sha3_blocks, s));
  if (nodes > st->slots / 2) {
    uint64_t ns = st->slots;
    while (nodes > ns / 2) ns *= 2;   // nodes < 2^32, so ns <= 2^33
    if (ns > (1ull << 31)) return fail(PV_ENOMEM, "state store table above 2^31 slots");
    if (const int rc = store_rehash(*st, (uint32_t)ns, d, s)) return rc;
  }
  HIP_OK(pv::launch_trie_store_insert(st->table, st->slots, st->dig, st->dup, (uint32_t)st->n_nodes, (uint32_t)n_new,
                                      st->unique, merkle_blocks(d), s));
  unsigned int uniq = 0;
  HIP_OK(hipMemcpyAsync(&uniq, st->unique, 4, hipMemcpyDeviceToHost, s));
  if (digests)
    HIP_OK(hipMemcpyAsync(digests, st->dig + 8 * st->n_nodes, n_new * 32,
                          host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  if (const int rc = tail.finish()) return rc;
  if (n_added) *n_added = uniq - st->n_unique;
  st->n_unique = uniq;
  st->n_nodes = nodes;
  st->n_bytes += total;
  return PV_OK;
}

}  // namespace

extern "C" {

int pv_state_store_create(uint64_t node_hint, uint64_t byte_hint, int device, int32_t* store_out) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!store_out) return fail(PV_EINVAL, "null pointer");
  if (node_hint > pv::TS_MAX_NODES) return fail(PV_EINVAL, "node_hint above 2^32 - 2 nodes");
  if (byte_hint > (1ull << 40)) return fail(PV_EINVAL, "byte_hint above 2^40 bytes");
  int32_t id;
  StateStore* sp;
  if (const int rc = g_stores.alloc(en.d->id, &id, &sp)) return rc;
  StateStore& st = *sp;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  uint64_t slots = pv::TS_MIN_SLOTS;
  while (node_hint > slots / 2) slots *= 2;
  int rc = slots > (1ull << 31) ? fail(PV_ENOMEM, "state store table above 2^31 slots") : PV_OK;
  if (rc == PV_OK) rc = store_reserve(st, node_hint ? node_hint : 1, byte_hint ? byte_hint : 1, s);
  if (rc == PV_OK) rc = store_rehash(st, (uint32_t)slots, *en.d, s);   // an empty table
  if (rc == PV_OK) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st.unique), 4);
    if (e == hipSuccess) e = hipMemsetAsync(st.unique, 0, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(st.blob, 0, 16, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(PV_EIO, "state store allocation failed: %s", hipGetErrorString(e));
  }
  if (rc) {
    g_stores.release(st);
    return rc;
  }
  *store_out = id;
  return PV_OK;
}

int pv_state_store_free(int32_t store) { return g_stores.free(store); }

int pv_state_store_add(int32_t store, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new,
                       uint8_t* digests, uint64_t* n_added) {
  return store_add(store, node_blob, node_off, n_new, digests, n_added, true, nullptr);
}

int pv_state_store_add_device(int32_t store, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new,
                              uint8_t* digests, void* stream) {
  return store_add(store, node_blob, node_off, n_new, digests, nullptr, false, stream);
}

int pv_state_store_info(int32_t store, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes, uint64_t* n_slots) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_nodes) *n_nodes = st->n_nodes;
  if (n_unique) *n_unique = st->n_unique;
  if (n_bytes) *n_bytes = st->n_bytes;
  if (n_slots) *n_slots = st->slots;
  return PV_OK;
}

int pv_state_store_walk_device(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                               const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries,
                               uint32_t max_nodes, uint8_t* status, uint32_t* node_count, uint32_t* node_ids,
                               uint64_t* proof_len, uint64_t* val_rel, uint64_t* val_len, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_blob || !key_off || !status || !node_count || !node_ids || !proof_len || !val_rel || !val_len)
    return fail(PV_EINVAL, "null device buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40) / max_nodes) return fail(PV_EINVAL, "n_queries x max_nodes above 2^40 node ids");
  if (reinterpret_cast<uintptr_t>(roots) & 3u) return fail(PV_EINVAL, "roots must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_trie_prove(st->blob, st->beg, st->end, st->dig, st->table, st->slots, (uint32_t)st->n_nodes,
                               w32(roots), root_idx, n_roots, key_blob, key_off, n_queries, max_nodes, status,
                               node_count, node_ids, proof_len, val_rel, val_len, merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_state_store_pack_device(int32_t store, const uint32_t* node_ids, const uint32_t* node_count,
                               uint32_t max_nodes, const uint64_t* proof_off, uint64_t n_queries,
                               uint8_t* proof_blob, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!node_ids || !node_count || !proof_off || !proof_blob) return fail(PV_EINVAL, "null device buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_trie_proof_pack(st->blob, st->beg, st->end, (uint32_t)st->n_nodes, node_ids, node_count,
                                    max_nodes, proof_off, n_queries, proof_blob, merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_state_store_prove(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                         const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, uint32_t max_nodes,
                         uint8_t* status, uint32_t* node_count, uint64_t* proof_off, uint64_t* val_rel,
                         uint64_t* val_len, uint8_t* proof_blob, uint64_t proof_cap) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_off || !status || !node_count || !proof_off || !val_rel || !val_len)
    return fail(PV_EINVAL, "null buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40) / max_nodes) return fail(PV_EINVAL, "n_queries x max_nodes above 2^40 node ids");
  if (!root_idx && n_roots < n_queries)
    return fail(PV_EINVAL, "%llu roots for %llu queries without root_idx", (unsigned long long)n_roots,
                (unsigned long long)n_queries);
  Ragged keys(key_off, n_queries);
  if (const int rc = keys.check("key_off")) return rc;
  if (keys.len && !key_blob) return fail(PV_EINVAL, "null buffer");
  if (root_idx)
    for (uint64_t i = 0; i < n_queries; ++i)
      if (root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "root_idx[%llu] = %u is not below n_roots %llu", (unsigned long long)i, root_idx[i],
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> droots, dkeys, dstatus, dproof;
  TmpBuf<uint32_t> dridx, dcount, dids;
  TmpBuf<uint64_t> dkoff, dlen, dvrel, dvlen, dpoff;
  StreamDrain tail{s};
  HIP_OK(droots.put(roots, n_roots * 32, s));
  if (root_idx) HIP_OK(dridx.put(root_idx, n_queries, s));
  HIP_OK(dkeys.alloc(keys.len + 4));
  if (keys.len) HIP_OK(hipMemcpyAsync(dkeys.p, key_blob + keys.b0, keys.len, hipMemcpyHostToDevice, s));
  HIP_OK(dkoff.put(keys.rebased(), n_queries + 1, s));
  HIP_OK(dstatus.alloc(n_queries));
  HIP_OK(dcount.alloc(n_queries));
  HIP_OK(dids.alloc(n_queries * max_nodes));
  HIP_OK(dlen.alloc(n_queries));
  HIP_OK(dvrel.alloc(n_queries));
  HIP_OK(dvlen.alloc(n_queries));
  HIP_OK(pv::launch_trie_prove(st->blob, st->beg, st->end, st->dig, st->table, st->slots, (uint32_t)st->n_nodes,
                               w32(droots.p), root_idx ? dridx.p : nullptr, n_roots, dkeys.p, dkoff.p, n_queries,
                               max_nodes, dstatus.p, dcount.p, dids.p, dlen.p, dvrel.p, dvlen.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n_queries, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(node_count, dcount.p, n_queries * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(proof_off + 1, dlen.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(val_rel, dvrel.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(val_len, dvlen.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  proof_off[0] = 0;   // the lengths, scanned in place
  for (uint64_t i = 0; i < n_queries; ++i) proof_off[i + 1] += proof_off[i];
  const uint64_t total = proof_off[n_queries];
  if (!proof_blob) return tail.finish();   // the sizing call
  if (proof_cap < total)
    return fail(PV_EINVAL, "proof_cap %llu is below the %llu bytes of the proofs", (unsigned long long)proof_cap,
                (unsigned long long)total);
  if (total == 0) return tail.finish();
  HIP_OK(dpoff.put(proof_off, n_queries + 1, s));
  HIP_OK(dproof.alloc(total));
  HIP_OK(pv::launch_trie_proof_pack(st->blob, st->beg, st->end, (uint32_t)st->n_nodes, dids.p, dcount.p, max_nodes,
                                    dpoff.p, n_queries, dproof.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(proof_blob, dproof.p, total, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

}  // extern "C"

namespace {

// the buffers a prune builds beside the store's own: freed unless the swap took them
struct FreshStore {
  uint8_t* blob = nullptr;
  uint64_t *beg = nullptr, *end = nullptr;
  uint32_t *dig = nullptr, *table = nullptr;
  uint8_t* dup = nullptr;
  unsigned int* unique = nullptr;
  bool taken = false;
  ~FreshStore() {
    if (taken) return;
    void* bufs[] = {blob, beg, end, dig, table, dup, unique};
    for (void* p : bufs)
      if (p) (void)hipFree(p);
  }
};

template <typename T>
hipError_t fresh_alloc(T** p, uint64_t n) {
  return hipMalloc(reinterpret_cast<void**>(p), (size_t)n * sizeof(T));
}

// pv_state_store_prune; phase_ms (NULL, or 3 floats: mark, scans + copy, rehash of an applied prune)
int prune_impl(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, int apply, uint8_t* root_status,
               uint64_t* n_kept, uint64_t* bytes_kept, uint64_t* n_missing, uint8_t* kept_digests,
               uint64_t digest_cap, float* phase_ms) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_roots == 0) return fail(PV_EINVAL, "no root to keep (free the store instead)");
  if (!keep_roots) return fail(PV_EINVAL, "null buffer");
  if (n_roots > (1ull << 31)) return fail(PV_EINVAL, "more than 2^31 roots to keep");
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  const int mb = merkle_blocks(d);
  const uint64_t n = st->n_nodes, words = (n + 31) / 32;
  TmpBuf<uint8_t> droots, dstatus;
  TmpBuf<uint32_t> bits, queue, ddig;
  TmpBuf<unsigned long long> counts;
  TmpBuf<uint64_t> keep, len;
  FreshStore f;
  PhaseEvents ph;
  StreamDrain tail{s};
  if (phase_ms) HIP_OK(ph.create());
  HIP_OK(ph.mark(0, s));
  // mark: the roots, then one launch per level until a level appends nothing
  HIP_OK(droots.put(keep_roots, n_roots * 32, s));
  HIP_OK(dstatus.alloc(n_roots));
  HIP_OK(bits.alloc(words));
  if (words) HIP_OK(hipMemsetAsync(bits.p, 0, words * 4, s));
  HIP_OK(queue.alloc(st->n_unique));   // an id is enqueued by the lane that flipped its bit: at most once
  HIP_OK(counts.alloc(pv::TP_COUNTS));
  HIP_OK(hipMemsetAsync(counts.p, 0, pv::TP_COUNTS * 8, s));
  const pv::TpCtx c{st->blob, st->beg,  st->end, st->dig,  st->table, st->slots,
                    (uint32_t)n, bits.p, queue.p, counts.p};
  HIP_OK(pv::launch_trie_prune_seed(c, w32(droots.p), n_roots, dstatus.p, mb, s));
  unsigned long long hc[pv::TP_COUNTS] = {0, 0, 0};
  for (uint64_t head = 0;;) {
    HIP_OK(hipMemcpyAsync(hc, counts.p, sizeof hc, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (hc[pv::TP_TAIL] > st->n_unique) return fail(PV_EIO, "state prune: the mark queue overran the store");
    if (hc[pv::TP_TAIL] == head) break;   // each level marks at least one new node, or ends the loop
    HIP_OK(pv::launch_trie_prune_level(c, head, hc[pv::TP_TAIL], mb, s));
    head = hc[pv::TP_TAIL];
  }
  const uint64_t kept = hc[pv::TP_TAIL];
  HIP_OK(ph.mark(1, s));
  std::vector<uint8_t> hstat(n_roots);
  HIP_OK(hipMemcpyAsync(hstat.data(), dstatus.p, n_roots, hipMemcpyDeviceToHost, s));
  // new ids and new byte offsets: two exclusive scans over the keep flags and the kept lengths
  HIP_OK(keep.alloc(n + 1));
  HIP_OK(len.alloc(n + 1));
  HIP_OK(pv::launch_trie_prune_flags(bits.p, st->beg, st->end, n, keep.p, len.p, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(n + 1)));
  HIP_OK(pv::launch_exclusive_scan(keep.p, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(len.p, n + 1, d.scan.p, s));
  uint64_t bytes = 0;
  HIP_OK(hipMemcpyAsync(&bytes, len.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (root_status) memcpy(root_status, hstat.data(), n_roots);
  if (hc[pv::TP_OVERFLOW])
    return fail(PV_EINVAL, "state prune: inline nodes nest more than %d deep under a stored node", pv::TP_MAX_INLINE);
  if (n_kept) *n_kept = kept;
  if (bytes_kept) *bytes_kept = bytes;
  if (n_missing) *n_missing = hc[pv::TP_MISSING];
  if (apply)
    for (uint64_t i = 0; i < n_roots; ++i)
      if (hstat[i] != PV_SP_OK)
        return fail(PV_EINVAL, "state prune: keep root %llu is not in the store", (unsigned long long)i);
  if (kept_digests && digest_cap < kept)
    return fail(PV_EINVAL, "digest capacity too small: %llu entries for %llu kept nodes",
                (unsigned long long)digest_cap, (unsigned long long)kept);
  if (!apply) {   // the reporting call: the store stays as it is
    if (kept_digests && kept) {
      HIP_OK(ddig.alloc(kept * 8));
      HIP_OK(pv::launch_trie_prune_copy(st->blob, st->beg, st->end, st->dig, bits.p, keep.p, len.p, n, nullptr,
                                        nullptr, nullptr, ddig.p, mb, s));
      HIP_OK(hipMemcpyAsync(kept_digests, ddig.p, kept * 32, hipMemcpyDeviceToHost, s));
    }
    return tail.finish();
  }
  // compact into fresh buffers beside the old ones; the swap is the last step
  const uint64_t cap_nodes = pv::tp_pow2(kept, 1), cap_bytes = pv::tp_pow2(bytes, 1);
  const uint64_t slots = pv::tp_pow2(2 * kept, pv::TS_MIN_SLOTS);   // kept <= n_unique <= 2^30
  HIP_OK(fresh_alloc(&f.blob, cap_bytes + 16));
  HIP_OK(fresh_alloc(&f.beg, cap_nodes));
  HIP_OK(fresh_alloc(&f.end, cap_nodes));
  HIP_OK(fresh_alloc(&f.dig, cap_nodes * 8));
  HIP_OK(fresh_alloc(&f.dup, cap_nodes));
  HIP_OK(fresh_alloc(&f.table, slots));
  HIP_OK(fresh_alloc(&f.unique, 1));
  HIP_OK(pv::launch_trie_prune_copy(st->blob, st->beg, st->end, st->dig, bits.p, keep.p, len.p, n, f.blob, f.beg,
                                    f.end, f.dig, mb, s));
  HIP_OK(hipMemsetAsync(f.blob + bytes, 0, 16, s));
  HIP_OK(ph.mark(2, s));
  HIP_OK(hipMemsetAsync(f.dup, 0, cap_nodes, s));
  HIP_OK(hipMemsetAsync(f.table, 0, slots * 4, s));
  HIP_OK(pv::launch_trie_store_rehash(f.table, (uint32_t)slots, f.dig, f.dup, (uint32_t)kept, mb, s));
  HIP_OK(ph.mark(3, s));
  if (kept_digests && kept) HIP_OK(hipMemcpyAsync(kept_digests, f.dig, kept * 32, hipMemcpyDeviceToHost, s));
  const unsigned int uniq = (unsigned int)kept;
  HIP_OK(hipMemcpyAsync(f.unique, &uniq, 4, hipMemcpyHostToDevice, s));
  if (const int rc = tail.finish()) return rc;
  if (phase_ms)
    for (int i = 0; i < 3; ++i) HIP_OK(hipEventElapsedTime(phase_ms + i, ph.ev[i], ph.ev[i + 1]));
  void* old[] = {st->blob, st->beg, st->end, st->dig, st->dup, st->table, st->unique};
  for (void* p : old)
    if (p) (void)hipFree(p);
  f.taken = true;
  st->blob = f.blob;
  st->beg = f.beg;
  st->end = f.end;
  st->dig = f.dig;
  st->dup = f.dup;
  st->table = f.table;
  st->unique = f.unique;
  st->cap_bytes = cap_bytes;
  st->cap_nodes = cap_nodes;
  st->slots = (uint32_t)slots;
  st->n_nodes = st->n_unique = kept;
  st->n_bytes = bytes;
  return PV_OK;
}

}  // namespace

extern "C" {

int pv_state_store_prune(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, int apply, uint8_t* root_status,
                         uint64_t* n_kept, uint64_t* bytes_kept, uint64_t* n_missing, uint8_t* kept_digests,
                         uint64_t digest_cap) {
  return prune_impl(store, keep_roots, n_roots, apply, root_status, n_kept, bytes_kept, n_missing, kept_digests,
                    digest_cap, nullptr);
}

int pv_time_state_store_prune(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, uint64_t* n_kept,
                              uint64_t* bytes_kept, float* ms_mark, float* ms_compact, float* ms_rehash) {
  if (!ms_mark || !ms_compact || !ms_rehash) return fail(PV_EINVAL, "null pointer");
  float ms[3] = {0, 0, 0};
  const int rc = prune_impl(store, keep_roots, n_roots, 1, nullptr, n_kept, bytes_kept, nullptr, nullptr, 0, ms);
  *ms_mark = ms[0];
  *ms_compact = ms[1];
  *ms_rehash = ms[2];
  return rc;
}

}  // extern "C"
