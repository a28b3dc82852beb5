// The state-trie part of include/plenum_verify.h: pv_state_sort_device,
// pv_state_build*, pv_state_update* and pv_state_apply* (the host sort, the
// device sort, the build, sets and removals onto a committed root), and
// pv_state_store_get* (reads at a root).
#include "pv_api_common.h"
#include "pv_trie_store.h"
#include "pv_trie_get.h"
#include "pv_trie_build.h"
#include "pv_trie_update.h"
#include "pv_trie_sort.h"

using namespace pvapi;

// ------------------------------------------------------- batch trie build
namespace {

// The tail of an add for nodes whose digests are known (pv_state_build with a
// store): copy, k_trie_store_layout, the digests copied instead of a second
// k_sha3_256, then k_trie_store_insert / k_trie_store_rehash as store_add.
// blob / off (off[0] = 0, off[n_new] = total) / dig are device memory.
int store_add_hashed(StateStore& st, Device& d, hipStream_t s, const uint8_t* blob, const uint64_t* off,
                     const uint32_t* dig, uint64_t n_new, uint64_t total) {
  if (n_new == 0) return PV_OK;
  const uint64_t nodes = st.n_nodes + n_new;
  if (const int rc = store_reserve(st, nodes, st.n_bytes + total, s)) return rc;
  if (total) HIP_OK(hipMemcpyAsync(st.blob + st.n_bytes, blob, total, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(st.blob + st.n_bytes + total, 0, 16, s));
  HIP_OK(hipMemsetAsync(st.dup + st.n_nodes, 0, n_new, s));
  HIP_OK(pv::launch_trie_store_layout(off, n_new, st.n_bytes, total, st.beg, st.end, st.n_nodes, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(st.dig + 8 * st.n_nodes, dig, n_new * 32, hipMemcpyDeviceToDevice, s));
  if (nodes > st.slots / 2) {
    uint64_t ns = st.slots;
    while (nodes > ns / 2) ns *= 2;
    if (ns > (1ull << 31)) return fail(PV_ENOMEM, "state store table above 2^31 slots");
    if (const int rc = store_rehash(st, (uint32_t)ns, d, s)) return rc;
  }
  HIP_OK(pv::launch_trie_store_insert(st.table, st.slots, st.dig, st.dup, (uint32_t)st.n_nodes, (uint32_t)n_new,
                                      st.unique, merkle_blocks(d), s));
  unsigned int uniq = 0;
  HIP_OK(hipMemcpyAsync(&uniq, st.unique, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  st.n_unique = uniq;
  st.n_nodes = nodes;
  st.n_bytes += total;
  return PV_OK;
}

// what k_trie_build_lcp refused: hs[1 .. 3] = the first index for order / value / offsets
int lcp_refusal(const uint32_t* hs) {
  if (hs[3] != 0xffffffffu)
    return fail(PV_EINVAL, "key_off or val_off decreases, or a key is above 2^20 bytes, at index %u", hs[3]);
  if (hs[2] != 0xffffffffu) return fail(PV_EINVAL, "value %u is empty or above 2^30 bytes", hs[2]);
  if (hs[1] != 0xffffffffu)
    return fail(PV_EINVAL, "keys not strictly increasing at index %u (key %u is not above key %u)", hs[1], hs[1],
                hs[1] - 1);
  return PV_OK;
}

// The build over device keys and values (sorted, distinct).  root, n_nodes and
// n_bytes are host memory; node_blob / node_off / digests are host memory with
// host_out, else device memory; st: the store that takes the nodes, or null.
int build_core(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb, const uint64_t* vo,
               uint64_t n, StateStore* st, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
               uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests, bool host_out,
               const uint32_t* knib = nullptr, const uint8_t* kind = nullptr) {
  const hipMemcpyKind out_kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (n == 0) return PV_OK;   // the entry points return before this
  uint64_t lvoff[pv::TB_MAX_LEVELS + 1];
  pv::TbCtx c{};
  c.key_blob = kb;
  c.key_off = ko;
  c.val_blob = vb;
  c.val_off = vo;
  c.n = n;
  c.knib = knib;   // a merged item list (update_core), else null
  c.kind = kind;
  c.nlv = pv::tb_tree_layout(n, lvoff);
  const uint64_t ents = 3 * n;
  TmpBuf<uint32_t> tree, child, lvl, aux, elen, stats, odig;
  TmpBuf<uint64_t> dlvoff, off, idx, ooff;
  TmpBuf<uint8_t> inl, oblob;
  StreamDrain tail{s};
  HIP_OK(tree.alloc(lvoff[c.nlv]));
  HIP_OK(dlvoff.put(lvoff, pv::TB_MAX_LEVELS + 1, s));
  HIP_OK(child.alloc(16 * n));
  HIP_OK(lvl.alloc(ents));
  HIP_OK(aux.alloc(ents));
  HIP_OK(elen.alloc(ents));
  HIP_OK(off.alloc(ents + 1));
  HIP_OK(idx.alloc(ents + 1));
  HIP_OK(inl.alloc(32 * ents));
  uint32_t hs[5] = {0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0};   // max h, three first-bad indices, the root's entity
  HIP_OK(stats.put(hs, 5, s));
  HIP_OK(hipMemsetAsync(child.p, 0, 16 * n * 4, s));
  HIP_OK(hipMemsetAsync(off.p, 0, (ents + 1) * 8, s));
  HIP_OK(hipMemsetAsync(idx.p, 0, (ents + 1) * 8, s));
  c.tree = tree.p;
  c.lvoff = dlvoff.p;
  c.child = child.p;
  c.lvl = lvl.p;
  c.aux = aux.p;
  c.elen = elen.p;
  c.off = off.p;
  c.idx = idx.p;
  c.inl = inl.p;
  c.root_e = stats.p + 4;
  const int mb = merkle_blocks(d);
  HIP_OK(pv::launch_trie_build_lcp(c, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 16, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (knib && (hs[1] & hs[2] & hs[3]) != 0xffffffffu)
    return fail(PV_EIO, "trie update: the merged list is not one a build takes (item %u)",
                hs[3] < hs[2] ? (hs[3] < hs[1] ? hs[3] : hs[1]) : (hs[2] < hs[1] ? hs[2] : hs[1]));
  if (const int rc = lcp_refusal(hs)) return rc;
  const uint32_t maxh = hs[0];
  for (uint32_t lv = 1; lv < c.nlv; ++lv) HIP_OK(pv::launch_trie_build_min(c, lv, lvoff[lv + 1] - lvoff[lv], mb, s));
  HIP_OK(pv::launch_trie_build_struct(c, stats.p + 4, mb, s));
  for (uint32_t lv = maxh + 1; lv-- > 0;) HIP_OK(pv::launch_trie_build_size(c, lv, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(ents + 1)));
  HIP_OK(pv::launch_exclusive_scan(off.p, ents + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(idx.p, ents + 1, d.scan.p, s));
  uint64_t total = 0, nodes = 0, root_id = 0;
  uint32_t root_e = 0;
  HIP_OK(hipMemcpyAsync(&total, off.p + ents, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&nodes, idx.p + ents, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&root_e, stats.p + 4, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (root_e >= ents || nodes == 0 || nodes > ents) return fail(PV_EIO, "trie build: inconsistent structure pass");
  HIP_OK(hipMemcpyAsync(&root_id, idx.p + root_e, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (n_nodes) *n_nodes = nodes;
  if (n_bytes) *n_bytes = total;
  if ((node_blob && blob_cap < total) || ((node_off || digests) && node_cap < nodes))
    return fail(PV_EINVAL, "node capacity too small: the build has %llu nodes of %llu bytes", (unsigned long long)nodes,
                (unsigned long long)total);
  if (st && (nodes > pv::TS_MAX_NODES || st->n_nodes + nodes > pv::TS_MAX_NODES))
    return fail(PV_EINVAL, "state store limited to 2^32 - 2 nodes");
  HIP_OK(oblob.alloc(total + 16));
  HIP_OK(ooff.alloc(nodes + 1));
  HIP_OK(odig.alloc(8 * nodes));
  HIP_OK(hipMemsetAsync(oblob.p + total, 0, 16, s));
  c.out_blob = oblob.p;
  c.node_off = ooff.p;
  c.dig = odig.p;
  for (uint32_t lv = maxh + 1; lv-- > 0;) HIP_OK(pv::launch_trie_build_emit(c, lv, mb, s));
  HIP_OK(hipMemcpyAsync(ooff.p + nodes, off.p + ents, 8, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(root, odig.p + 8 * root_id, 32, hipMemcpyDeviceToHost, s));
  if (node_blob && total) HIP_OK(hipMemcpyAsync(node_blob, oblob.p, total, out_kind, s));
  if (node_off) HIP_OK(hipMemcpyAsync(node_off, ooff.p, (nodes + 1) * 8, out_kind, s));
  if (digests) HIP_OK(hipMemcpyAsync(digests, odig.p, nodes * 32, out_kind, s));
  if (st)
    if (const int rc = store_add_hashed(*st, d, s, oblob.p, ooff.p, odig.p, nodes, total)) return rc;
  return tail.finish();
}

const uint8_t kBlankRoot[32] = {0xbc, 0x20, 0x71, 0xa4, 0xde, 0x84, 0x6f, 0x28, 0x57, 0x02, 0x44,
                                0x7f, 0x25, 0x89, 0xdd, 0x16, 0x36, 0x78, 0xe0, 0x97, 0x2a, 0x8a,
                                0x1b, 0x0d, 0x28, 0xb0, 0x4e, 0xd5, 0xc0, 0x94, 0x54, 0x7f};   // SHA3-256(0x80)

// The empty batch: the blank root, no nodes.  Every output that is given is
// written; nothing is launched for the build and nothing is inserted, so the
// store is not looked at.
int build_empty(Entry& en, void* stream, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint64_t* node_off,
                bool host_out) {
  if (root) memcpy(root, kBlankRoot, 32);
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (!node_off) return PV_OK;
  if (host_out) {
    node_off[0] = 0;
    return PV_OK;
  }
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(hipMemsetAsync(node_off, 0, 8, en.s));
  return en.finish();
}

// key a before key b: bytewise, a proper prefix first
bool key_less(const uint8_t* blob, const uint64_t* off, uint64_t a, uint64_t b, bool* equal) {
  const uint64_t la = off[a + 1] - off[a], lb = off[b + 1] - off[b];
  const uint64_t m = la < lb ? la : lb;
  const int c = m ? memcmp(blob + off[a], blob + off[b], m) : 0;
  *equal = c == 0 && la == lb;
  return c < 0 || (c == 0 && la < lb);
}

// The host forms' input: the checks of the arrays, then the pairs sorted with
// the last of equal keys kept, as blobs with 16 spare bytes and offsets from 0.
int sorted_pairs(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                 uint64_t n, std::vector<uint64_t>& ko, std::vector<uint64_t>& vo, std::vector<uint8_t>& kb,
                 std::vector<uint8_t>& vb, bool empty_ok = false) {
  if (!key_off || !val_off || (!val_blob && !empty_ok)) return fail(PV_EINVAL, "null buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  Ragged keys(key_off, n), vals(val_off, n);
  if (const int rc = keys.check("key_off")) return rc;
  if (const int rc = vals.check("val_off")) return rc;
  if ((keys.len && !key_blob) || (vals.len && !val_blob))   // a batch of removals alone has no value byte
    return fail(PV_EINVAL, "null buffer");
  for (uint64_t i = 0; i < n; ++i) {
    if (val_off[i + 1] == val_off[i] && !empty_ok)   // pv_state_apply: a removal
      return fail(PV_EINVAL, "value %llu is empty", (unsigned long long)i);
    if (key_off[i + 1] - key_off[i] > pv::TB_MAX_KEY_BYTES || val_off[i + 1] - val_off[i] > pv::TB_MAX_VAL_BYTES)
      return fail(PV_EINVAL, "pair %llu: a key above 2^20 or a value above 2^30 bytes", (unsigned long long)i);
  }
  // sorted index; of equal keys the last occurrence stays
  std::vector<uint64_t> order(n), pick;
  for (uint64_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    bool eq;
    return key_less(key_blob, key_off, a, b, &eq);
  });
  for (uint64_t k = 0; k < n; ++k) {
    bool eq = false;
    if (k + 1 < n) (void)key_less(key_blob, key_off, order[k], order[k + 1], &eq);
    if (!eq) pick.push_back(order[k]);
  }
  const uint64_t m = pick.size();
  ko.assign(m + 1, 0);
  vo.assign(m + 1, 0);
  for (uint64_t k = 0; k < m; ++k) {
    ko[k + 1] = ko[k] + (key_off[pick[k] + 1] - key_off[pick[k]]);
    vo[k + 1] = vo[k] + (val_off[pick[k] + 1] - val_off[pick[k]]);
  }
  kb.assign(ko[m] + 16, 0);
  vb.assign(vo[m] + 16, 0);
  for (uint64_t k = 0; k < m; ++k) {
    if (ko[k + 1] > ko[k]) memcpy(&kb[ko[k]], key_blob + key_off[pick[k]], ko[k + 1] - ko[k]);
    if (vo[k + 1] > vo[k]) memcpy(&vb[vo[k]], val_blob + val_off[pick[k]], vo[k + 1] - vo[k]);
  }
  return PV_OK;
}

// ------------------------------------------- the device sort (pv_trie_sort.h)
// what k_trie_sort_init refused: hs[0 .. 2] = the first input index for offsets / key length / value
int sort_refusal(const uint32_t* hs) {
  if (hs[0] != 0xffffffffu) return fail(PV_EINVAL, "key_off or val_off decreases at index %u", hs[0]);
  if (hs[1] != 0xffffffffu)
    return fail(PV_EINVAL,
                "key %u is above 1024 bytes: the device sort takes keys up to 1024 bytes, the host forms "
                "(pv_state_build, pv_state_update, pv_state_apply) sort keys of any length",
                hs[1]);
  if (hs[2] != 0xffffffffu) return fail(PV_EINVAL, "value %u is empty or above 2^30 bytes", hs[2]);
  return PV_OK;
}

// perm[0 .. *kept) = the input indices of the distinct keys in order, the last of equal keys kept
// (device memory, n entries); val_off: checked with the keys when given (the fused forms).  Nothing
// is written to perm when the first kernel refuses.  *rounds: the rounds run.  Ends synchronised.
int sort_core(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint64_t* vo, bool empty_ok,
              uint64_t n, uint32_t* perm, uint64_t* kept, uint32_t* rounds = nullptr) {
  const int mb = merkle_blocks(d);
  const uint64_t table_words = 256 * pv::trie_sort_blocks(n);
  TmpBuf<pv::TsRec> ra, rb;
  TmpBuf<uint64_t> x, table;
  TmpBuf<uint32_t> stats;
  StreamDrain tail{s};
  HIP_OK(ra.alloc(n));
  HIP_OK(rb.alloc(n));
  HIP_OK(x.alloc(n + 1));
  HIP_OK(table.alloc(table_words));
  uint32_t hs[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
  HIP_OK(stats.put(hs, 3, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(table_words > n + 1 ? table_words : n + 1)));
  HIP_OK(pv::launch_trie_sort_init(kb, ko, vo, empty_ok, n, ra.p, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 12, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (const int rc = sort_refusal(hs)) return rc;
  pv::TsRec *cur = ra.p, *other = rb.p;
  uint64_t runs = 1;
  uint32_t r = 0;
  for (;; ++r) {
    if (r >= pv::TS_MAX_ROUNDS) return fail(PV_EIO, "device sort: keys unresolved after %u rounds", r);
    if (r > 0) {   // the segment of round r is the run's rank after round r - 1
      HIP_OK(pv::launch_trie_sort_round(kb, ko, cur, x.p, n, r, other, mb, s));
      std::swap(cur, other);
    }
    const uint32_t passes = 9 + (r > 0 ? pv::ts_seg_digits(runs) : 0);
    for (uint32_t p = 0; p < passes; ++p) {
      HIP_OK(pv::launch_trie_sort_pass(cur, n, p, table.p, d.scan.p, other, s));
      std::swap(cur, other);
    }
    HIP_OK(pv::launch_trie_sort_flags(cur, n, x.p, mb, s));
    HIP_OK(pv::launch_exclusive_scan(x.p, n + 1, d.scan.p, s));
    uint64_t totals = 0;   // unresolved << 32 | runs
    HIP_OK(hipMemcpyAsync(&totals, x.p + n, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    runs = totals & 0xffffffffull;
    if (runs == 0 || runs > n) return fail(PV_EIO, "device sort: inconsistent flag pass");
    if ((totals >> 32) == 0) break;
  }
  HIP_OK(pv::launch_trie_sort_finish(cur, x.p, n, perm, mb, s));
  *kept = runs;
  if (rounds) *rounds = r + 1;
  return tail.finish();
}

// The fused forms' input: device pairs in any order -> the pairs sorted with the last of equal
// keys kept, as blobs with 16 spare bytes and offsets from 0 (what sorted_pairs gives the host forms).
struct DevicePairs {
  TmpBuf<uint8_t> kb, vb;
  TmpBuf<uint64_t> ko, vo;
  uint64_t m = 0;
};

int sort_pairs_device(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb,
                      const uint64_t* vo, uint64_t n, bool empty_ok, DevicePairs& out, uint32_t* rounds = nullptr,
                      hipEvent_t sorted = nullptr) {
  const int mb = merkle_blocks(d);
  TmpBuf<uint32_t> perm;
  StreamDrain tail{s};
  HIP_OK(perm.alloc(n));
  if (const int rc = sort_core(d, s, kb, ko, vo, empty_ok, n, perm.p, &out.m, rounds)) return rc;
  if (sorted) HIP_OK(hipEventRecord(sorted, s));   // pv_time_state_sort_device: the sort ends, the gather begins
  const uint64_t m = out.m;
  HIP_OK(out.ko.alloc(m + 1));
  HIP_OK(out.vo.alloc(m + 1));
  HIP_OK(pv::launch_trie_sort_lens(perm.p, m, n, ko, vo, out.ko.p, out.vo.p, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(m + 1)));
  HIP_OK(pv::launch_exclusive_scan(out.ko.p, m + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(out.vo.p, m + 1, d.scan.p, s));
  uint64_t kbytes = 0, vbytes = 0;
  HIP_OK(hipMemcpyAsync(&kbytes, out.ko.p + m, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&vbytes, out.vo.p + m, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(out.kb.alloc(kbytes + 16));
  HIP_OK(out.vb.alloc(vbytes + 16));
  HIP_OK(hipMemsetAsync(out.kb.p + kbytes, 0, 16, s));
  HIP_OK(hipMemsetAsync(out.vb.p + vbytes, 0, 16, s));
  HIP_OK(pv::launch_trie_sort_copy(perm.p, m, n, kb, ko, vb, vo, out.ko.p, out.vo.p, out.kb.p, out.vb.p, mb, s));
  return tail.finish();
}

// The build's first kernel checks the order again.  After the device sort that refusal is a bug
// in the sort, not in the caller's input: it is reported as one, and nothing is retried.
int sort_selfcheck(int rc) {
  if (rc == PV_EINVAL && last_error().compare(0, 28, "keys not strictly increasing") == 0) {
    const std::string was = last_error();
    return fail(PV_EIO, "device sort: a bug in the sort, its output was refused by the build (%s)", was.c_str());
  }
  return rc;
}

}  // namespace

extern "C" {

// The permutation that sorts state keys: bytewise, a proper prefix first, the last of equal keys
// kept (csrc/pv_trie_sort.h); see include/plenum_verify.h.
int pv_state_sort_device(const uint8_t* key_blob, const uint64_t* key_off, uint64_t n, uint32_t* perm,
                         uint64_t* n_kept, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) {
    if (n_kept) *n_kept = 0;
    return PV_OK;
  }
  if (!n_kept) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !perm) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if (reinterpret_cast<uintptr_t>(key_blob) & 3u) return fail(PV_EINVAL, "key_blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  *n_kept = 0;
  return sort_core(*en.d, en.s, key_blob, key_off, nullptr, true, n, perm, n_kept);
}

// pv_state_build_device over pairs in any order, the last of equal keys winning: the device sort,
// the gather, then the same build; see include/plenum_verify.h.
int pv_state_build_unsorted_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                                   const uint64_t* val_off, uint64_t n, int32_t store, uint8_t* root,
                                   uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap,
                                   uint64_t* node_off, uint64_t node_cap, uint8_t* digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return build_empty(en, stream, root, n_nodes, n_bytes, node_off, false);
  if (!root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  StateStore* st = nullptr;
  if (store != -1) {
    st = find_store(store);
    if (!st) return fail(PV_EINVAL, "no state store with id %d", (int)store);
    if (st->dev != en.d->id)
      return fail(PV_EINVAL, "state store %d lives on device %d, not on device %d", (int)store, st->dev, device);
  }
  if (const int rc = en.begin(stream)) return rc;
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  DevicePairs sp;
  StreamDrain tail{en.s};
  if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, false, sp)) return rc;
  return sort_selfcheck(build_core(*en.d, en.s, sp.kb.p, sp.ko.p, sp.vb.p, sp.vo.p, sp.m, st, root, n_nodes, n_bytes,
                                   node_blob, blob_cap, node_off, node_cap, digests, false));
}

// The sort and the gather of the fused forms alone, each timed with HIP events on the call's
// stream (tools/bench_state_sort.py); see include/plenum_verify.h.
int pv_time_state_sort_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                              const uint64_t* val_off, uint64_t n, int device, void* stream, uint64_t* n_kept,
                              uint32_t* rounds, float* ms_sort, float* ms_gather) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!n_kept || !rounds || !ms_sort || !ms_gather) return n == 0 ? PV_OK : fail(PV_EINVAL, "null pointer");
  *n_kept = 0;
  *rounds = 0;
  *ms_sort = *ms_gather = 0;
  if (n == 0) return PV_OK;
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  PhaseEvents ev;
  HIP_OK(ev.create());
  DevicePairs sp;
  StreamDrain tail{en.s};
  HIP_OK(ev.mark(0, en.s));
  if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, true, sp, rounds, ev.ev[1]))
    return rc;
  HIP_OK(ev.mark(2, en.s));
  HIP_OK(hipEventSynchronize(ev.ev[2]));
  HIP_OK(hipEventElapsedTime(ms_sort, ev.ev[0], ev.ev[1]));
  HIP_OK(hipEventElapsedTime(ms_gather, ev.ev[1], ev.ev[2]));
  *n_kept = sp.m;
  return tail.finish();
}

// PruningState.set per pair and headHash (state/pruning_state.py:60-61, 136; Trie.update,
// state/trie/pruning_trie.py:1006-1027) as one batch; see include/plenum_verify.h.
int pv_state_build_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                          const uint64_t* val_off, uint64_t n, int32_t store, uint8_t* root, uint64_t* n_nodes,
                          uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                          uint64_t node_cap, uint8_t* digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return build_empty(en, stream, root, n_nodes, n_bytes, node_off, false);
  if (!root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  StateStore* st = nullptr;
  if (store != -1) {
    st = find_store(store);
    if (!st) return fail(PV_EINVAL, "no state store with id %d", (int)store);
    if (st->dev != en.d->id)
      return fail(PV_EINVAL, "state store %d lives on device %d, not on device %d", (int)store, st->dev, device);
  }
  if (const int rc = en.begin(stream)) return rc;
  return build_core(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, st, root, n_nodes, n_bytes, node_blob,
                    blob_cap, node_off, node_cap, digests, false);
}

// The host form of the same (state/pruning_state.py:60-61; state/trie/pruning_trie.py:1006-1027):
// keys in any order, the last of equal keys wins, as a sequence of sets gives.
int pv_state_build(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                   uint64_t n, int32_t store, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
                   uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests) {
  if (n == 0) {
    Entry en;
    if (const int rc = en.check()) return rc;
    return build_empty(en, nullptr, root, n_nodes, n_bytes, node_off, true);
  }
  // The argument checks and the sorted copy touch no library state: they run
  // before the library lock is taken, so a large sort blocks no other call.
  if (!root) return fail(PV_EINVAL, "null pointer");
  std::vector<uint64_t> ko, vo;
  std::vector<uint8_t> kb, vb;
  if (const int rc = sorted_pairs(key_blob, key_off, val_blob, val_off, n, ko, vo, kb, vb)) return rc;
  const uint64_t m = ko.size() - 1;
  Entry en;
  if (const int rc = en.check()) return rc;
  StateStore* st = nullptr;
  if (store != -1)
    if (const int rc = store_enter(en, store, &st)) return rc;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(kb.data(), kb.size(), s));
  HIP_OK(dvb.put(vb.data(), vb.size(), s));
  HIP_OK(dko.put(ko.data(), m + 1, s));
  HIP_OK(dvo.put(vo.data(), m + 1, s));
  return build_core(*en.d, s, dkb.p, dko.p, dvb.p, dvo.p, m, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off,
                    node_cap, digests, true);
}

}  // extern "C"

// ------------------------------------------- sets onto a committed root
namespace {

// No item left: the blank root and no node (the outputs of build_empty, on the call's stream).
int nothing_left(hipStream_t s, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint64_t* node_off, bool host_out) {
  memcpy(root, kBlankRoot, 32);
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (node_off) {
    if (host_out) node_off[0] = 0;
    else HIP_OK(hipMemsetAsync(node_off, 0, 8, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  return PV_OK;
}

// A batch with removals onto the blank root: the removals are dropped and the rest is a build.
// The batch has passed tb_lcp_one, so its offsets are monotone and bounded.  Not a hot path (a
// ledger's first batch): the pairs are compacted on the host.
int build_without_removals(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb,
                           const uint64_t* vo, uint64_t n, StateStore* st, uint8_t* root, uint64_t* n_nodes,
                           uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                           uint64_t node_cap, uint8_t* digests, bool host_out) {
  std::vector<uint64_t> hko(n + 1), hvo(n + 1);
  HIP_OK(hipMemcpyAsync(hko.data(), ko, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(hvo.data(), vo, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) kept += hvo[i + 1] > hvo[i];
  if (kept == n)
    return build_core(d, s, kb, ko, vb, vo, n, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap,
                      digests, host_out);
  if (kept == 0) return nothing_left(s, root, n_nodes, n_bytes, node_off, host_out);
  std::vector<uint8_t> hk(hko[n] - hko[0]), hv(hvo[n] - hvo[0]);
  if (!hk.empty()) HIP_OK(hipMemcpyAsync(hk.data(), kb + hko[0], hk.size(), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(hv.data(), vb + hvo[0], hv.size(), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  std::vector<uint64_t> cko(kept + 1, 0), cvo(kept + 1, 0);
  std::vector<uint8_t> ck, cv;
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (hvo[i + 1] == hvo[i]) continue;
    ck.insert(ck.end(), hk.begin() + (hko[i] - hko[0]), hk.begin() + (hko[i + 1] - hko[0]));
    cv.insert(cv.end(), hv.begin() + (hvo[i] - hvo[0]), hv.begin() + (hvo[i + 1] - hvo[0]));
    ++k;
    cko[k] = ck.size();
    cvo[k] = cv.size();
  }
  ck.resize(ck.size() + 16, 0);
  cv.resize(cv.size() + 16, 0);
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(ck.data(), ck.size(), s));
  HIP_OK(dvb.put(cv.data(), cv.size(), s));
  HIP_OK(dko.put(cko.data(), kept + 1, s));
  HIP_OK(dvo.put(cvo.data(), kept + 1, s));
  return build_core(d, s, dkb.p, dko.p, dvb.p, dvo.p, kept, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off,
                    node_cap, digests, host_out);
}

// The update over device keys and values (sorted, distinct): the merge of
// pv_trie_update.h, then build_core over the merged items.  old_root, root,
// n_nodes and n_bytes are host memory; the node outputs as build_core's.
// removals (pv_state_apply): an empty value removes its key.
int update_core(Device& d, hipStream_t s, StateStore& st, const uint8_t* old_root, const uint8_t* kb,
                const uint64_t* ko, const uint8_t* vb, const uint64_t* vo, uint64_t n, bool insert, uint8_t* root,
                uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                uint64_t node_cap, uint8_t* digests, bool host_out, bool removals = false) {
  const bool blank = memcmp(old_root, kBlankRoot, 32) == 0;
  if (blank && !removals)   // nothing to merge with: the store is not read
    return build_core(d, s, kb, ko, vb, vo, n, insert ? &st : nullptr, root, n_nodes, n_bytes, node_blob, blob_cap,
                      node_off, node_cap, digests, host_out);
  const char* const what = removals ? "state apply" : "state update";
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  const int mb = merkle_blocks(d);
  TmpBuf<uint32_t> h, stats, droot, inib;
  TmpBuf<uint64_t> sizes, ikoff, ivoff;
  TmpBuf<uint8_t> status, ikey, ival, ikind;
  StreamDrain tail{s};
  // the batch's own checks and h[], by the build's first kernel: the same refusals
  pv::TbCtx b{};
  b.key_blob = kb;
  b.key_off = ko;
  b.val_blob = vb;
  b.val_off = vo;
  b.n = n;
  HIP_OK(h.alloc(n + 1));
  b.tree = h.p;
  uint32_t hs[5] = {0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0};   // hs[4]: the batch holds a removal
  HIP_OK(stats.put(hs, 5, s));
  if (removals) b.empty_seen = stats.p + 4;
  HIP_OK(pv::launch_trie_build_lcp(b, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 20, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (const int rc = lcp_refusal(hs)) return rc;
  // a batch without a removal is a batch of sets: it takes the walk without the removal mode
  const bool opening = removals && hs[4] != 0;
  if (blank)
    return build_without_removals(d, s, kb, ko, vb, vo, n, insert ? &st : nullptr, root, n_nodes, n_bytes, node_blob,
                                  blob_cap, node_off, node_cap, digests, host_out);
  // count, scan, write
  pv::TuCtx c{};
  c.blob = st.blob;
  c.beg = st.beg;
  c.end = st.end;
  c.dig = st.dig;
  c.table = st.table;
  c.slots = st.slots;
  c.n_nodes = (uint32_t)st.n_nodes;
  uint32_t rw[8];
  memcpy(rw, old_root, 32);
  HIP_OK(droot.put(rw, 8, s));
  c.root = droot.p;
  c.key_blob = kb;
  c.key_off = ko;
  c.val_blob = vb;
  c.val_off = vo;
  c.n = n;
  c.h = h.p;
  HIP_OK(sizes.alloc(3 * (n + 1)));
  HIP_OK(hipMemsetAsync(sizes.p, 0, 3 * (n + 1) * 8, s));
  c.cnt = sizes.p;
  c.pbytes = sizes.p + (n + 1);
  c.vbytes = sizes.p + 2 * (n + 1);
  HIP_OK(status.alloc(n));
  c.status = status.p;
  HIP_OK(opening ? pv::launch_trie_apply_count(c, mb, s) : pv::launch_trie_update_count(c, mb, s));
  std::vector<uint8_t> hstat(n);
  HIP_OK(hipMemcpyAsync(hstat.data(), status.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(n + 1)));
  HIP_OK(pv::launch_exclusive_scan(c.cnt, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(c.pbytes, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(c.vbytes, n + 1, d.scan.p, s));
  uint64_t tot[3] = {0, 0, 0};   // items, path bytes, payload bytes
  for (int k = 0; k < 3; ++k)
    HIP_OK(hipMemcpyAsync(&tot[k], sizes.p + k * (n + 1) + n, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (uint64_t j = 0; j < n; ++j)
    if (hstat[j] != pv::SP_OK)
      return fail(PV_EINVAL,
                  hstat[j] == pv::SP_NODE_MISSING
                      ? "%s: key %llu: the root or a node on its path is not in the store (status %u)"
                      : "%s: key %llu: a node on its path is not a well-formed trie node (status %u)",
                  what, (unsigned long long)j, (unsigned)hstat[j]);
  if ((!removals && tot[0] < n) || tot[0] > pv::TB_MAX_KEYS)
    return fail(PV_EINVAL, "%s: %llu merged items, above the 2^28 of one build", what, (unsigned long long)tot[0]);
  const uint64_t items = tot[0];
  if (items == 0) {   // every key of the state removed: no build launch
    tail.done = true;
    return nothing_left(s, root, n_nodes, n_bytes, node_off, host_out);
  }
  HIP_OK(ikey.alloc(tot[1] + 16));
  HIP_OK(ival.alloc(tot[2] + 16));
  HIP_OK(ikoff.alloc(items + 1));
  HIP_OK(ivoff.alloc(items + 1));
  HIP_OK(inib.alloc(items));
  HIP_OK(ikind.alloc(items));
  HIP_OK(hipMemsetAsync(ikey.p + tot[1], 0, 16, s));
  HIP_OK(hipMemsetAsync(ival.p + tot[2], 0, 16, s));
  HIP_OK(hipMemcpyAsync(ikoff.p + items, c.pbytes + n, 8, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(ivoff.p + items, c.vbytes + n, 8, hipMemcpyDeviceToDevice, s));
  c.ikey = ikey.p;
  c.ikoff = ikoff.p;
  c.ival = ival.p;
  c.ivoff = ivoff.p;
  c.inib = inib.p;
  c.ikind = ikind.p;
  HIP_OK(opening ? pv::launch_trie_apply_emit(c, mb, s) : pv::launch_trie_update_emit(c, mb, s));
  return build_core(d, s, ikey.p, ikoff.p, ival.p, ivoff.p, items, insert ? &st : nullptr, root, n_nodes, n_bytes,
                    node_blob, blob_cap, node_off, node_cap, digests, host_out, inib.p, ikind.p);
}

// n == 0: the root stays, no node, no launch for the update; every output that is given is
// written, and, as with the empty build, neither the store nor an input buffer is looked at
int update_empty(Entry& en, void* stream, const uint8_t* old_root, uint8_t* new_root, uint64_t* n_nodes,
                 uint64_t* n_bytes, uint64_t* node_off, bool host_out) {
  if (new_root && old_root) memcpy(new_root, old_root, 32);
  return build_empty(en, stream, nullptr, n_nodes, n_bytes, node_off, host_out);
}

// pv_state_update_device / pv_state_apply_device: device buffers, strictly increasing keys
int update_device_entry(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                        const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                        uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                        uint64_t node_cap, uint8_t* digests, void* stream, bool removals, bool unsorted = false) {
  Entry en;
  if (n == 0) {   // as the empty build: nothing is looked at, the store included
    if (const int rc = en.check()) return rc;
    return update_empty(en, stream, old_root, new_root, n_nodes, n_bytes, node_off, false);
  }
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (!old_root || !new_root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  if (unsorted) {   // pv_state_apply_unsorted_device: the device sort and the gather first
    if (n_nodes) *n_nodes = 0;
    if (n_bytes) *n_bytes = 0;
    DevicePairs sp;
    StreamDrain tail{en.s};
    if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, removals, sp)) return rc;
    return sort_selfcheck(update_core(*en.d, en.s, *st, old_root, sp.kb.p, sp.ko.p, sp.vb.p, sp.vo.p, sp.m, insert != 0,
                                      new_root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests,
                                      false, removals));
  }
  return update_core(*en.d, en.s, *st, old_root, key_blob, key_off, val_blob, val_off, n, insert != 0, new_root,
                     n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests, false, removals);
}

// pv_state_update / pv_state_apply: host buffers, keys in any order, the last of equal keys wins
int update_host_entry(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                      const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                      uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                      uint64_t node_cap, uint8_t* digests, bool removals) {
  if (n == 0) {
    Entry en;
    if (const int rc = en.check()) return rc;
    return update_empty(en, nullptr, old_root, new_root, n_nodes, n_bytes, node_off, true);
  }
  // checks and the sorted copy before the library lock, as pv_state_build
  if (!old_root || !new_root) return fail(PV_EINVAL, "null pointer");
  std::vector<uint64_t> ko, vo;
  std::vector<uint8_t> kb, vb;
  if (const int rc = sorted_pairs(key_blob, key_off, val_blob, val_off, n, ko, vo, kb, vb, removals)) return rc;
  const uint64_t m = ko.size() - 1;
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(kb.data(), kb.size(), s));
  HIP_OK(dvb.put(vb.data(), vb.size(), s));
  HIP_OK(dko.put(ko.data(), m + 1, s));
  HIP_OK(dvo.put(vo.data(), m + 1, s));
  return update_core(*en.d, s, *st, old_root, dkb.p, dko.p, dvb.p, dvo.p, m, insert != 0, new_root, n_nodes, n_bytes,
                     node_blob, blob_cap, node_off, node_cap, digests, true, removals);
}

}  // namespace

extern "C" {

// A 3PC batch of PruningState.set onto the state at a committed root, and the new headHash
// (state/pruning_state.py:60-61, 136; Trie.update, state/trie/pruning_trie.py:1006-1027), as one
// batch over device buffers; see include/plenum_verify.h.
int pv_state_update_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                           const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert,
                           uint8_t* new_root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
                           uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, false);
}

// The host form of the same (state/pruning_state.py:60-61; state/trie/pruning_trie.py:1006-1027):
// keys in any order, the last of equal keys wins, as a sequence of sets gives.
int pv_state_update(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                    const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                    uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                    uint64_t node_cap, uint8_t* digests) {
  return update_host_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                           n_bytes, node_blob, blob_cap, node_off, node_cap, digests, false);
}

// A 3PC batch of PruningState.set and PruningState.remove onto the state at a committed root, and
// the new headHash (state/pruning_state.py:60-61, 84-85, 136; Trie.update and Trie.delete,
// state/trie/pruning_trie.py:1006-1027, 683-848), as one batch over device buffers: an empty
// value removes its key; see include/plenum_verify.h.
int pv_state_apply_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                          const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                          uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap,
                          uint64_t* node_off, uint64_t node_cap, uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, true);
}

// pv_state_apply_device over pairs in any order, the last of equal keys winning (a later removal
// over an earlier set as a later set over an earlier removal): the device sort, the gather, then
// the same apply; see include/plenum_verify.h.
int pv_state_apply_unsorted_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob,
                                   const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                                   uint64_t n, int insert, uint8_t* new_root, uint64_t* n_nodes, uint64_t* n_bytes,
                                   uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap,
                                   uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, true, true);
}

// The host form of the same (state/pruning_state.py:60-61, 84-85; state/trie/pruning_trie.py:683-848,
// 1006-1027): keys in any order, the last of equal keys wins, a removal over a set as a set over a
// removal, as the sequence of calls gives.
int pv_state_apply(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                   const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                   uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                   uint64_t node_cap, uint8_t* digests) {
  return update_host_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                           n_bytes, node_blob, blob_cap, node_off, node_cap, digests, true);
}

}  // extern "C"

// ------------------------------------------------------- reads at a root
namespace {

// the walk and the scan of a read: status / found / src / val_off (scanned) are device memory
int get_walk(StateStore& st, Device& d, hipStream_t s, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
             const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, bool decode, uint8_t* status,
             uint8_t* found, uint64_t* src, uint64_t* val_off) {
  HIP_OK(d.scan.ensure(pv::scan_sums_words(n_queries + 1)));
  HIP_OK(pv::launch_trie_get(st.blob, st.beg, st.end, st.dig, st.table, st.slots, (uint32_t)st.n_nodes, w32(roots),
                             root_idx, n_roots, key_blob, key_off, n_queries, decode, status, found, src, val_off,
                             merkle_blocks(d), s));
  HIP_OK(pv::launch_exclusive_scan(val_off, n_queries + 1, d.scan.p, s));
  return PV_OK;
}

int cap_refusal(uint64_t val_cap, uint64_t total) {
  return fail(PV_EINVAL, "val_cap %llu is below the %llu bytes of the values", (unsigned long long)val_cap,
              (unsigned long long)total);
}

}  // namespace

extern "C" {

// PruningState.get / get_for_root_hash per key (state/pruning_state.py:63-77; with decode,
// get_decoded, :162-163; Trie._get, state/trie/pruning_trie.py:376-407) as one batch at any roots
// the store holds; see include/plenum_verify.h.
int pv_state_store_get(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                       const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, int32_t decode,
                       uint8_t* status, uint8_t* found, uint64_t* val_off, uint8_t* val_blob, uint64_t val_cap) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_off || !status || !found || !val_off) return fail(PV_EINVAL, "null buffer");
  if (decode != 0 && decode != 1) return fail(PV_EINVAL, "decode must be 0 or 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40)) return fail(PV_EINVAL, "more than 2^40 queries in one call");
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
  TmpBuf<uint8_t> droots, dkeys, dstatus, dfound, dvals;
  TmpBuf<uint32_t> dridx;
  TmpBuf<uint64_t> dkoff, dsrc, dvoff;
  StreamDrain tail{s};
  HIP_OK(droots.put(roots, n_roots * 32, s));
  if (root_idx) HIP_OK(dridx.put(root_idx, n_queries, s));
  HIP_OK(dkeys.alloc(keys.len + 4));
  if (keys.len) HIP_OK(hipMemcpyAsync(dkeys.p, key_blob + keys.b0, keys.len, hipMemcpyHostToDevice, s));
  HIP_OK(dkoff.put(keys.rebased(), n_queries + 1, s));
  HIP_OK(dstatus.alloc(n_queries));
  HIP_OK(dfound.alloc(n_queries));
  HIP_OK(dsrc.alloc(n_queries));
  HIP_OK(dvoff.alloc(n_queries + 1));
  if (const int rc = get_walk(*st, d, s, droots.p, root_idx ? dridx.p : nullptr, n_roots, dkeys.p, dkoff.p, n_queries,
                              decode != 0, dstatus.p, dfound.p, dsrc.p, dvoff.p))
    return rc;
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n_queries, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(found, dfound.p, n_queries, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(val_off, dvoff.p, (n_queries + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const uint64_t total = val_off[n_queries];
  if (!val_blob) return tail.finish();   // the sizing call
  if (val_cap < total) return cap_refusal(val_cap, total);
  if (total == 0) return tail.finish();
  HIP_OK(dvals.alloc(total));
  HIP_OK(pv::launch_trie_get_copy(st->blob, dsrc.p, dvoff.p, n_queries, dvals.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(val_blob, dvals.p, total, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

// The same read (state/pruning_state.py:63-77, 162-163) over DEVICE buffers, which only the
// kernels read: key_off and root_idx are not checked here; see include/plenum_verify.h.
int pv_state_store_get_device(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                              const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, int32_t decode,
                              uint8_t* status, uint8_t* found, uint64_t* val_off, uint8_t* val_blob, uint64_t val_cap,
                              void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_blob || !key_off || !status || !found || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (decode != 0 && decode != 1) return fail(PV_EINVAL, "decode must be 0 or 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40)) return fail(PV_EINVAL, "more than 2^40 queries in one call");
  if (reinterpret_cast<uintptr_t>(roots) & 3u) return fail(PV_EINVAL, "roots must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  Device& d = *en.d;
  HIP_OK(d.vsrc.ensure(n_queries));
  if (const int rc = get_walk(*st, d, en.s, roots, root_idx, n_roots, key_blob, key_off, n_queries, decode != 0, status,
                              found, d.vsrc.p, val_off))
    return rc;
  uint64_t total = 0;
  HIP_OK(hipMemcpyAsync(&total, val_off + n_queries, 8, hipMemcpyDeviceToHost, en.s));
  HIP_OK(hipStreamSynchronize(en.s));
  if (!val_blob) return PV_OK;   // the sizing call
  if (val_cap < total) return cap_refusal(val_cap, total);
  if (total == 0) return PV_OK;
  HIP_OK(pv::launch_trie_get_copy(st->blob, d.vsrc.p, val_off, n_queries, val_blob, merkle_blocks(d), en.s));
  return en.finish();
}

}  // extern "C"
