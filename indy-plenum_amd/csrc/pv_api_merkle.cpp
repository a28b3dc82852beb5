// The ledger part of include/plenum_verify.h: pv_sha256_batch*, pv_merkle_root*,
// inclusion / consistency verification, and the resident Merkle tree
// (pv_merkle_tree_*: audit paths, the write cycle, the hash store).
#include "pv_api_common.h"

using namespace pvapi;

namespace {
// leaf digests (n x 8 words) -> root (8 words) on stream s, all device memory
// root of the empty tree: hash_empty(), SHA-256 of the empty string (ledger/tree_hasher.py:17-19)
const uint32_t EMPTY_ROOT[8] = {0x42c4b0e3u, 0x141cfc98u, 0xc8f4fb9au, 0x24b96f99u,
                                0xe441ae27u, 0x4c939b64u, 0x1b9995a4u, 0x55b85278u};
int enqueue_merkle(Device& d, const uint8_t* blob, const uint64_t* off, uint64_t n, uint32_t* leaves, uint32_t* root,
                   hipStream_t s) {
  if (n == 0) {
    HIP_OK(hipMemcpyAsync(root, EMPTY_ROOT, 32, hipMemcpyHostToDevice, s));
    return PV_OK;
  }
  HIP_OK(pv::launch_sha256(blob, off, n, 1, 0x00, d.counter.p, leaves, d.sha256_blocks, s));
  const uint32_t* in = leaves;
  uint64_t m = n;
  int which = 0;
  while (m > 1) {
    if (m <= (uint64_t)pv::MERKLE_TAIL) {   // the last levels: one launch
      HIP_OK(pv::launch_merkle_tail(in, m, root, s));
      break;
    }
    uint32_t* out = (m + 1) / 2 == 1 ? root : (which ? d.mk1.p : d.mk0.p);
    HIP_OK(pv::launch_merkle_level(in, m, out, s));
    in = out;
    m = (m + 1) / 2;
    which ^= 1;
  }
  if (n == 1) HIP_OK(hipMemcpyAsync(root, leaves, 32, hipMemcpyDeviceToDevice, s));
  return PV_OK;
}
}  // namespace

extern "C" {

int pv_sha256_batch_device(const uint8_t* blob, const uint64_t* off, uint64_t n, int32_t prefix, uint8_t* digests,
                           int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!blob || !off || !digests) return fail(PV_EINVAL, "null device buffer");
  if (prefix > 255) return fail(PV_EINVAL, "prefix must be -1 (none) or a byte value");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_sha256(blob, off, n, prefix < 0 ? 0 : 1, prefix < 0 ? 0 : (uint32_t)prefix, en.d->counter.p,
                           reinterpret_cast<uint32_t*>(digests), en.d->sha256_blocks, en.s));
  return en.finish();
}

int pv_merkle_root_device(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* leaf_hashes, uint8_t* root,
                          int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!root || (n && (!blob || !off))) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  uint32_t* leaves = reinterpret_cast<uint32_t*>(leaf_hashes);
  if (!leaves && n) {
    HIP_OK(d->mk1.ensure((n + 1) / 2 * 8 + n * 8));
    leaves = d->mk1.p + (n + 1) / 2 * 8;
  }
  HIP_OK(d->mk0.ensure((n + 1) / 2 * 8 + 8));
  if (leaf_hashes) HIP_OK(d->mk1.ensure((n + 1) / 2 * 8 + 8));
  return en.finish(enqueue_merkle(*d, blob, off, n, leaves, reinterpret_cast<uint32_t*>(root), en.s));
}

int pv_merkle_root(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* root, uint8_t* leaf_hashes) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (!root || (n && (!off || (!blob && off[n] != off[0])))) return fail(PV_EINVAL, "null buffer");
  Ragged leaf(off, n);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure((n + 1) / 2 * 8 + 8));
  HIP_OK(d.mk1.ensure((n + 1) / 2 * 8 + n * 8 + 8));
  uint32_t* leaves = d.mk1.p + (n + 1) / 2 * 8;
  uint32_t* droot = d.mk0.p + (n + 1) / 2 * 8;
  if (const int rc = leaf.stage(blob, d, d.stream)) return rc;
  if (const int rc = enqueue_merkle(d, d.blob.p, d.off.p, n, leaves, droot, d.stream)) return rc;
  HIP_OK(hipMemcpyAsync(root, droot, 32, hipMemcpyDeviceToHost, d.stream));
  if (leaf_hashes && n) HIP_OK(hipMemcpyAsync(leaf_hashes, leaves, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_sha256_batch(const uint8_t* blob, const uint64_t* off, uint64_t n, int32_t prefix, uint8_t* digests) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!off || !digests || (!blob && off[n] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (prefix > 255) return fail(PV_EINVAL, "prefix must be -1 (none) or a byte value");
  Ragged msgs(off, n);
  if (const int rc = msgs.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure(n * 8));
  if (const int rc = msgs.stage(blob, d, d.stream)) return rc;
  HIP_OK(pv::launch_sha256(d.blob.p, d.off.p, n, prefix < 0 ? 0 : 1, prefix < 0 ? 0 : (uint32_t)prefix, d.counter.p,
                           d.mk0.p, d.sha256_blocks, d.stream));
  HIP_OK(hipMemcpyAsync(digests, d.mk0.p, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

}  // extern "C"

// ------------------------------------------ Merkle audit paths / consistency
namespace {

// A resident tree: one device buffer per level (level 0 = leaf hashes, an odd
// last node moves up), capacities geometric, plus the device table of level
// pointers the generation kernels read.
constexpr uint32_t MT_LEVELS = 65;
struct MerkleTree {
  bool live = false;
  int dev = -1;           // Device::id
  uint64_t n = 0;         // leaves
  uint64_t committed = 0; // leaves [committed, n) are staged (pv_merkle_tree_stage*)
  uint32_t depth = 0;     // levels above the leaves
  uint64_t hint = 1;
  std::vector<uint32_t*> lv;
  std::vector<uint64_t> cap;   // nodes
  const uint32_t** table = nullptr;   // device: MT_LEVELS level pointers
  std::vector<const uint32_t*> host_table;
  bool dirty = true;
};

void tree_drop(MerkleTree& t) {
  for (uint32_t* p : t.lv)
    if (p) (void)hipFree(p);
  if (t.table) (void)hipFree(t.table);
}
HandleTable<MerkleTree> g_trees{tree_drop, "Merkle tree", "handle"};   // handle = index + 1
int tree_enter(Entry& en, int32_t handle, MerkleTree** t) { return g_trees.enter(en, handle, t); }

uint64_t level_count(uint64_t n, uint32_t l) { return n == 0 ? 0 : ((n - 1) >> l) + 1; }

// level l holds at least `need` nodes afterwards; on overflow the capacity
// doubles and the nodes in use are copied device-to-device on s
int tree_grow(MerkleTree& t, uint32_t l, uint64_t need, hipStream_t s) {
  if (l >= MT_LEVELS) return fail(PV_EINVAL, "Merkle tree deeper than %u levels", MT_LEVELS - 1);
  if (l >= t.lv.size()) {
    t.lv.resize(l + 1, nullptr);
    t.cap.resize(l + 1, 0);
  }
  if (need <= t.cap[l]) return PV_OK;
  uint64_t used = l <= t.depth ? level_count(t.n, l) : 0;
  if (used > t.cap[l]) used = t.cap[l];
  const uint64_t first = l < 64 ? ((t.hint - 1) >> l) + 1 : 1;   // an empty level: its share of the hint
  uint64_t words = t.cap[l] * 8;                                 // 8 words per node
  if (const int rc = grow_device(&t.lv[l], &words, need * 8, used * 8, 0, first * 8, s)) return rc;
  t.cap[l] = words / 8;
  t.dirty = true;
  return PV_OK;
}

// a level moved (or the tree is new): the table of level pointers the read kernels use
int tree_publish(MerkleTree& t, hipStream_t s) {
  if (!t.dirty) return PV_OK;
  if (!t.table) HIP_OK(hipMalloc(reinterpret_cast<void**>(&t.table), MT_LEVELS * sizeof(uint32_t*)));
  t.host_table.assign(MT_LEVELS, nullptr);
  for (size_t i = 0; i < t.lv.size(); ++i) t.host_table[i] = t.lv[i];
  HIP_OK(hipMemcpyAsync(t.table, t.host_table.data(), MT_LEVELS * sizeof(uint32_t*), hipMemcpyHostToDevice, s));
  t.dirty = false;
  return PV_OK;
}

// leaves n .. n + k - 1 are in level 0: rebuild the parents they change.  At
// level l + 1 the first changed parent is n_old >> (l + 1) (the old promoted
// right-edge node is recomputed); levels are added as the tree deepens.
int tree_rebuild(MerkleTree& t, uint64_t n_new, hipStream_t s) {
  const uint64_t n_old = t.n;
  uint64_t m = n_new;
  uint32_t l = 0;
  while (m > 1) {
    const uint64_t outs = (m + 1) / 2;
    int rc = tree_grow(t, l + 1, outs, s);
    if (rc) return rc;
    HIP_OK(pv::launch_merkle_level_keep(t.lv[l], l + 1 < 64 ? n_old >> (l + 1) : 0, m, t.lv[l + 1], s));
    m = outs;
    ++l;
  }
  t.depth = l;
  t.n = n_new;
  return tree_publish(t, s);
}

// extend* appends and commits: refused while leaves are staged
int tree_unstaged(const MerkleTree& t) {
  if (t.committed == t.n) return PV_OK;
  return fail(PV_EINVAL, "the tree holds %llu staged leaves: commit or discard them before extend",
              (unsigned long long)(t.n - t.committed));
}

// the tree has n_new leaves and the leaves from f0 on are new (stage: f0 = the old size) or lost
// their right neighbours (discard: f0 = n_new - 1): one k_merkle_edge launch rebuilds their ancestors
int tree_edge(MerkleTree& t, uint64_t f0, uint64_t n_new, hipStream_t s) {
  uint32_t depth = 0;
  for (uint64_t m = n_new; m > 1; m = (m + 1) / 2) {
    ++depth;
    if (const int rc = tree_grow(t, depth, (m + 1) / 2, s)) return rc;
  }
  if (n_new > 1) HIP_OK(pv::launch_merkle_edge(t.lv.data(), depth + 1, f0, n_new, s));
  t.depth = depth;
  t.n = n_new;
  return tree_publish(t, s);
}

// root (HOST, may be null) <- MTH(0, n) once the work queued on s is done
int tree_root(const MerkleTree& t, uint8_t* root, hipStream_t s) {
  if (!root) return PV_OK;
  if (t.n == 0) {
    memcpy(root, EMPTY_ROOT, 32);
    return PV_OK;
  }
  HIP_OK(hipMemcpyAsync(root, t.lv[t.depth], 32, hipMemcpyDeviceToHost, s));
  return PV_OK;
}

// k staged leaf hashes are in level 0 behind the n the tree has: their ancestors.  Up to
// MERKLE_EDGE_MAX leaves in one launch, more by the per-level rebuild of extend.
int tree_stage(MerkleTree& t, uint64_t k, uint8_t* root_out, hipStream_t s) {
  const int rc = k <= pv::MERKLE_EDGE_MAX ? tree_edge(t, t.n, t.n + k, s) : tree_rebuild(t, t.n + k, s);
  if (rc) return rc;
  return tree_root(t, root_out, s);
}

// all device memory; leaf = leaf hashes, or NULL: hash blob / off into d.mk0 first
int enqueue_verify_incl(Device& d, const uint32_t* leaf, const uint8_t* blob, const uint64_t* off,
                        const uint64_t* index, const uint64_t* tree_size, const uint32_t* nodes,
                        const uint64_t* proof_off, const uint32_t* roots, const uint32_t* root_idx, uint64_t n,
                        uint8_t* status, uint32_t* computed, uint64_t* stop_index, hipStream_t s) {
  if (!leaf) {   // leaf mode: the existing leaf hasher, then the walk
    HIP_OK(d.mk0.ensure(n * 8));
    HIP_OK(pv::launch_sha256(blob, off, n, 1, 0x00, d.counter.p, d.mk0.p, d.sha256_blocks, s));
    leaf = d.mk0.p;
  }
  HIP_OK(pv::launch_merkle_verify_incl(leaf, index, tree_size, nodes, proof_off, roots, root_idx, n, status, computed,
                                       stop_index, merkle_blocks(d), s));
  return PV_OK;
}

}  // namespace

void pvapi::release_trees() { g_trees.release_all(); }

extern "C" {

int pv_merkle_verify_inclusion_device(const uint8_t* leaf_hashes, const uint8_t* leaf_blob, const uint64_t* leaf_off,
                                      const uint64_t* index, const uint64_t* tree_size, const uint8_t* nodes,
                                      const uint64_t* proof_off, const uint8_t* roots, const uint32_t* root_idx,
                                      uint64_t n_roots, uint64_t n, uint8_t* status, uint8_t* computed,
                                      uint64_t* stop_index, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if ((!leaf_hashes && (!leaf_blob || !leaf_off)) || !index || !tree_size || !nodes || !proof_off || !roots ||
      !status || !computed || !stop_index)
    return fail(PV_EINVAL, "null device buffer");
  if (root_idx && n_roots == 0) return fail(PV_EINVAL, "root_idx without roots");
  if (misaligned16(leaf_hashes) || misaligned16(nodes) || misaligned16(roots) || misaligned16(computed))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  return en.finish(enqueue_verify_incl(*en.d, w32(leaf_hashes), leaf_blob, leaf_off, index, tree_size, w32(nodes),
                                       proof_off, w32(roots), root_idx, n, status, w32(computed), stop_index, en.s));
}

int pv_merkle_verify_inclusion(const uint8_t* leaf_hashes, const uint8_t* leaf_blob, const uint64_t* leaf_off,
                               const uint64_t* index, const uint64_t* tree_size, const uint8_t* nodes,
                               const uint64_t* proof_off, const uint8_t* roots, const uint32_t* root_idx,
                               uint64_t n_roots, uint64_t n, uint8_t* status, uint8_t* computed,
                               uint64_t* stop_index) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if ((!leaf_hashes && !leaf_off) || !index || !tree_size || !proof_off || !roots || !status || !computed ||
      !stop_index)
    return fail(PV_EINVAL, "null buffer");
  Ragged proofs(proof_off, n);   // in nodes
  if (const int rc = proofs.check("proof_off")) return rc;
  if (proofs.len && !nodes) return fail(PV_EINVAL, "null buffer");
  Ragged leaf(leaf_hashes ? nullptr : leaf_off, leaf_hashes ? 0 : n);   // leaf mode only
  if (const int rc = leaf.check("leaf_off")) return rc;
  if (leaf.len && !leaf_blob) return fail(PV_EINVAL, "null buffer");
  if (root_idx)
    for (uint64_t i = 0; i < n; ++i)
      if (root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "root_idx[%llu] = %u is not below n_roots %llu", (unsigned long long)i, root_idx[i],
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dleaf, dblob, dnodes, droots, dstatus, dcomp;
  TmpBuf<uint64_t> dloff, dindex, dsize, dpoff, dstop;
  TmpBuf<uint32_t> dridx;
  StreamDrain tail{s};
  if (leaf_hashes) {
    HIP_OK(dleaf.put(leaf_hashes, n * 32, s));
  } else if (const int rc = leaf.stage(leaf_blob, dblob, dloff, s)) {
    return rc;
  }
  HIP_OK(dindex.put(index, n, s));
  HIP_OK(dsize.put(tree_size, n, s));
  HIP_OK(dnodes.put(proofs.len ? nodes + proofs.b0 * 32 : nullptr, proofs.len * 32, s));
  HIP_OK(dpoff.put(proofs.rebased(), n + 1, s));
  HIP_OK(droots.put(roots, (root_idx ? n_roots : n) * 32, s));
  if (root_idx) HIP_OK(dridx.put(root_idx, n, s));
  HIP_OK(dstatus.alloc(n));
  HIP_OK(dcomp.alloc(n * 32));
  HIP_OK(dstop.alloc(n));
  if (const int rc = enqueue_verify_incl(*en.d, leaf_hashes ? w32(dleaf.p) : nullptr, dblob.p, dloff.p, dindex.p,
                                         dsize.p, w32(dnodes.p), dpoff.p, w32(droots.p), dridx.p, n, dstatus.p,
                                         w32(dcomp.p), dstop.p, s))
    return rc;
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(computed, dcomp.p, n * 32, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(stop_index, dstop.p, n * 8, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

int pv_merkle_verify_consistency_device(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                        const uint8_t* new_roots, const uint32_t* old_root_idx,
                                        const uint32_t* new_root_idx, uint64_t n_roots, const uint8_t* nodes,
                                        const uint64_t* proof_off, uint64_t n, uint8_t* status, uint8_t* old_computed,
                                        uint8_t* new_computed, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!old_size || !new_size || !old_roots || !new_roots || !nodes || !proof_off || !status || !old_computed ||
      !new_computed)
    return fail(PV_EINVAL, "null device buffer");
  if ((old_root_idx == nullptr) != (new_root_idx == nullptr))
    return fail(PV_EINVAL, "old_root_idx and new_root_idx go together");
  if (old_root_idx && n_roots == 0) return fail(PV_EINVAL, "root indices without roots");
  if (misaligned16(old_roots) || misaligned16(new_roots) || misaligned16(nodes) || misaligned16(old_computed) ||
      misaligned16(new_computed))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_merkle_verify_cons(old_size, new_size, w32(old_roots), w32(new_roots), old_root_idx, new_root_idx,
                                       w32(nodes), proof_off, n, status, w32(old_computed), w32(new_computed),
                                       merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_merkle_verify_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                 const uint8_t* new_roots, const uint32_t* old_root_idx, const uint32_t* new_root_idx,
                                 uint64_t n_roots, const uint8_t* nodes, const uint64_t* proof_off, uint64_t n,
                                 uint8_t* status, uint8_t* old_computed, uint8_t* new_computed) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!old_size || !new_size || !old_roots || !new_roots || !proof_off || !status || !old_computed || !new_computed)
    return fail(PV_EINVAL, "null buffer");
  if ((old_root_idx == nullptr) != (new_root_idx == nullptr))
    return fail(PV_EINVAL, "old_root_idx and new_root_idx go together");
  Ragged proofs(proof_off, n);   // in nodes
  if (const int rc = proofs.check("proof_off")) return rc;
  if (proofs.len && !nodes) return fail(PV_EINVAL, "null buffer");
  if (old_root_idx)
    for (uint64_t i = 0; i < n; ++i)
      if (old_root_idx[i] >= n_roots || new_root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "a root index of pair %llu is not below n_roots %llu", (unsigned long long)i,
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  const uint64_t nr = old_root_idx ? n_roots : n;
  TmpBuf<uint8_t> dnodes, dro, drn, dstatus, dco, dcn;
  TmpBuf<uint64_t> dold, dnew, dpoff;
  TmpBuf<uint32_t> dio, din;
  StreamDrain tail{s};
  HIP_OK(dold.put(old_size, n, s));
  HIP_OK(dnew.put(new_size, n, s));
  HIP_OK(dro.put(old_roots, nr * 32, s));
  HIP_OK(drn.put(new_roots, nr * 32, s));
  if (old_root_idx) {
    HIP_OK(dio.put(old_root_idx, n, s));
    HIP_OK(din.put(new_root_idx, n, s));
  }
  HIP_OK(dnodes.put(proofs.len ? nodes + proofs.b0 * 32 : nullptr, proofs.len * 32, s));
  HIP_OK(dpoff.put(proofs.rebased(), n + 1, s));
  HIP_OK(dstatus.alloc(n));
  HIP_OK(dco.alloc(n * 32));
  HIP_OK(dcn.alloc(n * 32));
  HIP_OK(pv::launch_merkle_verify_cons(dold.p, dnew.p, w32(dro.p), w32(drn.p), dio.p, din.p, w32(dnodes.p), dpoff.p, n,
                                       dstatus.p, w32(dco.p), w32(dcn.p), merkle_blocks(*en.d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(old_computed, dco.p, n * 32, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(new_computed, dcn.p, n * 32, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

int pv_merkle_tree_create(uint64_t capacity_hint, int device, int32_t* handle) {
  Entry en(device);
  if (!handle) return fail(PV_EINVAL, "null pointer");
  if (const int rc = en.check()) return rc;
  Device* d = en.d;
  if (capacity_hint > (1ull << 40)) return fail(PV_EINVAL, "capacity_hint above 2^40 leaves");
  int32_t id;
  MerkleTree* tp;
  if (const int rc = g_trees.alloc(d->id, &id, &tp)) return rc;
  MerkleTree& t = *tp;
  t.hint = capacity_hint ? capacity_hint : 1;
  if (const int rc = en.begin()) return rc;
  int rc = tree_grow(t, 0, t.hint, d->stream);
  if (rc == PV_OK) rc = tree_rebuild(t, 0, d->stream);   // uploads the level table
  if (rc == PV_OK) {
    hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) rc = fail(PV_EIO, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  }
  if (rc) {
    g_trees.release(t);
    return rc;
  }
  *handle = id;
  return PV_OK;
}

int pv_merkle_tree_free(int32_t handle) { return g_trees.free(handle); }

// append k leaf hashes from host or device memory and rebuild the parents they change
static int tree_extend_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, hipMemcpyKind kind,
                              void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!leaf_hashes) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  if (const int rc = tree_unstaged(*t)) return rc;
  if (const int rc = en.begin(stream)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, en.s)) return rc;
  HIP_OK(hipMemcpyAsync(t->lv[0] + 8 * t->n, leaf_hashes, k * 32, kind, en.s));
  if (const int rc = tree_rebuild(*t, t->n + k, en.s)) return rc;
  t->committed = t->n;
  return en.finish();
}

int pv_merkle_tree_extend_hashes_device(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, void* stream) {
  return tree_extend_hashes(handle, leaf_hashes, k, hipMemcpyDeviceToDevice, stream);
}

int pv_merkle_tree_extend_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k) {
  return tree_extend_hashes(handle, leaf_hashes, k, hipMemcpyHostToDevice, nullptr);
}

int pv_merkle_tree_extend(int32_t handle, const uint8_t* blob, const uint64_t* off, uint64_t k) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!off || (!blob && off[k] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  Ragged leaf(off, k);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = tree_unstaged(*t)) return rc;
  if (const int rc = en.begin()) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  if (const int rc = leaf.stage(blob, *d, s)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, s)) return rc;
  HIP_OK(pv::launch_sha256(d->blob.p, d->off.p, k, 1, 0x00, d->counter.p, t->lv[0] + 8 * t->n, d->sha256_blocks, s));
  if (const int rc = tree_rebuild(*t, t->n + k, s)) return rc;
  t->committed = t->n;
  return en.finish();
}

int pv_merkle_tree_info(int32_t handle, uint64_t* n, uint32_t* depth, uint8_t* root) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (n) *n = t->n;
  if (depth) *depth = t->depth;
  if (root && t->n == 0) memcpy(root, EMPTY_ROOT, 32);
  if (!root || t->n == 0) return PV_OK;
  if (const int rc = en.begin()) return rc;
  HIP_OK(hipMemcpyAsync(root, t->lv[t->depth], 32, hipMemcpyDeviceToHost, en.s));
  return en.finish();
}

// k requests over a resident tree: audit paths (a = index, b = tree_size, roots_out given) or
// consistency proofs (a = first, b = second).  host: the arrays are host memory and every
// request is checked before any launch; else they are device memory and the kernel marks a
// refused request in its length.
static int tree_requests(int32_t handle, const uint64_t* a, const uint64_t* b, uint64_t k, uint8_t* nodes_out,
                         uint32_t* len_out, uint8_t* roots_out, bool paths, bool host, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!a || !b || !nodes_out || !len_out || (paths && !roots_out)) return fail(PV_EINVAL, "null buffer");
  if (host) {
    for (uint64_t i = 0; i < k; ++i)   // refused before any launch, never clamped
      if (paths ? (b[i] == 0 || b[i] > t->n || a[i] >= b[i]) : (a[i] > b[i] || b[i] > t->n))
        return fail(PV_EINVAL, "request %llu: (%llu, %llu) outside a tree of %llu leaves", (unsigned long long)i,
                    (unsigned long long)a[i], (unsigned long long)b[i], (unsigned long long)t->n);
  } else if (misaligned16(nodes_out) || misaligned16(roots_out)) {
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  }
  if (const int rc = en.begin(stream)) return rc;
  hipStream_t s = en.s;
  const uint64_t node_bytes = k * ((uint64_t)t->depth + 1) * 32;
  TmpBuf<uint64_t> da, db;
  TmpBuf<uint8_t> dnodes, droots;
  TmpBuf<uint32_t> dlen;
  StreamDrain tail{s};
  const uint64_t *pa = a, *pb = b;
  uint8_t *pn = nodes_out, *pr = roots_out;
  uint32_t* pl = len_out;
  if (host) {
    HIP_OK(da.put(a, k, s));
    HIP_OK(db.put(b, k, s));
    HIP_OK(dnodes.alloc(node_bytes));
    HIP_OK(droots.alloc(k * 32));
    HIP_OK(dlen.alloc(k));
    pa = da.p, pb = db.p, pn = dnodes.p, pr = droots.p, pl = dlen.p;
  }
  if (paths)
    HIP_OK(pv::launch_merkle_paths(t->table, t->n, t->depth, pa, pb, k, w32(pn), pl, w32(pr), merkle_blocks(*en.d), s));
  else
    HIP_OK(pv::launch_merkle_cons_proofs(t->table, t->n, t->depth, pa, pb, k, w32(pn), pl, merkle_blocks(*en.d), s));
  if (host) {
    HIP_OK(hipMemcpyAsync(nodes_out, pn, node_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(len_out, pl, k * 4, hipMemcpyDeviceToHost, s));
    if (paths) HIP_OK(hipMemcpyAsync(roots_out, pr, k * 32, hipMemcpyDeviceToHost, s));
  }
  return tail.finish();
}

int pv_merkle_audit_paths_device(int32_t handle, const uint64_t* index, const uint64_t* tree_size, uint64_t k,
                                 uint8_t* nodes_out, uint32_t* len_out, uint8_t* roots_out, void* stream) {
  return tree_requests(handle, index, tree_size, k, nodes_out, len_out, roots_out, true, false, stream);
}

int pv_merkle_audit_paths(int32_t handle, const uint64_t* index, const uint64_t* tree_size, uint64_t k,
                          uint8_t* nodes_out, uint32_t* len_out, uint8_t* roots_out) {
  return tree_requests(handle, index, tree_size, k, nodes_out, len_out, roots_out, true, true, nullptr);
}

int pv_merkle_consistency_proofs_device(int32_t handle, const uint64_t* first, const uint64_t* second, uint64_t k,
                                        uint8_t* nodes_out, uint32_t* len_out, void* stream) {
  return tree_requests(handle, first, second, k, nodes_out, len_out, nullptr, false, false, stream);
}

int pv_merkle_consistency_proofs(int32_t handle, const uint64_t* first, const uint64_t* second, uint64_t k,
                                 uint8_t* nodes_out, uint32_t* len_out) {
  return tree_requests(handle, first, second, k, nodes_out, len_out, nullptr, false, true, nullptr);
}

// ------------------------------------------------ the ledger write cycle
// stage k leaf hashes from host or device memory
static int tree_stage_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out,
                             hipMemcpyKind kind, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;   // as extend: nothing staged, nothing written
  if (!leaf_hashes) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  if (const int rc = en.begin(stream)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, en.s)) return rc;
  HIP_OK(hipMemcpyAsync(t->lv[0] + 8 * t->n, leaf_hashes, k * 32, kind, en.s));
  return en.finish(tree_stage(*t, k, root_out, en.s));
}

int pv_merkle_tree_stage_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out) {
  return tree_stage_hashes(handle, leaf_hashes, k, root_out, hipMemcpyHostToDevice, nullptr);
}

int pv_merkle_tree_stage_hashes_device(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out,
                                       void* stream) {
  return tree_stage_hashes(handle, leaf_hashes, k, root_out, hipMemcpyDeviceToDevice, stream);
}

int pv_merkle_tree_stage(int32_t handle, const uint8_t* blob, const uint64_t* off, uint64_t k, uint8_t* root_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;   // as extend: nothing staged, nothing written
  if (!off || (!blob && off[k] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  Ragged leaf(off, k);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  if (const int rc = leaf.stage(blob, *d, s)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, s)) return rc;
  HIP_OK(pv::launch_sha256(d->blob.p, d->off.p, k, 1, 0x00, d->counter.p, t->lv[0] + 8 * t->n, d->sha256_blocks, s));
  return en.finish(tree_stage(*t, k, root_out, s));
}

int pv_merkle_tree_commit(int32_t handle, uint64_t count) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (count > t->n - t->committed)
    return fail(PV_EINVAL, "commit of %llu leaves, %llu staged", (unsigned long long)count,
                (unsigned long long)(t->n - t->committed));
  t->committed += count;
  return PV_OK;
}

int pv_merkle_tree_discard(int32_t handle, uint64_t count, uint8_t* root_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (count > t->n - t->committed)
    return fail(PV_EINVAL, "expected to revert %llu txns while there are only %llu", (unsigned long long)count,
                (unsigned long long)(t->n - t->committed));
  if (const int rc = en.begin()) return rc;
  if (count) {
    const uint64_t n_new = t->n - count;
    if (const int rc = tree_edge(*t, n_new ? n_new - 1 : 0, n_new, en.s)) return rc;
  }
  return en.finish(tree_root(*t, root_out, en.s));
}

int pv_merkle_tree_sizes(int32_t handle, uint64_t* committed, uint64_t* total) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (committed) *committed = t->committed;
  if (total) *total = t->n;
  return PV_OK;
}

int pv_merkle_tree_frontier(int32_t handle, uint64_t tree_size, uint8_t* hashes_out, uint32_t* count_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (tree_size > t->n)
    return fail(PV_EINVAL, "frontier of %llu leaves outside a tree of %llu", (unsigned long long)tree_size,
                (unsigned long long)t->n);
  const uint32_t cnt = (uint32_t)__builtin_popcountll(tree_size);
  if (count_out) *count_out = cnt;
  if (cnt == 0 || !hashes_out) return PV_OK;
  if (const int rc = en.begin()) return rc;
  TmpBuf<uint8_t> dout;
  StreamDrain tail{en.s};
  HIP_OK(dout.alloc(64 * 32));
  HIP_OK(pv::launch_merkle_frontier(t->table, tree_size, w32(dout.p), en.s));
  HIP_OK(hipMemcpyAsync(hashes_out, dout.p, (size_t)cnt * 32, hipMemcpyDeviceToHost, en.s));
  return tail.finish();
}

// nodes the reference's hash store receives while leaves first + 1 .. last are appended
static uint64_t hs_nodes(uint64_t first, uint64_t last) {
  return (last - (uint64_t)__builtin_popcountll(last)) - (first - (uint64_t)__builtin_popcountll(first));
}

static int tree_hs_range(const MerkleTree& t, uint64_t first, uint64_t last) {
  if (first > last || last > t.n)
    return fail(PV_EINVAL, "leaves (%llu, %llu] outside a tree of %llu", (unsigned long long)first,
                (unsigned long long)last, (unsigned long long)t.n);
  return PV_OK;
}

static int tree_hash_store(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out, uint8_t* node_out,
                           uint64_t node_cap, uint64_t* n_nodes, bool host, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (const int rc = tree_hs_range(*t, first, last)) return rc;
  const uint64_t need = hs_nodes(first, last);
  if (n_nodes) *n_nodes = need;
  if (node_out && node_cap < need)
    return fail(PV_EINVAL, "node_cap %llu below the %llu nodes of the range", (unsigned long long)node_cap,
                (unsigned long long)need);
  if (first == last || (!leaf_out && !(node_out && need))) return PV_OK;
  if (!host && (misaligned16(leaf_out) || misaligned16(node_out)))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dleaf, dnode;
  StreamDrain tail{s};
  uint8_t *pl = leaf_out, *pn = need ? node_out : nullptr;
  if (host) {
    if (pl) {
      HIP_OK(dleaf.alloc((last - first) * 32));
      pl = dleaf.p;
    }
    if (pn) {
      HIP_OK(dnode.alloc(need * 32));
      pn = dnode.p;
    }
  }
  HIP_OK(pv::launch_merkle_hs_gather(t->table, first, last, w32(pl), w32(pn), merkle_blocks(*en.d), s));
  if (host) {
    if (pl) HIP_OK(hipMemcpyAsync(leaf_out, pl, (last - first) * 32, hipMemcpyDeviceToHost, s));
    if (pn) HIP_OK(hipMemcpyAsync(node_out, pn, need * 32, hipMemcpyDeviceToHost, s));
  }
  return tail.finish();
}

int pv_merkle_tree_hash_store(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out, uint8_t* node_out,
                              uint64_t node_cap, uint64_t* n_nodes) {
  return tree_hash_store(handle, first, last, leaf_out, node_out, node_cap, n_nodes, true, nullptr);
}

int pv_merkle_tree_hash_store_device(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out,
                                     uint8_t* node_out, uint64_t node_cap, uint64_t* n_nodes, void* stream) {
  return tree_hash_store(handle, first, last, leaf_out, node_out, node_cap, n_nodes, false, stream);
}

int pv_merkle_tree_check_nodes(int32_t handle, uint64_t first, uint64_t last, const uint8_t* node_hashes,
                               uint64_t* n_bad, uint64_t* first_bad) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (const int rc = tree_hs_range(*t, first, last)) return rc;
  if (!n_bad || !first_bad) return fail(PV_EINVAL, "null pointer");
  const uint64_t need = hs_nodes(first, last);
  *n_bad = 0;
  *first_bad = UINT64_MAX;
  if (need == 0) return PV_OK;
  if (!node_hashes) return fail(PV_EINVAL, "null buffer");
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dnodes;
  TmpBuf<unsigned long long> dres;
  StreamDrain tail{s};
  unsigned long long res[2] = {0, ~0ull};
  HIP_OK(dnodes.put(node_hashes, need * 32, s));
  HIP_OK(dres.put(res, 2, s));
  HIP_OK(pv::launch_merkle_hs_check(t->table, first, last, w32(dnodes.p), dres.p, merkle_blocks(*en.d), s));
  HIP_OK(hipMemcpyAsync(res, dres.p, sizeof(res), hipMemcpyDeviceToHost, s));
  if (const int rc = tail.finish()) return rc;
  *n_bad = res[0];
  *first_bad = res[1];
  return PV_OK;
}

}  // extern "C"
