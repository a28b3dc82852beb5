// The batch trie build on the host -- test tooling only.  It includes the
// product header indy-plenum_amd/csrc/pv_trie_build.h unchanged and runs what
// the kernels of pv_state_build_device run, sequentially and in the same order:
// tb_lcp_one per position, the min tree level by level, tb_struct_one per key,
// tb_size_one per level (deepest first), the two exclusive scans, tb_emit_one
// per level (deepest first).  Every work array has its exact size.  Shared by
// libstatebuildcheck.so and statebuildcheck_asan.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#ifndef PV_HD
#define PV_HD static inline
#endif
#include "../../indy-plenum_amd/csrc/pv_sha3.h"
#include "../../indy-plenum_amd/csrc/pv_trie_build.h"

namespace sbh {

enum { OK = 0, BAD_ORDER = 1, BAD_VALUE = 2, BAD_OFFSET = 3, TOO_SMALL = 4 };

struct Built {
  std::vector<uint8_t> blob;    // n_bytes + 16 (the over-read contract of pv_sha3.h)
  std::vector<uint64_t> off;    // n_nodes + 1
  std::vector<uint32_t> dig;    // 8 n_nodes
  uint8_t root[32];
  uint64_t n_nodes = 0, n_bytes = 0, bad_index = 0;
  uint32_t max_level = 0;
};

inline int build(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                 uint64_t n, Built& out, const uint32_t* knib = nullptr, const uint8_t* kind = nullptr) {
  out = Built();
  if (n == 0) {
    alignas(16) uint8_t blank[32] = {0x80};   // the message and the bytes the hash may read past it
    uint32_t d[8];
    pv::sha3_256_msg(d, blank, 1);
    memcpy(out.root, d, 32);
    out.blob.assign(16, 0);
    out.off.assign(1, 0);
    return OK;
  }
  uint64_t lvoff[pv::TB_MAX_LEVELS + 1];
  pv::TbCtx c{};
  c.key_blob = key_blob;
  c.key_off = key_off;
  c.val_blob = val_blob;
  c.val_off = val_off;
  c.n = n;
  c.knib = knib;   // a merged item list (stateupdate_host.h), else null
  c.kind = kind;
  c.nlv = pv::tb_tree_layout(n, lvoff);
  c.lvoff = lvoff;
  std::vector<uint32_t> tree(lvoff[c.nlv]), child(16 * n, 0), lvl(3 * n), aux(3 * n), elen(3 * n, 0);
  std::vector<uint64_t> off(3 * n + 1, 0), idx(3 * n + 1, 0);
  std::vector<uint8_t> inl(32 * 3 * n);
  uint32_t root_e = 0;
  c.tree = tree.data();
  c.child = child.data();
  c.lvl = lvl.data();
  c.aux = aux.data();
  c.elen = elen.data();
  c.off = off.data();
  c.idx = idx.data();
  c.inl = inl.data();
  c.root_e = &root_e;
  uint32_t maxh = 0;
  uint64_t bad_at[3] = {n + 1, n + 1, n + 1};   // first index per kind: order, value, offset
  for (uint64_t i = 0; i <= n; ++i) {
    uint32_t bad;
    const uint32_t h = pv::tb_lcp_one(c, i, bad);
    tree[i] = h;
    if (h > maxh) maxh = h;
    for (int k = 0; k < 3; ++k)
      if ((bad >> k & 1) && i < bad_at[k]) bad_at[k] = i;
  }
  if (bad_at[2] <= n) return out.bad_index = bad_at[2], BAD_OFFSET;
  if (bad_at[1] <= n) return out.bad_index = bad_at[1], BAD_VALUE;
  if (bad_at[0] <= n) return out.bad_index = bad_at[0], BAD_ORDER;
  for (uint32_t lv = 1; lv < c.nlv; ++lv)
    for (uint64_t j = 0; j < lvoff[lv + 1] - lvoff[lv]; ++j) pv::tb_min_one(c, lv, j);
  for (uint64_t i = 0; i < n; ++i)
    if (const uint32_t r = pv::tb_struct_one(c, i)) root_e = r - 1;
  const uint32_t ents = (uint32_t)(3 * n);
  for (uint32_t lv = maxh + 1; lv-- > 0;)
    for (uint32_t e = 0; e < ents; ++e)
      if (lvl[e] == lv) pv::tb_size_one(c, e);
  uint64_t bytes = 0, nodes = 0;
  for (uint32_t e = 0; e <= ents; ++e) {   // the exclusive scans; entry 3 n is the total
    const uint64_t b = off[e], k = idx[e];
    off[e] = bytes;
    idx[e] = nodes;
    bytes += b;
    nodes += k;
  }
  out.n_nodes = nodes;
  out.n_bytes = bytes;
  out.max_level = maxh;
  out.blob.assign(bytes + 16, 0);
  out.off.assign(nodes + 1, 0);
  out.dig.assign(8 * nodes, 0);
  c.out_blob = out.blob.data();
  c.node_off = out.off.data();
  c.dig = out.dig.data();
  for (uint32_t lv = maxh + 1; lv-- > 0;)
    for (uint32_t e = 0; e < ents; ++e)
      if (lvl[e] == lv) pv::tb_emit_one(c, e);
  out.off[nodes] = bytes;
  memcpy(out.root, &out.dig[8 * idx[root_e]], 32);
  return OK;
}

// The outputs of pv_state_build_device from a Built: sizes always; nodes only
// when the capacity of every output that is given suffices -- blob_cap for
// node_blob, node_cap for node_off and digests (TOO_SMALL otherwise, nothing
// written).
inline int deliver(const Built& b, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
                   uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests) {
  memcpy(root, b.root, 32);
  *n_nodes = b.n_nodes;
  *n_bytes = b.n_bytes;
  if (!node_blob && !node_off && !digests) return OK;
  if ((node_blob && blob_cap < b.n_bytes) || ((node_off || digests) && node_cap < b.n_nodes)) return TOO_SMALL;
  if (node_blob && b.n_bytes) memcpy(node_blob, b.blob.data(), b.n_bytes);
  if (node_off) memcpy(node_off, b.off.data(), 8 * (b.n_nodes + 1));
  if (digests && b.n_nodes) memcpy(digests, b.dig.data(), 32 * b.n_nodes);
  return OK;
}

}  // namespace sbh
