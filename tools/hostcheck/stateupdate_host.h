// Sets onto a committed root on the host -- test tooling only.  It includes the
// product header indy-plenum_amd/csrc/pv_trie_update.h unchanged and runs what
// pv_state_update_device runs, sequentially and in the same order: tb_lcp_one
// over the batch (its checks and h[]), tu_walk per key in count mode, the three
// exclusive scans, tu_walk per key in write mode, then the build of
// statebuild_host.h over the merged items.  Every work array has its exact
// size.  Shared by libstateupdatecheck.so and stateupdatecheck_asan, and, with
// `removals` (what pv_state_apply_device runs: tb_lcp_one admits an empty value
// and the walk is tu_walk_t<true> if the batch holds one), by libstateapplycheck.so and
// stateapplycheck_asan.
#pragma once
#include "statebuild_host.h"
#include "statestore_host.h"
#include "../../indy-plenum_amd/csrc/pv_trie_update.h"

namespace suh {

enum { OK = 0, BAD_ORDER = 1, BAD_VALUE = 2, BAD_OFFSET = 3, TOO_SMALL = 4, BAD_WALK = 5, TOO_MANY = 6 };

struct Merged {
  std::vector<uint8_t> ikey, ival, ikind;   // ikey / ival: the exact bytes, no spare ones
  std::vector<uint64_t> ikoff, ivoff;
  std::vector<uint32_t> inib;
  uint64_t items = 0, bad_index = 0;
  uint32_t status = 0;
};

// the merge alone: the batch (sorted, distinct; checked here as the device form checks it)
// against the trie at old_root (not the blank root) in the store
inline int merge(const ssh::View& v, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                 const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, Merged& m, bool removals = false) {
  m = Merged();
  pv::TbCtx b{};
  uint32_t empty_seen = 0;
  if (removals) b.empty_seen = &empty_seen;
  b.key_blob = key_blob;
  b.key_off = key_off;
  b.val_blob = val_blob;
  b.val_off = val_off;
  b.n = n;
  std::vector<uint32_t> h(n + 1);
  uint64_t bad_at[3] = {n + 1, n + 1, n + 1};
  for (uint64_t i = 0; i <= n; ++i) {
    uint32_t bad;
    h[i] = pv::tb_lcp_one(b, i, bad);
    for (int k = 0; k < 3; ++k)
      if ((bad >> k & 1) && i < bad_at[k]) bad_at[k] = i;
  }
  if (bad_at[2] <= n) return m.bad_index = bad_at[2], BAD_OFFSET;
  if (bad_at[1] <= n) return m.bad_index = bad_at[1], BAD_VALUE;
  if (bad_at[0] <= n) return m.bad_index = bad_at[0], BAD_ORDER;
  uint32_t root[8];
  memcpy(root, old_root, 32);
  pv::TuCtx c{};
  c.blob = v.blob;
  c.beg = v.beg;
  c.end = v.end;
  c.dig = v.dig;
  c.table = v.table;
  c.slots = v.slots;
  c.n_nodes = v.n_nodes;
  c.root = root;
  c.key_blob = key_blob;
  c.key_off = key_off;
  c.val_blob = val_blob;
  c.val_off = val_off;
  c.n = n;
  c.h = h.data();
  std::vector<uint64_t> cnt(n + 1, 0), pbytes(n + 1, 0), vbytes(n + 1, 0);
  std::vector<uint8_t> status(n, 0);
  c.cnt = cnt.data();
  c.pbytes = pbytes.data();
  c.vbytes = vbytes.data();
  c.status = status.data();
  const bool opening = removals && empty_seen != 0;   // no removal in the batch: the walk of a batch of sets
  for (uint64_t j = 0; j < n; ++j)
    status[j] = (uint8_t)(opening ? pv::tu_walk_t<true>(c, j, false) : pv::tu_walk(c, j, false));
  for (uint64_t j = 0; j < n; ++j)
    if (status[j] != pv::SP_OK) return m.bad_index = j, m.status = status[j], BAD_WALK;
  uint64_t tot[3] = {0, 0, 0};
  for (uint64_t j = 0; j <= n; ++j) {   // the exclusive scans; entry n is the total
    const uint64_t a = cnt[j], p = pbytes[j], q = vbytes[j];
    cnt[j] = tot[0];
    pbytes[j] = tot[1];
    vbytes[j] = tot[2];
    tot[0] += a;
    tot[1] += p;
    tot[2] += q;
  }
  if (tot[0] > pv::TB_MAX_KEYS) return TOO_MANY;
  m.items = tot[0];
  m.ikey.assign(tot[1], 0xee);
  m.ival.assign(tot[2], 0xee);
  m.ikoff.assign(m.items + 1, 0);
  m.ivoff.assign(m.items + 1, 0);
  m.inib.assign(m.items, 0);
  m.ikind.assign(m.items, 0xee);
  m.ikoff[m.items] = tot[1];
  m.ivoff[m.items] = tot[2];
  c.ikey = m.ikey.data();
  c.ikoff = m.ikoff.data();
  c.ival = m.ival.data();
  c.ivoff = m.ivoff.data();
  c.inib = m.inib.data();
  c.ikind = m.ikind.data();
  for (uint64_t j = 0; j < n; ++j) (void)(opening ? pv::tu_walk_t<true>(c, j, true) : pv::tu_walk(c, j, true));
  return OK;
}

// the tail of pv_state_update with insert: the emitted nodes appended with the build's digests
inline void add_hashed(ssh::Store& st, const sbh::Built& b) {
  if (b.n_nodes == 0) return;
  const uint64_t first = st.nodes(), base = st.n_bytes;
  st.blob.resize(base + b.n_bytes + 16);
  memcpy(st.blob.data() + base, b.blob.data(), b.n_bytes);
  memset(st.blob.data() + base + b.n_bytes, 0, 16);
  st.n_bytes += b.n_bytes;
  st.dig.resize(8 * (first + b.n_nodes));
  memcpy(&st.dig[8 * first], b.dig.data(), 32 * b.n_nodes);
  for (uint64_t i = 0; i < b.n_nodes; ++i) {
    st.beg.push_back(base + b.off[i]);
    st.end.push_back(base + b.off[i + 1]);
  }
  (void)ssh::insert_new(st, first, b.n_nodes);
}

// pv_state_update_device up to the delivery: out.root / n_nodes / n_bytes and the nodes
inline int update(const ssh::View& v, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                  const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, sbh::Built& out, Merged& m,
                  bool removals = false) {
  sbh::Built blank;
  (void)sbh::build(nullptr, nullptr, nullptr, nullptr, 0, blank);
  m = Merged();
  if (n == 0) {
    out = blank;
    memcpy(out.root, old_root, 32);
    return OK;
  }
  if (memcmp(old_root, blank.root, 32) == 0 && !removals) {
    const int rc = sbh::build(key_blob, key_off, val_blob, val_off, n, out);
    m.bad_index = out.bad_index;
    return rc;
  }
  if (memcmp(old_root, blank.root, 32) == 0) {   // the batch's checks, then the build of the pairs that are no removal
    pv::TbCtx b{};
    b.key_blob = key_blob;
    b.key_off = key_off;
    b.val_blob = val_blob;
    b.val_off = val_off;
    b.n = n;
    uint32_t empty_seen = 0;
    b.empty_seen = &empty_seen;
    uint64_t bad_at[3] = {n + 1, n + 1, n + 1};
    for (uint64_t i = 0; i <= n; ++i) {
      uint32_t bad;
      (void)pv::tb_lcp_one(b, i, bad);
      for (int k = 0; k < 3; ++k)
        if ((bad >> k & 1) && i < bad_at[k]) bad_at[k] = i;
    }
    out = sbh::Built();
    if (bad_at[2] <= n) return m.bad_index = bad_at[2], BAD_OFFSET;
    if (bad_at[1] <= n) return m.bad_index = bad_at[1], BAD_VALUE;
    if (bad_at[0] <= n) return m.bad_index = bad_at[0], BAD_ORDER;
    std::vector<uint8_t> kb, vb;
    std::vector<uint64_t> ko(1, 0), vo(1, 0);
    for (uint64_t i = 0; i < n; ++i) {
      if (val_off[i + 1] == val_off[i]) continue;
      kb.insert(kb.end(), key_blob + key_off[i], key_blob + key_off[i + 1]);
      vb.insert(vb.end(), val_blob + val_off[i], val_blob + val_off[i + 1]);
      ko.push_back(kb.size());
      vo.push_back(vb.size());
    }
    const int rc = sbh::build(kb.data(), ko.data(), vb.data(), vo.data(), ko.size() - 1, out);
    m.bad_index = out.bad_index;
    return rc;
  }
  if (const int rc = merge(v, old_root, key_blob, key_off, val_blob, val_off, n, m, removals)) {
    out = sbh::Built();
    return rc;
  }
  if (m.items == 0) {   // every key of the state removed: the blank root, no node
    out = blank;
    return OK;
  }
  if (sbh::build(m.ikey.data(), m.ikoff.data(), m.ival.data(), m.ivoff.data(), m.items, out, m.inib.data(),
                 m.ikind.data()) != sbh::OK) {
    m.bad_index = out.bad_index;
    out = sbh::Built();
    return TOO_MANY;   // the merged list is not one a build takes: never
  }
  return OK;
}

}  // namespace suh
