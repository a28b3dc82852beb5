// Reads from the resident trie node store on the host -- test tooling only.  It
// includes the product header indy-plenum_amd/csrc/pv_trie_get.h unchanged and
// runs what the kernels run, sequentially: tg_get per query (k_trie_get), the
// exclusive scan of the lengths and tg_copy_group for every member of every
// value's lane group (k_trie_get_copy).  Shared by libstategetcheck.so and
// stategetcheck_asan.
#pragma once
#include "statestore_host.h"
#include "../../indy-plenum_amd/csrc/pv_trie_get.h"

namespace sgh {

// pv_state_store_get on the host; src (n_queries) is the scratch the device keeps.  0, -22 when
// decode is not 0 or 1, or when val_blob is given and val_cap is below the values' bytes (val_off
// and the rest are written).
inline int get(const ssh::View& v, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
               const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, int32_t decode, uint8_t* status,
               uint8_t* found, uint64_t* src, uint64_t* val_off, uint8_t* val_blob, uint64_t val_cap) {
  if (decode != 0 && decode != 1) return -22;
  for (uint64_t q = 0; q < n_queries; ++q) {
    const uint64_t p = root_idx ? root_idx[q] : q;
    pv::TgResult r;
    r.status = pv::SP_MALFORMED;
    r.found = 0;
    r.beg = r.len = 0;
    if (p < n_roots) {
      uint32_t rt[8];
      memcpy(rt, roots + 32 * p, 32);
      pv::tg_get(v.blob, v.beg, v.end, v.dig, v.table, v.slots, v.n_nodes, rt, key_blob + key_off[q],
                 key_off[q + 1] - key_off[q], decode != 0, r);
    }
    status[q] = (uint8_t)r.status;
    found[q] = (uint8_t)r.found;
    src[q] = r.beg;
    val_off[q] = r.len;
  }
  uint64_t run = 0;   // the exclusive scan, in place
  for (uint64_t q = 0; q < n_queries; ++q) {
    const uint64_t len = val_off[q];
    val_off[q] = run;
    run += len;
  }
  val_off[n_queries] = run;
  if (!val_blob) return 0;
  if (val_cap < run) return -22;
  for (uint64_t q = 0; q < n_queries; ++q)
    for (uint32_t lane = 0; lane < pv::TG_GROUP; ++lane) pv::tg_copy_group(v.blob, src, val_off, q, lane, val_blob);
  return 0;
}

}  // namespace sgh
