// HOST BUILD of the sets and removals onto a committed root -- test tooling only, never
// loaded by the product (tests/test_state_apply_host.py, tests/test_gpu_state_apply.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_update.h and pv_trie_build.h (unchanged)
// with g++ through stateupdate_host.h in its removal mode (tb_lcp_one admitting an
// empty value, tu_walk_t<true>), so that the routines k_trie_apply_count /
// k_trie_apply_emit run can be compared on the CPU with the Python mirror and with
// the fixture recorded from the reference, and the GPU with this build.
#include "stateupdate_host.h"

extern "C" {

void* sa_store_new(uint64_t node_hint) {
  ssh::Store* st = new ssh::Store();
  ssh::init(*st, node_hint);
  return st;
}

void sa_store_free(void* h) { delete static_cast<ssh::Store*>(h); }

uint64_t sa_store_add(void* h, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  return ssh::add(*static_cast<ssh::Store*>(h), node_blob, node_off, n_new);
}

void sa_store_info(void* h, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  *n_nodes = st.nodes();
  *n_unique = st.n_unique;
  *n_bytes = st.n_bytes;
}

// pv_state_apply_device's outputs over host arrays, or, with removals == 0, pv_state_update_device's
// (the same store, for the comparison of the two).  0; 1 / 2 / 3: refused for key order / a value
// / offsets; 4: a capacity is too small (root and sizes are written, no node is, nothing is
// inserted); 5: the walk of key *bad_index met a missing or malformed node (*status = its PV_SP_*
// status).  *n_items = the merged list's length (0: no merge ran, or nothing is left).
int sa_apply(void* h, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
             const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, int removals, uint8_t* root,
             uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
             uint64_t node_cap, uint8_t* digests, uint64_t* bad_index, uint32_t* status, uint64_t* n_items) {
  ssh::Store& st = *static_cast<ssh::Store*>(h);
  sbh::Built b;
  suh::Merged m;
  const int rc = suh::update(ssh::view(st), old_root, key_blob, key_off, val_blob, val_off, n, b, m, removals != 0);
  if (bad_index) *bad_index = m.bad_index;
  if (status) *status = m.status;
  if (n_items) *n_items = m.items;
  if (rc) return rc;
  const int dc = sbh::deliver(b, root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests);
  if (dc) return dc;
  if (insert) suh::add_hashed(st, b);
  return 0;
}

}  // extern "C"
