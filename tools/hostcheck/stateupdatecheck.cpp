// HOST BUILD of the sets onto a committed root -- test tooling only, never loaded
// by the product (tests/test_state_update_host.py, tests/test_gpu_state_update.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_update.h and pv_trie_build.h (unchanged)
// with g++ through stateupdate_host.h, so that the routines the HIP kernels run
// can be compared on the CPU with the Python mirror and with the fixture recorded
// from the reference, and the GPU with this build.
#include "stateupdate_host.h"

extern "C" {

void* su_store_new(uint64_t node_hint) {
  ssh::Store* st = new ssh::Store();
  ssh::init(*st, node_hint);
  return st;
}

void su_store_free(void* h) { delete static_cast<ssh::Store*>(h); }

uint64_t su_store_add(void* h, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  return ssh::add(*static_cast<ssh::Store*>(h), node_blob, node_off, n_new);
}

void su_store_info(void* h, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  *n_nodes = st.nodes();
  *n_unique = st.n_unique;
  *n_bytes = st.n_bytes;
}

// pv_state_update_device's outputs over host arrays.  0; 1 / 2 / 3: refused for key order / an
// empty value / offsets; 4: a capacity is too small (root and sizes are written, no node is,
// nothing is inserted); 5: the walk of key *bad_index met a missing or malformed node
// (*status = its PV_SP_* status).  *n_items = the merged list's length (0: no merge ran).
int su_update(void* h, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
              const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* root,
              uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
              uint64_t node_cap, uint8_t* digests, uint64_t* bad_index, uint32_t* status, uint64_t* n_items) {
  ssh::Store& st = *static_cast<ssh::Store*>(h);
  sbh::Built b;
  suh::Merged m;
  const int rc = suh::update(ssh::view(st), old_root, key_blob, key_off, val_blob, val_off, n, b, m);
  if (bad_index) *bad_index = m.bad_index;
  if (status) *status = m.status;
  if (n_items) *n_items = m.items;
  if (rc) return rc;
  const int dc = sbh::deliver(b, root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests);
  if (dc) return dc;
  if (insert) suh::add_hashed(st, b);
  return 0;
}

// the merged list of a batch, for the tests that look at it: 0 or a code as above.  Sizes
// first (buffers null), then the arrays: paths (bytes, offsets, nibble counts), kinds, payloads.
int su_merge(void* h, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
             const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, uint64_t* n_items, uint64_t* path_bytes,
             uint64_t* val_bytes, uint8_t* ikey, uint64_t* ikoff, uint32_t* inib, uint8_t* ikind, uint8_t* ival,
             uint64_t* ivoff) {
  suh::Merged m;
  const int rc = suh::merge(ssh::view(*static_cast<ssh::Store*>(h)), old_root, key_blob, key_off, val_blob, val_off,
                            n, m);
  if (rc) return rc;
  *n_items = m.items;
  *path_bytes = m.ikey.size();
  *val_bytes = m.ival.size();
  if (!ikoff) return 0;
  if (!m.ikey.empty()) memcpy(ikey, m.ikey.data(), m.ikey.size());
  if (!m.ival.empty()) memcpy(ival, m.ival.data(), m.ival.size());
  memcpy(ikoff, m.ikoff.data(), 8 * (m.items + 1));
  memcpy(ivoff, m.ivoff.data(), 8 * (m.items + 1));
  memcpy(inib, m.inib.data(), 4 * m.items);
  memcpy(ikind, m.ikind.data(), m.items);
  return 0;
}

}  // extern "C"
