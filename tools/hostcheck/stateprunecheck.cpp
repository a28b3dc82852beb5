// HOST BUILD of the store prune -- test tooling only, never loaded by the product
// (tests/test_state_prune_host.py, tests/test_gpu_state_prune.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_prune.h (unchanged) with g++ through
// stateprune_host.h, so that the mark rule and the compaction the HIP kernels
// run can be compared on the CPU with the Python mirror and with the fixtures
// recorded from the reference, and the GPU with this build.
#include "stateprune_host.h"

extern "C" {

void* pr_store_new(uint64_t node_hint) {
  ssh::Store* st = new ssh::Store();
  ssh::init(*st, node_hint);
  return st;
}

void pr_store_free(void* h) { delete static_cast<ssh::Store*>(h); }

uint64_t pr_store_add(void* h, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  return ssh::add(*static_cast<ssh::Store*>(h), node_blob, node_off, n_new);
}

void pr_store_info(void* h, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes, uint64_t* n_slots) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  *n_nodes = st.nodes();
  *n_unique = st.n_unique;
  *n_bytes = st.n_bytes;
  *n_slots = st.table.size();
}

// the store's arrays: blob (n_bytes), beg / end (n_nodes), dig (n_nodes x 32 bytes), dup (n_nodes)
void pr_store_dump(void* h, uint8_t* blob, uint64_t* beg, uint64_t* end, uint8_t* dig, uint8_t* dup) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  const uint64_t n = st.nodes();
  if (st.n_bytes) memcpy(blob, st.blob.data(), st.n_bytes);
  if (n) {
    memcpy(beg, st.beg.data(), 8 * n);
    memcpy(end, st.end.data(), 8 * n);
    memcpy(dig, st.dig.data(), 32 * n);
    memcpy(dup, st.dup.data(), n);
  }
}

// the 16 bytes after the last node (the over-read contract) are all zero
int pr_store_tail_zero(void* h) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  if (st.blob.size() != st.n_bytes + 16) return 0;
  for (int k = 0; k < 16; ++k)
    if (st.blob[st.n_bytes + k]) return 0;
  return 1;
}

int pr_prune(void* h, const uint8_t* roots, uint64_t n_roots, int apply, uint8_t* root_status, uint64_t* n_kept,
             uint64_t* bytes_kept, uint64_t* n_missing, uint8_t* kept_digests, uint64_t digest_cap,
             uint64_t* bad_root) {
  return sph::prune(*static_cast<ssh::Store*>(h), roots, n_roots, apply, root_status, n_kept, bytes_kept, n_missing,
                    kept_digests, digest_cap, bad_root);
}

}  // extern "C"
