// HOST BUILD of the resident trie node store -- test tooling only, never loaded
// by the product (tests/test_state_store_host.py, tests/test_gpu_state_store.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_store.h (unchanged) with g++ through
// statestore_host.h, so that the table, the generation walk and the pack the HIP
// kernels run can be compared on the CPU with the Python mirror and with the
// fixture recorded from the reference, and the GPU with this build.
#include "statestore_host.h"

extern "C" {

void* ss_create(uint64_t node_hint) {
  ssh::Store* st = new ssh::Store();
  ssh::init(*st, node_hint);
  return st;
}

void ss_free(void* h) { delete static_cast<ssh::Store*>(h); }

// -> nodes new to the store
uint64_t ss_add(void* h, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  return ssh::add(*static_cast<ssh::Store*>(h), node_blob, node_off, n_new);
}

// raw digests as nodes without bytes: the table's edges
uint64_t ss_add_digests(void* h, const uint8_t* digests, uint64_t n_new) {
  return ssh::add_digests(*static_cast<ssh::Store*>(h), digests, n_new);
}

void ss_info(void* h, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes, uint64_t* n_slots) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  *n_nodes = st.nodes();
  *n_unique = st.n_unique;
  *n_bytes = st.n_bytes;
  *n_slots = st.table.size();
}

// id of the node with this digest, or -1
int64_t ss_find(void* h, const uint8_t* digest) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  uint32_t t[8];
  memcpy(t, digest, 32);
  const uint32_t id = pv::ts_find(st.table.data(), (uint32_t)st.table.size(), st.dig.data(), (uint32_t)st.nodes(), t);
  return id == pv::TS_ABSENT ? -1 : (int64_t)id;
}

// the slot that holds node id, or -1 (a flagged duplicate holds none)
int64_t ss_slot_of(void* h, uint32_t id) {
  const ssh::Store& st = *static_cast<ssh::Store*>(h);
  for (size_t s = 0; s < st.table.size(); ++s)
    if (st.table[s] == id + 1) return (int64_t)s;
  return -1;
}

int ss_is_dup(void* h, uint32_t id) { return static_cast<ssh::Store*>(h)->dup[id]; }

void ss_digest(void* h, uint32_t id, uint8_t* out) { memcpy(out, &static_cast<ssh::Store*>(h)->dig[8 * id], 32); }

// pv_state_store_prove with node_ids (n_queries x max_nodes) as an extra output
int ss_prove(void* h, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots, const uint8_t* key_blob,
             const uint64_t* key_off, uint64_t n_queries, uint32_t max_nodes, uint8_t* status, uint32_t* node_count,
             uint32_t* node_ids, uint64_t* proof_off, uint64_t* val_rel, uint64_t* val_len, uint8_t* proof_blob,
             uint64_t proof_cap) {
  return ssh::prove(ssh::view(*static_cast<ssh::Store*>(h)), roots, root_idx, n_roots, key_blob, key_off, n_queries,
                    max_nodes, status, node_count, node_ids, proof_off, val_rel, val_len, proof_blob, proof_cap);
}

}  // extern "C"
