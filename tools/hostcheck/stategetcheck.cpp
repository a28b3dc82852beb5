// HOST BUILD of the reads from the resident trie node store -- test tooling only,
// never loaded by the product (tests/test_state_get_host.py, tests/test_gpu_state_get.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_get.h (unchanged) with g++ through
// stateget_host.h, so that the read walk, the decode and the copy the HIP kernels
// run can be compared on the CPU with the Python mirror and with the fixtures
// recorded from the reference, and the GPU with this build.
#include "stateget_host.h"

extern "C" {

void* sgc_create(uint64_t node_hint) {
  ssh::Store* st = new ssh::Store();
  ssh::init(*st, node_hint);
  return st;
}

void sgc_free(void* h) { delete static_cast<ssh::Store*>(h); }

uint64_t sgc_add(void* h, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  return ssh::add(*static_cast<ssh::Store*>(h), node_blob, node_off, n_new);
}

// pv_state_store_get
int sgc_get(void* h, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots, const uint8_t* key_blob,
            const uint64_t* key_off, uint64_t n_queries, int32_t decode, uint8_t* status, uint8_t* found,
            uint64_t* val_off, uint8_t* val_blob, uint64_t val_cap) {
  std::vector<uint64_t> src(n_queries ? n_queries : 1);
  return sgh::get(ssh::view(*static_cast<ssh::Store*>(h)), roots, root_idx, n_roots, key_blob, key_off, n_queries,
                  decode, status, found, src.data(), val_off, val_blob, val_cap);
}

// tg_decode over value[0 .. len): 1 and the payload range, or 0
int sgc_decode(const uint8_t* value, uint64_t len, uint64_t* pb, uint64_t* pe) {
  *pb = *pe = 0;
  return pv::tg_decode(value, 0, len, *pb, *pe) ? 1 : 0;
}

}  // extern "C"
