// HOST BUILD of the batch trie build -- test tooling only, never loaded by the
// product (tests/test_state_build_host.py, tests/test_gpu_state_build.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_build.h (unchanged) with g++ through
// statebuild_host.h, so that the routines the HIP kernels run can be compared on
// the CPU with the Python mirror and with the fixture recorded from the
// reference, and the GPU with this build.
#include "statebuild_host.h"

extern "C" {

// pv_state_build_device's outputs over host arrays.  0; 1 / 2 / 3: refused for
// key order / an empty value / offsets, *bad_index = the first offending index;
// 4: a capacity is too small (root and sizes are written, no node is).
int sb_build(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
             uint64_t n, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap,
             uint64_t* node_off, uint64_t node_cap, uint8_t* digests, uint64_t* bad_index, uint32_t* max_level) {
  sbh::Built b;
  const int rc = sbh::build(key_blob, key_off, val_blob, val_off, n, b);
  if (bad_index) *bad_index = b.bad_index;
  if (max_level) *max_level = b.max_level;
  if (rc) return rc;
  return sbh::deliver(b, root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests);
}

}  // extern "C"
