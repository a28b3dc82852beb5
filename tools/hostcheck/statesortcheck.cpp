// HOST BUILD of the sort of state keys -- test tooling only, never loaded by the
// product (tests/test_state_sort_host.py, tests/test_gpu_state_sort.py).
//
// Compiles indy-plenum_amd/csrc/pv_trie_sort.h (unchanged) with g++ through
// statesort_host.h, so that the routines the k_trie_sort_* kernels run can be
// compared on the CPU with the Python mirror, and the GPU with both.
#include "statesort_host.h"

extern "C" {

// pv_state_sort_device's outputs over host arrays: perm (n words of room) and *m.  lsd: sort each
// round by the device's counting passes instead of std::stable_sort.  0; 1 / 2: refused for
// offsets / a key above TS_MAX_KEY_BYTES, *bad_index the first such key, perm not written;
// 3: unresolved at the round limit (a bug).  *rounds = the rounds run.
int ss_sort(const uint8_t* key_blob, const uint64_t* key_off, uint64_t n, int lsd, uint32_t* perm, uint64_t* m,
            uint32_t* rounds, uint64_t* bad_index) {
  ssoh::Sorted s;
  const int rc = ssoh::sort(key_blob, key_off, n, lsd != 0, s);
  if (bad_index) *bad_index = s.bad_index;
  if (m) *m = s.m;
  if (rounds) *rounds = s.rounds;
  if (rc) return rc;
  for (uint64_t k = 0; k < s.m; ++k) perm[k] = s.perm[k];
  return 0;
}

uint32_t ss_tile(void) { return pv::TS_TILE; }
uint64_t ss_max_key_bytes(void) { return pv::TS_MAX_KEY_BYTES; }

}  // extern "C"
