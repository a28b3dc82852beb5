// HOST BUILD of the SHA3-256 and state-proof routines -- test tooling only,
// never loaded by the product (tests/test_state_proofs_host.py).
//
// Compiles indy-plenum_amd/csrc/pv_sha3.h and pv_trie_proof.h with g++ so that
// the exact per-lane code the HIP kernels run (block assembly at any byte
// offset, the Keccak permutation, the trie walk on RLP bytes) can be compared
// on the CPU with hashlib and with the fixture recorded from the reference.
#include <stdint.h>
#include <string.h>

#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_sha3.h"
#include "../../indy-plenum_amd/csrc/pv_trie_proof.h"

extern "C" {

// SHA3-256 of blob[beg .. end) in place; the caller's blob is 4-byte aligned
// and has >= 16 readable bytes after `end` (the kernels' convention)
void sc_sha3_256(const uint8_t* blob, uint64_t beg, uint64_t end, uint8_t* out) {
  uint32_t d[8];
  pv::sha3_256_msg(d, blob + beg, end - beg);
  memcpy(out, d, 32);
}

// what pv_state_proof_verify computes: every node hashed once, then one walk
// per query.  The blob follows the convention above.
void sc_state_proof_verify(const uint8_t* node_blob, const uint64_t* node_beg, const uint64_t* node_end,
                           const uint64_t* proof_first, const uint8_t* roots, const uint32_t* proof_idx,
                           const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                           const uint64_t* val_off, uint64_t N, uint64_t P, uint64_t Q, uint8_t* status) {
  std::vector<uint32_t> dig(8 * N + 8);
  for (uint64_t j = 0; j < N; ++j) pv::sha3_256_msg(&dig[8 * j], node_blob + node_beg[j], node_end[j] - node_beg[j]);
  for (uint64_t i = 0; i < Q; ++i) {
    const uint64_t p = proof_idx[i];
    uint32_t st = pv::SP_MALFORMED;
    if (p < P) {
      uint32_t r[8];
      memcpy(r, roots + 32 * p, 32);
      st = pv::sp_verify(node_blob, node_beg, node_end, dig.data(), proof_first[p], proof_first[p + 1], r,
                         key_blob + key_off[i], key_off[i + 1] - key_off[i], val_blob + val_off[i],
                         val_off[i + 1] - val_off[i]);
    }
    status[i] = (uint8_t)st;
  }
}

// pv_rlp_split_list's logic: 0 on success, -22 otherwise
int sc_rlp_split_list(const uint8_t* rlp, uint64_t len, uint64_t* item_beg, uint64_t* item_end, uint64_t cap,
                      uint64_t* count) {
  return pv::rlp_split_list(rlp, len, item_beg, item_end, cap, count) ? 0 : -22;
}

}  // extern "C"
