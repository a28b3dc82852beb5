// HOST BUILD of the Merkle proof routines -- test tooling only, never loaded
// by the product (tests/test_merkle_proofs_host.py).
//
// Compiles indy-plenum_amd/csrc/pv_merkle_proof.h with g++ so that the exact
// per-lane walks the HIP kernels run (audit-path check, consistency check,
// path and proof generation over a level-wise tree) can be compared on the CPU
// with the fixture recorded from the reference.
#include <stdint.h>
#include <string.h>

#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_merkle_proof.h"

namespace {

struct Tree {
  uint64_t n = 0;
  uint32_t depth = 0;
  std::vector<std::vector<uint32_t>> lv;
  std::vector<const uint32_t*> table;
};

// the level-wise tree k_merkle_level_keep builds: an odd last node moves up
Tree* build(const uint8_t* leaf_hashes, uint64_t n) {
  Tree* t = new Tree;
  t->n = n;
  t->lv.emplace_back(8 * n);
  if (n) memcpy(t->lv[0].data(), leaf_hashes, 32 * n);
  uint64_t m = n;
  while (m > 1) {
    const uint64_t outs = (m + 1) / 2;
    std::vector<uint32_t> nx(8 * outs);
    const std::vector<uint32_t>& in = t->lv.back();
    for (uint64_t i = 0; i < m / 2; ++i) pv::sha256_node(&nx[8 * i], &in[16 * i]);
    if (m & 1) memcpy(&nx[8 * (outs - 1)], &in[8 * (m - 1)], 32);
    t->lv.push_back(std::move(nx));
    m = outs;
  }
  t->depth = (uint32_t)t->lv.size() - 1;
  for (auto& v : t->lv) t->table.push_back(v.data());
  return t;
}

}  // namespace

extern "C" {

uint32_t mc_verify_inclusion(const uint8_t* leaf_hash, uint64_t index, uint64_t tree_size, const uint8_t* nodes,
                             uint64_t n_nodes, const uint8_t* root, uint8_t* computed, uint64_t* stop) {
  uint32_t lh[8], r[8], c[8];
  std::vector<uint32_t> nd(8 * n_nodes + 8);
  memcpy(lh, leaf_hash, 32);
  memcpy(r, root, 32);
  if (n_nodes) memcpy(nd.data(), nodes, 32 * n_nodes);
  const uint32_t st = pv::mp_verify_inclusion(lh, index, tree_size, nd.data(), n_nodes, r, c, stop);
  memcpy(computed, c, 32);
  return st;
}

uint32_t mc_verify_consistency(uint64_t old_size, uint64_t new_size, const uint8_t* old_root, const uint8_t* new_root,
                               const uint8_t* nodes, uint64_t n_nodes, uint8_t* old_computed, uint8_t* new_computed) {
  uint32_t r0[8], r1[8], c0[8], c1[8];
  std::vector<uint32_t> nd(8 * n_nodes + 8);
  memcpy(r0, old_root, 32);
  memcpy(r1, new_root, 32);
  if (n_nodes) memcpy(nd.data(), nodes, 32 * n_nodes);
  const uint32_t st = pv::mp_verify_consistency(old_size, new_size, r0, r1, nd.data(), n_nodes, c0, c1);
  memcpy(old_computed, c0, 32);
  memcpy(new_computed, c1, 32);
  return st;
}

void* mc_tree_new(const uint8_t* leaf_hashes, uint64_t n) { return build(leaf_hashes, n); }
void mc_tree_free(void* t) { delete static_cast<Tree*>(t); }
uint32_t mc_tree_depth(void* t) { return static_cast<Tree*>(t)->depth; }

// out: (depth + 1) * 32 bytes; returns the length, 0xffffffff for a request outside the tree
uint32_t mc_audit_path(void* tp, uint64_t m, uint64_t s, uint8_t* out, uint8_t* root) {
  Tree* t = static_cast<Tree*>(tp);
  if (s == 0 || s > t->n || m >= s) return pv::MP_LEN_REFUSED;
  std::vector<uint32_t> o(8 * (t->depth + 1));
  uint32_t r[8];
  const uint32_t len = pv::mp_audit_path(t->table.data(), t->n, m, s, o.data(), r);
  memcpy(out, o.data(), 32 * (size_t)len);
  memcpy(root, r, 32);
  return len;
}

uint32_t mc_cons_proof(void* tp, uint64_t a, uint64_t b, uint8_t* out) {
  Tree* t = static_cast<Tree*>(tp);
  if (a > b || b > t->n) return pv::MP_LEN_REFUSED;
  std::vector<uint32_t> o(8 * (t->depth + 1));
  const uint32_t len = pv::mp_cons_proof(t->table.data(), t->n, a, b, o.data());
  memcpy(out, o.data(), 32 * (size_t)len);
  return len;
}

}  // extern "C"
