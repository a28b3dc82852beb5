// Stand-alone self-check of indy-plenum_amd/csrc/pv_merkle_proof.h, meant to
// be built with -fsanitize=address,undefined (make merklecheck_asan) and run
// as its own process (tests/test_merkle_proofs_host.py).
//
// Trees of 1..130 leaves are built level-wise with the header's own SHA-256.
// For every tree every audit path and consistency proof at the full size, and
// for the largest tree every (m, s) and (a, b) below it too, is generated with
// mp_audit_path / mp_cons_proof into buffers of exactly depth + 1 nodes,
// checked against the recursive RFC 6962 definition of the tree hash, verified
// with mp_verify_inclusion / mp_verify_consistency, and verified again with
// one bit flipped.  Exit status 1 on any disagreement.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_merkle_proof.h"

namespace {

typedef std::vector<uint32_t> Words;
int g_bad = 0;
uint64_t g_paths = 0, g_proofs = 0;

void bad(const char* what, uint64_t n, uint64_t a, uint64_t b) {
  if (++g_bad <= 20) fprintf(stderr, "FAIL %s: tree %llu, (%llu, %llu)\n", what, (unsigned long long)n,
                             (unsigned long long)a, (unsigned long long)b);
}

// RFC 6962 section 2.1: MTH(D[lo:hi]), split at the largest power of two below the width
void mth(uint32_t out[8], const Words& leaves, uint64_t lo, uint64_t hi) {
  if (hi - lo == 1) {
    memcpy(out, &leaves[8 * lo], 32);
    return;
  }
  uint64_t k = 1;
  while (2 * k < hi - lo) k *= 2;
  uint32_t lr[16];
  mth(lr, leaves, lo, lo + k);
  mth(lr + 8, leaves, lo + k, hi);
  pv::sha256_node(out, lr);
}

uint32_t path_length(uint64_t index, uint64_t size) {   // MerkleVerifier.audit_path_length
  uint32_t len = 0;
  for (uint64_t last = size - 1; last > 0; index >>= 1, last >>= 1)
    if ((index & 1) || index < last) ++len;
  return len;
}

struct Tree {
  uint64_t n;
  uint32_t depth;
  std::vector<Words> lv;
  std::vector<const uint32_t*> table;
};

void build(Tree& t, const Words& leaves, uint64_t n) {
  t.n = n;
  t.lv.clear();
  t.table.clear();
  t.lv.emplace_back(leaves.begin(), leaves.begin() + 8 * n);
  for (uint64_t m = n; m > 1; m = (m + 1) / 2) {
    const Words& in = t.lv.back();
    Words nx(8 * ((m + 1) / 2));
    for (uint64_t i = 0; i < m / 2; ++i) pv::sha256_node(&nx[8 * i], &in[16 * i]);
    if (m & 1) memcpy(&nx[8 * (m / 2)], &in[8 * (m - 1)], 32);
    t.lv.push_back(std::move(nx));
  }
  t.depth = (uint32_t)t.lv.size() - 1;
  for (auto& v : t.lv) t.table.push_back(v.data());
}

void check_path(const Tree& t, const Words& leaves, const std::vector<Words>& roots, uint64_t m, uint64_t s) {
  ++g_paths;
  Words out(8 * (t.depth + 1));   // exactly the stride the kernels get
  uint32_t root[8], comp[8];
  uint64_t stop = 0;
  const uint32_t len = pv::mp_audit_path(t.table.data(), t.n, m, s, out.data(), root);
  if (len != path_length(m, s)) bad("path length", t.n, m, s);
  if (memcmp(root, roots[s].data(), 32)) bad("path root", t.n, m, s);
  Words exact(out.begin(), out.begin() + 8 * len);   // no slack behind the proof
  exact.resize(8 * len + (len ? 0 : 8));
  if (pv::mp_verify_inclusion(&leaves[8 * m], m, s, exact.data(), len, roots[s].data(), comp, &stop) != pv::MP_OK)
    bad("path verify", t.n, m, s);
  if (memcmp(comp, roots[s].data(), 32)) bad("path computed", t.n, m, s);
  if (len) {
    exact[(m * 7 + s) % (8 * len)] ^= 1u << ((m + s) % 32);
    if (pv::mp_verify_inclusion(&leaves[8 * m], m, s, exact.data(), len, roots[s].data(), comp, &stop) !=
        pv::MP_ROOT_MISMATCH)
      bad("mutated path accepted", t.n, m, s);
    if (pv::mp_verify_inclusion(&leaves[8 * m], m, s, exact.data(), len - 1, roots[s].data(), comp, &stop) !=
        pv::MP_TOO_SHORT)
      bad("short path accepted", t.n, m, s);
  } else {
    uint32_t lh[8];
    memcpy(lh, &leaves[8 * m], 32);
    lh[0] ^= 1;
    if (pv::mp_verify_inclusion(lh, m, s, exact.data(), 0, roots[s].data(), comp, &stop) != pv::MP_ROOT_MISMATCH)
      bad("mutated leaf accepted", t.n, m, s);
  }
}

void check_proof(const Tree& t, const std::vector<Words>& roots, uint64_t a, uint64_t b) {
  ++g_proofs;
  Words out(8 * (t.depth + 1));
  uint32_t c0[8], c1[8];
  const uint32_t len = pv::mp_cons_proof(t.table.data(), t.n, a, b, out.data());
  if ((a == 0 || a == b) && len) bad("proof not empty", t.n, a, b);
  Words exact(out.begin(), out.begin() + 8 * len);
  exact.resize(8 * len + (len ? 0 : 8));
  const uint32_t* r0 = roots[a ? a : b].data();   // a == 0: any old root passes
  if (pv::mp_verify_consistency(a, b, r0, roots[b].data(), exact.data(), len, c0, c1) != pv::MP_OK)
    bad("proof verify", t.n, a, b);
  if (len) {
    exact[(a * 5 + b) % (8 * len)] ^= 1u << ((a + b) % 32);
    if (pv::mp_verify_consistency(a, b, r0, roots[b].data(), exact.data(), len, c0, c1) == pv::MP_OK)
      bad("mutated proof accepted", t.n, a, b);
    if (pv::mp_verify_consistency(a, b, r0, roots[b].data(), exact.data(), len - 1, c0, c1) != pv::MP_TOO_SHORT)
      bad("short proof accepted", t.n, a, b);
  }
}

}  // namespace

int main() {
  const uint64_t N = 130;
  // leaf i = SHA-256(0x00 || "leaf-<i>"), by the header's own message hasher
  // (it reads up to 15 bytes past a message: the text buffer is padded)
  Words leaves(8 * N);
  for (uint64_t i = 0; i < N; ++i) {
    uint8_t text[64] = {0};
    const int len = snprintf(reinterpret_cast<char*>(text), 32, "leaf-%llu", (unsigned long long)i);
    pv::sha256_msg(&leaves[8 * i], text, (uint64_t)len, 1, 0x00);
  }
  std::vector<Words> roots(N + 1, Words(8));
  for (uint64_t s = 1; s <= N; ++s) mth(roots[s].data(), leaves, 0, s);
  Tree t;
  for (uint64_t n = 1; n <= N; ++n) {
    build(t, leaves, n);
    if (memcmp(t.lv[t.depth].data(), roots[n].data(), 32)) bad("tree root", n, 0, n);
    for (uint64_t s = (n == N ? 1 : n); s <= n; ++s)
      for (uint64_t m = 0; m < s; ++m) check_path(t, leaves, roots, m, s);
    for (uint64_t b = (n == N ? 1 : n); b <= n; ++b)
      for (uint64_t a = 0; a <= b; ++a) check_proof(t, roots, a, b);
  }
  // range refusals and the early decisions of the consistency check
  uint32_t c0[8], c1[8];
  uint64_t stop = 0;
  Words none(8);
  if (pv::mp_verify_inclusion(&leaves[0], 5, 5, none.data(), 0, roots[5].data(), c0, &stop) != pv::MP_BAD_RANGE)
    bad("index == tree_size", 5, 5, 5);
  if (pv::mp_verify_inclusion(&leaves[0], 0, 0, none.data(), 0, roots[5].data(), c0, &stop) != pv::MP_BAD_RANGE)
    bad("tree_size == 0", 0, 0, 0);
  if (pv::mp_verify_consistency(6, 5, roots[6].data(), roots[5].data(), none.data(), 0, c0, c1) != pv::MP_BAD_RANGE)
    bad("old > new", 6, 6, 5);
  if (pv::mp_verify_consistency(5, 5, roots[5].data(), roots[6].data(), none.data(), 0, c0, c1) != pv::MP_INCONSISTENT)
    bad("equal sizes, different roots", 5, 5, 5);
  printf("merklecheck: %llu paths, %llu proofs, %d failures\n", (unsigned long long)g_paths,
         (unsigned long long)g_proofs, g_bad);
  return g_bad ? 1 : 0;
}
