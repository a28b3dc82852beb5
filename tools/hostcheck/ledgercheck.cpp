// HOST BUILD of the ledger write cycle -- test tooling only, never loaded by
// the product (tests/test_ledger_tree_host.py).
//
// Compiles indy-plenum_amd/csrc/pv_merkle_ledger.h with g++ so that the exact
// routines the HIP kernels run (the right-edge rebuild of stage and discard,
// the hash-store gather and check, the frontier) can be compared on the CPU
// with the fixture recorded from the reference.  The tree mirrors the C ABI's:
// committed <= n leaves, one buffer per level, sized exactly.
#include <stdint.h>
#include <string.h>

#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_merkle_ledger.h"

namespace {

const uint32_t EMPTY_ROOT[8] = {0x42c4b0e3u, 0x141cfc98u, 0xc8f4fb9au, 0x24b96f99u,
                                0xe441ae27u, 0x4c939b64u, 0x1b9995a4u, 0x55b85278u};   // SHA-256("")

struct Tree {
  uint64_t n = 0, committed = 0;
  uint32_t depth = 0;
  std::vector<std::vector<uint32_t>> lv{1};
  std::vector<uint32_t*> table;
  std::vector<const uint32_t*> ctable;
};

// level l holds exactly the nodes of n_new leaves (a prefix of what it held is kept)
void resize(Tree& t, uint64_t n_new) {
  uint32_t depth = 0;
  for (uint64_t m = n_new; m > 1; m = (m + 1) / 2) ++depth;
  if (t.lv.size() < depth + 1) t.lv.resize(depth + 1);
  for (uint32_t l = 0; l < t.lv.size(); ++l) t.lv[l].resize(l <= depth ? 8 * pv::ml_level_count(n_new, l) : 0);
  t.table.clear();
  t.ctable.clear();
  for (auto& v : t.lv) {
    t.table.push_back(v.data());
    t.ctable.push_back(v.data());
  }
}

void edge(Tree& t, uint64_t f0, uint64_t n_new) {
  std::vector<uint32_t> b0(8 * pv::ML_EDGE_BUF), b1(8 * pv::ML_EDGE_BUF);
  t.depth = pv::ml_edge_rebuild(t.table.data(), f0, n_new, b0.data(), b1.data(), 0u, 1u, [] {});
  t.n = n_new;
}

void root(const Tree& t, uint8_t* out) {
  if (out) memcpy(out, t.n ? t.lv[t.depth].data() : EMPTY_ROOT, 32);
}

}  // namespace

extern "C" {

void* lc_tree_new() { return new Tree; }
void lc_tree_free(void* t) { delete static_cast<Tree*>(t); }

// pv_merkle_tree_stage_hashes; spans above ML_EDGE_MAX go in pieces (the C ABI rebuilds per level there)
int lc_stage(void* tp, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out) {
  Tree& t = *static_cast<Tree*>(tp);
  for (uint64_t done = 0; done < k;) {
    const uint64_t step = k - done < pv::ML_EDGE_MAX ? k - done : pv::ML_EDGE_MAX;
    const uint64_t n_old = t.n;
    resize(t, n_old + step);
    memcpy(t.lv[0].data() + 8 * n_old, leaf_hashes + 32 * done, 32 * step);
    edge(t, n_old, n_old + step);
    done += step;
  }
  root(t, root_out);
  return 0;
}

int lc_commit(void* tp, uint64_t count) {
  Tree& t = *static_cast<Tree*>(tp);
  if (count > t.n - t.committed) return -22;
  t.committed += count;
  return 0;
}

int lc_discard(void* tp, uint64_t count, uint8_t* root_out) {
  Tree& t = *static_cast<Tree*>(tp);
  if (count > t.n - t.committed) return -22;
  if (count) {
    const uint64_t n_new = t.n - count;
    resize(t, n_new);
    if (n_new) edge(t, n_new - 1, n_new);
    else t.n = t.depth = 0;
  }
  root(t, root_out);
  return 0;
}

void lc_sizes(void* tp, uint64_t* committed, uint64_t* total) {
  *committed = static_cast<Tree*>(tp)->committed;
  *total = static_cast<Tree*>(tp)->n;
}

// out: popcount(size) x 32 bytes; returns the count, 0xffffffff for size > n
uint32_t lc_frontier(void* tp, uint64_t size, uint8_t* out) {
  Tree& t = *static_cast<Tree*>(tp);
  if (size > t.n) return 0xffffffffu;
  const uint32_t cnt = pv::ml_popc64(size);
  std::vector<uint32_t> o(8 * cnt + 8);
  for (uint32_t b = 0; b < 64; ++b)
    if ((size >> b) & 1) pv::ml_frontier_node(t.ctable.data(), size, b, o.data());
  memcpy(out, o.data(), 32 * (size_t)cnt);
  return cnt;
}

// leaf_out: (last - first) x 32 bytes, node_out: the returned count x 32 bytes (either may be null)
uint64_t lc_hash_store(void* tp, uint64_t first, uint64_t last, uint8_t* leaf_out, uint8_t* node_out) {
  Tree& t = *static_cast<Tree*>(tp);
  if (first > last || last > t.n) return ~0ull;
  const uint64_t need = pv::ml_nodes_upto(last) - pv::ml_nodes_upto(first);
  std::vector<uint32_t> lo(8 * (last - first)), no(8 * need);
  for (uint64_t e = first + 1; e <= last; ++e)
    pv::ml_hs_gather(t.ctable.data(), first, e, leaf_out ? lo.data() : nullptr, node_out ? no.data() : nullptr);
  if (leaf_out) memcpy(leaf_out, lo.data(), 4 * lo.size());
  if (node_out) memcpy(node_out, no.data(), 4 * no.size());
  return need;
}

uint64_t lc_check_nodes(void* tp, uint64_t first, uint64_t last, const uint8_t* nodes, uint64_t* first_bad) {
  Tree& t = *static_cast<Tree*>(tp);
  *first_bad = ~0ull;
  if (first > last || last > t.n) return ~0ull;
  const uint64_t need = pv::ml_nodes_upto(last) - pv::ml_nodes_upto(first);
  std::vector<uint32_t> nd(8 * need);
  if (need) memcpy(nd.data(), nodes, 32 * need);
  uint64_t bad = 0;
  for (uint64_t e = first + 1; e <= last; ++e) {
    uint64_t lowest = ~0ull;
    bad += pv::ml_hs_check(t.ctable.data(), first, e, nd.data(), &lowest);
    if (lowest < *first_bad) *first_bad = lowest;
  }
  return bad;
}

}  // extern "C"
