// Stand-alone self-check of indy-plenum_amd/csrc/pv_merkle_ledger.h, meant to
// be built with -fsanitize=address,undefined (make ledgercheck_asan) and run
// as its own process (tests/test_ledger_tree_host.py).
//
// 1. For every (n_old, n_new) in 0..130 x 0..130 the edge rebuild (stage for
//    n_new > n_old, discard for n_new < n_old, the idle repair for n_new ==
//    n_old) runs into level buffers of exactly the nodes of n_new leaves, from
//    the levels of n_old leaves; every level is compared with a level-wise
//    build and the root with the recursive RFC 6962 definition.
// 2. For every size <= 130 and every (first, last] the hash-store order and the
//    frontier are compared with an append-by-append simulation of
//    CompactMerkleTree (a stack of full subtrees, one carry per trailing one
//    bit), into outputs of exactly the reported size; the check routine is
//    clean on them and names a flipped node.
// Exit status 1 on any disagreement.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_merkle_ledger.h"

namespace {

typedef std::vector<uint32_t> Words;
int g_bad = 0;
uint64_t g_edges = 0, g_ranges = 0;

void bad(const char* what, uint64_t a, uint64_t b, uint64_t c) {
  if (++g_bad <= 20)
    fprintf(stderr, "FAIL %s: (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c);
}

// RFC 6962 section 2.1
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

// the level-wise tree k_merkle_level_keep builds
std::vector<Words> build(const Words& leaves, uint64_t n) {
  std::vector<Words> lv;
  lv.emplace_back(leaves.begin(), leaves.begin() + 8 * n);
  for (uint64_t m = n; m > 1; m = (m + 1) / 2) {
    const Words& in = lv.back();
    Words nx(8 * ((m + 1) / 2));
    for (uint64_t i = 0; i < m / 2; ++i) pv::sha256_node(&nx[8 * i], &in[16 * i]);
    if (m & 1) memcpy(&nx[8 * (m / 2)], &in[8 * (m - 1)], 32);
    lv.push_back(std::move(nx));
  }
  return lv;
}

void check_edge(const std::vector<std::vector<Words>>& full, const std::vector<Words>& roots, const Words& leaves,
                uint64_t n_old, uint64_t n_new) {
  ++g_edges;
  const std::vector<Words>& want = full[n_new];
  const std::vector<Words>& old = full[n_old];
  // heap blocks of exactly the nodes of n_new leaves: one node too far is a sanitizer report
  std::vector<std::unique_ptr<uint32_t[]>> lv;
  std::vector<uint32_t*> table;
  for (uint32_t l = 0; l < want.size(); ++l) {
    const uint64_t cnt = pv::ml_level_count(n_new, l);
    lv.emplace_back(new uint32_t[8 * cnt]);
    memset(lv[l].get(), 0xa5, 32 * cnt);
    const uint64_t have = l < old.size() ? old[l].size() / 8 : 0;
    const uint64_t keep = have < cnt ? have : cnt;
    if (keep) memcpy(lv[l].get(), old[l].data(), 32 * keep);
    table.push_back(lv[l].get());
  }
  uint64_t f0 = n_new - 1;
  if (n_new > n_old) {
    memcpy(lv[0].get() + 8 * n_old, &leaves[8 * n_old], 32 * (n_new - n_old));
    f0 = n_old;
  }
  std::unique_ptr<uint32_t[]> b0(new uint32_t[8 * pv::ML_EDGE_BUF]), b1(new uint32_t[8 * pv::ML_EDGE_BUF]);
  const uint32_t depth = pv::ml_edge_rebuild(table.data(), f0, n_new, b0.get(), b1.get(), 0u, 1u, [] {});
  if (depth + 1 != want.size()) bad("depth", n_old, n_new, depth);
  for (uint32_t l = 0; l < want.size(); ++l)
    if (memcmp(lv[l].get(), want[l].data(), 4 * want[l].size())) bad("level", n_old, n_new, l);
  if (memcmp(lv[want.size() - 1].get(), roots[n_new].data(), 32)) bad("root", n_old, n_new, 0);
}

}  // namespace

int main() {
  const uint64_t N = 130;
  Words leaves(8 * N);
  for (uint64_t i = 0; i < N; ++i) {
    uint8_t text[64] = {0};
    const int len = snprintf(reinterpret_cast<char*>(text), 32, "txn-%llu", (unsigned long long)i);
    pv::sha256_msg(&leaves[8 * i], text, (uint64_t)len, 1, 0x00);
  }
  std::vector<Words> roots(N + 1, Words(8));
  std::vector<std::vector<Words>> full(N + 1);
  for (uint64_t s = 1; s <= N; ++s) {
    mth(roots[s].data(), leaves, 0, s);
    full[s] = build(leaves, s);
    if (memcmp(full[s].back().data(), roots[s].data(), 32)) bad("level-wise root", s, s, 0);
  }

  // ---- 1. every transition
  for (uint64_t n_old = 0; n_old <= N; ++n_old)
    for (uint64_t n_new = 1; n_new <= N; ++n_new) check_edge(full, roots, leaves, n_old, n_new);
  {   // n_new == 0: nothing to rebuild, nothing touched
    uint32_t* none[1] = {nullptr};
    for (uint64_t n_old = 0; n_old <= N; ++n_old)
      if (pv::ml_edge_rebuild(none, 0, 0, nullptr, nullptr, 0u, 1u, [] {}) != 0) bad("empty depth", n_old, 0, 0);
    g_edges += N + 1;
  }

  // ---- 2. append-by-append simulation: stack of (height, hash), one carry per trailing one bit
  Words sim_nodes;                       // writeNode order
  std::vector<uint64_t> sim_upto(N + 1); // nodes written once s leaves are in
  std::vector<Words> sim_frontier(N + 1);
  {
    std::vector<std::pair<uint32_t, Words>> stack;
    for (uint64_t e = 1; e <= N; ++e) {
      stack.emplace_back(0u, Words(leaves.begin() + 8 * (e - 1), leaves.begin() + 8 * e));
      while (stack.size() >= 2 && stack[stack.size() - 2].first == stack.back().first) {
        uint32_t lr[16], h[8];
        memcpy(lr, stack[stack.size() - 2].second.data(), 32);
        memcpy(lr + 8, stack.back().second.data(), 32);
        pv::sha256_node(h, lr);
        const uint32_t height = stack.back().first + 1;
        stack.pop_back();
        stack.back() = {height, Words(h, h + 8)};
        sim_nodes.insert(sim_nodes.end(), h, h + 8);
      }
      sim_upto[e] = sim_nodes.size() / 8;
      for (auto& s : stack) sim_frontier[e].insert(sim_frontier[e].end(), s.second.begin(), s.second.end());
    }
  }
  for (uint64_t n = 1; n <= N; ++n) {
    std::vector<const uint32_t*> table;
    for (auto& v : full[n]) table.push_back(v.data());
    for (uint64_t s = 1; s <= n; ++s) {   // frontier of every prefix
      const uint32_t cnt = pv::ml_popc64(s);
      std::unique_ptr<uint32_t[]> out(new uint32_t[8 * cnt]);
      for (uint32_t b = 0; b < 64; ++b)
        if ((s >> b) & 1) pv::ml_frontier_node(table.data(), s, b, out.get());
      if (sim_frontier[s].size() != 8 * cnt || memcmp(out.get(), sim_frontier[s].data(), 32 * cnt))
        bad("frontier", n, s, cnt);
    }
    for (uint64_t first = 0; first <= n; ++first)
      for (uint64_t last = first; last <= n; ++last) {
        ++g_ranges;
        const uint64_t need = pv::ml_nodes_upto(last) - pv::ml_nodes_upto(first);
        if (need != sim_upto[last] - sim_upto[first]) bad("node count", n, first, last);
        std::unique_ptr<uint32_t[]> lo(new uint32_t[8 * (last - first)]), no(new uint32_t[8 * need]);
        for (uint64_t e = first + 1; e <= last; ++e) pv::ml_hs_gather(table.data(), first, e, lo.get(), no.get());
        if (last > first && memcmp(lo.get(), &leaves[8 * first], 32 * (last - first))) bad("store leaves", n, first, last);
        if (need && memcmp(no.get(), &sim_nodes[8 * sim_upto[first]], 32 * need)) bad("store nodes", n, first, last);
        uint64_t nbad = 0, lowest = ~0ull;
        for (uint64_t e = first + 1; e <= last; ++e) {
          uint64_t lw = ~0ull;
          nbad += pv::ml_hs_check(table.data(), first, e, no.get(), &lw);
          if (lw < lowest) lowest = lw;
        }
        if (nbad || lowest != ~0ull) bad("clean check", n, first, last);
        if (need) {
          const uint64_t at = (first * 7 + last * 3 + n) % need;
          no[8 * at + (first + last) % 8] ^= 1u << (n % 32);
          nbad = 0, lowest = ~0ull;
          for (uint64_t e = first + 1; e <= last; ++e) {
            uint64_t lw = ~0ull;
            nbad += pv::ml_hs_check(table.data(), first, e, no.get(), &lw);
            if (lw < lowest) lowest = lw;
          }
          if (nbad != 1 || lowest != at) bad("flipped node", n, first, last);
        }
      }
  }
  printf("ledgercheck: %llu edge rebuilds, %llu store ranges, %d failures\n", (unsigned long long)g_edges,
         (unsigned long long)g_ranges, g_bad);
  return g_bad ? 1 : 0;
}
