// Stand-alone self-check of pv_sha3.h and pv_trie_proof.h under
// AddressSanitizer + UBSan (tools/hostcheck/Makefile: stateproofcheck_asan).
// It is a program of its own, never loaded into Python.
//
//   SHA3: known answers; every length 0..600 at byte offsets 0..7 of a heap
//   buffer that ends exactly 16 bytes after the message (the over-read
//   convention of the header) must equal the digest of an aligned copy.
//   Walk: a hand-built proof gives the expected statuses; then truncated,
//   bit-flipped and random node bytes -- with the root set to the node's own
//   digest, so the walk does enter it -- run on a heap copy that ends exactly
//   at the node's last byte.  Every status must be one of SP_*, and the
//   sanitizers must stay silent.
//   With a case file as its argument: each case's walk, over the same exact-size
//   copies, must give the recorded status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_sha3.h"
#include "../../indy-plenum_amd/csrc/pv_trie_proof.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}

// digest of m[0 .. len) placed at byte offset `off` of a heap buffer with 16 bytes after it
void sha3_at(uint8_t out[32], const uint8_t* m, size_t len, size_t off) {
  uint8_t* buf = static_cast<uint8_t*>(malloc(off + len + 16));
  memset(buf, 0xa5, off + len + 16);
  if (len) memcpy(buf + off, m, len);
  uint32_t d[8];
  pv::sha3_256_msg(d, buf + off, len);
  memcpy(out, d, 32);
  free(buf);
}

void from_hex(uint8_t* out, const char* hex, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    sscanf(hex + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}

// one-proof, one-query walk over exact-size heap copies of every buffer
uint32_t walk(const std::vector<std::vector<uint8_t>>& nodes, const uint8_t root[32], const std::vector<uint8_t>& key,
              const std::vector<uint8_t>& val) {
  std::vector<uint32_t> dig(8 * nodes.size() + 8);
  std::vector<uint64_t> beg, end;
  size_t total = 0;
  for (size_t j = 0; j < nodes.size(); ++j) {
    uint8_t d[32];
    sha3_at(d, nodes[j].data(), nodes[j].size(), 0);
    memcpy(&dig[8 * j], d, 32);
    beg.push_back(total);
    total += nodes[j].size();
    end.push_back(total);
  }
  uint8_t* blob = static_cast<uint8_t*>(malloc(total ? total : 1));
  for (size_t j = 0; j < nodes.size(); ++j)
    if (!nodes[j].empty()) memcpy(blob + beg[j], nodes[j].data(), nodes[j].size());
  uint8_t* k = static_cast<uint8_t*>(malloc(key.size() ? key.size() : 1));
  uint8_t* v = static_cast<uint8_t*>(malloc(val.size() ? val.size() : 1));
  if (!key.empty()) memcpy(k, key.data(), key.size());
  if (!val.empty()) memcpy(v, val.data(), val.size());
  uint32_t r[8];
  memcpy(r, root, 32);
  const uint32_t st = pv::sp_verify(blob, beg.data(), end.data(), dig.data(), 0, nodes.size(), r, k, key.size(), v,
                                    val.size());
  free(blob);
  free(k);
  free(v);
  return st;
}

void root_of(uint8_t root[32], const std::vector<uint8_t>& node) { sha3_at(root, node.data(), node.size(), 0); }

}  // namespace

int main(int argc, char** argv) {
  // ---- SHA3-256
  uint8_t want[32], got[32];
  from_hex(want, "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a", 32);
  sha3_at(got, nullptr, 0, 0);
  CHECK(memcmp(got, want, 32) == 0);
  from_hex(want, "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532", 32);
  sha3_at(got, reinterpret_cast<const uint8_t*>("abc"), 3, 0);
  CHECK(memcmp(got, want, 32) == 0);
  const uint8_t blank = 0x80;
  sha3_at(got, &blank, 1, 0);
  uint32_t bw[8];
  memcpy(bw, got, 32);
  CHECK(pv::sp_is_blank_root(bw));
  std::vector<uint8_t> msg(600);
  for (auto& b : msg) b = (uint8_t)rnd();
  for (size_t len = 0; len <= msg.size(); ++len) {
    sha3_at(want, msg.data(), len, 0);
    for (size_t off = 1; off < 8; ++off) {
      sha3_at(got, msg.data(), len, off);
      CHECK(memcmp(got, want, 32) == 0);
    }
  }

  // ---- the walk on a hand-built trie: root = branch-free leaf for key "k1" -> "v"
  const std::vector<uint8_t> leaf = {0xc5, 0x83, 0x20, 0x6b, 0x31, 0x76};
  const std::vector<uint8_t> k1 = {0x6b, 0x31}, k2 = {0x6b, 0x32}, v = {0x76}, w = {0x77}, none;
  uint8_t root[32];
  root_of(root, leaf);
  CHECK(walk({leaf}, root, k1, v) == pv::SP_OK);
  CHECK(walk({leaf}, root, k1, w) == pv::SP_VALUE_MISMATCH);
  CHECK(walk({leaf}, root, k1, none) == pv::SP_VALUE_MISMATCH);
  CHECK(walk({leaf}, root, k2, none) == pv::SP_OK);
  CHECK(walk({leaf}, root, k2, v) == pv::SP_VALUE_MISMATCH);
  CHECK(walk({}, root, k1, v) == pv::SP_NODE_MISSING);
  sha3_at(got, &blank, 1, 0);
  CHECK(walk({}, got, k1, none) == pv::SP_OK);
  CHECK(walk({}, got, k1, v) == pv::SP_VALUE_MISMATCH);
  // an extension (path 6) over the leaf (path b 3 1, odd): rlp([0x16, hash(leaf2)])
  const std::vector<uint8_t> leaf2 = {0xc5, 0x83, 0x3b, 0x31, 0x00, 0x76};   // path b,3,1,0,0 != key: absent
  std::vector<uint8_t> ext = {0xe2, 0x16, 0xa0};
  uint8_t h2[32];
  root_of(h2, leaf2);
  ext.insert(ext.end(), h2, h2 + 32);
  root_of(root, ext);
  CHECK(walk({leaf2, ext}, root, k1, none) == pv::SP_OK);            // leaf path mismatch: blank
  CHECK(walk({ext}, root, k1, none) == pv::SP_NODE_MISSING);
  // an extension with an empty path never ends a walk: malformed by rule
  std::vector<uint8_t> ext0 = {0xe2, 0x00, 0xa0};
  ext0.insert(ext0.end(), h2, h2 + 32);
  root_of(root, ext0);
  CHECK(walk({leaf2, ext0}, root, k1, none) == pv::SP_MALFORMED);

  // ---- truncated, flipped and random nodes
  std::vector<std::vector<uint8_t>> seeds = {leaf, ext, leaf2};
  std::vector<uint8_t> branch = {0xd1};   // 17 empty items
  branch.insert(branch.end(), 17, 0x80);
  seeds.push_back(branch);
  std::vector<uint8_t> longnode = {0xf8, 0x46, 0x83, 0x20, 0x6b, 0x31, 0xb8, 0x40};
  longnode.insert(longnode.end(), 64, 0x55);
  seeds.push_back(longnode);
  for (const auto& s : seeds) {
    for (size_t cut = 0; cut <= s.size(); ++cut) {
      std::vector<uint8_t> t(s.begin(), s.begin() + cut);
      root_of(root, t);
      CHECK(walk({t}, root, k1, v) <= pv::SP_MALFORMED);
      CHECK(walk({t, leaf2}, root, k2, none) <= pv::SP_MALFORMED);
    }
    for (size_t bit = 0; bit < 8 * s.size(); ++bit) {
      std::vector<uint8_t> t = s;
      t[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      root_of(root, t);
      CHECK(walk({t, leaf2}, root, k1, v) <= pv::SP_MALFORMED);
    }
  }
  for (int it = 0; it < 20000; ++it) {
    std::vector<uint8_t> t(rnd() % 80);
    for (auto& b : t) b = (uint8_t)rnd();
    // bias the first bytes towards list headers so that the item scan runs
    if (!t.empty() && (it & 1)) t[0] = (uint8_t)(0xc0 + rnd() % 64);
    std::vector<uint8_t> key(rnd() % 5);
    for (auto& b : key) b = (uint8_t)rnd();
    root_of(root, t);
    CHECK(walk({t, leaf2}, root, key, (it & 2) ? v : none) <= pv::SP_MALFORMED);
    // the same bytes as a serialized proof
    std::vector<uint64_t> ib(8), ie(8);
    uint64_t count = 0;
    uint8_t* exact = static_cast<uint8_t*>(malloc(t.size() ? t.size() : 1));
    if (!t.empty()) memcpy(exact, t.data(), t.size());
    const bool ok = pv::rlp_split_list(exact, t.size(), ib.data(), ie.data(), 8, &count);
    CHECK(count <= 8);
    if (ok)
      for (uint64_t k = 0; k < count; ++k) CHECK(ib[k] < ie[k] && ie[k] <= t.size());
    free(exact);
  }
  // ---- a case file (tests/test_state_proofs_host.py): "SVC1", count, then per case the node count,
  // each node as (length, bytes), the root, the key and the expected value as (length, bytes) and the
  // status the host build gave
  if (argc > 1) {
    FILE* fh = fopen(argv[1], "rb");
    char magic[4] = {0};
    uint32_t n_cases = 0;
    CHECK(fh && fread(magic, 1, 4, fh) == 4 && memcmp(magic, "SVC1", 4) == 0 && fread(&n_cases, 4, 1, fh) == 1);
    auto bytes = [&](std::vector<uint8_t>& out) {
      uint64_t len = 0;
      bool ok = fread(&len, 8, 1, fh) == 1 && len < (1u << 20);
      out.assign(ok ? len : 0, 0);
      return ok && (len == 0 || fread(out.data(), 1, len, fh) == len);
    };
    uint32_t done = 0;
    for (; fh && !g_fail && done < n_cases; ++done) {
      uint64_t n_nodes = 0;
      CHECK(fread(&n_nodes, 8, 1, fh) == 1 && n_nodes < 1024);
      std::vector<std::vector<uint8_t>> nodes(g_fail ? 0 : n_nodes);
      for (auto& node : nodes) CHECK(bytes(node));
      std::vector<uint8_t> key, val;
      uint32_t status = 0;
      CHECK(fread(root, 1, 32, fh) == 32 && bytes(key) && bytes(val) && fread(&status, 4, 1, fh) == 1);
      if (!g_fail) CHECK(walk(nodes, root, key, val) == status);
    }
    if (fh) fclose(fh);
    if (!g_fail) printf("stateproofcheck: %u cases ok\n", done);
  }
  if (g_fail) {
    printf("stateproofcheck: %d failures\n", g_fail);
    return 1;
  }
  printf("stateproofcheck ok\n");
  return 0;
}
