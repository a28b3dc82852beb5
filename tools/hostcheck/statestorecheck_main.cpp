// Stand-alone run of the resident trie node store under AddressSanitizer +
// UBSan (tools/hostcheck/Makefile: statestorecheck_asan).  A program of its
// own, never loaded into Python; nothing here runs on a GPU.
//
//   statestorecheck_asan CASEFILE
//
// The case file is written by tests/test_state_store_host.py (layout below,
// little-endian).  Each case is a store filled by some add calls and one prove
// call with its expected outputs.  Insert runs on the store's own (padded)
// blob, as hashing needs; the walk and the pack then run with EVERY buffer --
// blob without its 16 spare bytes, ranges, digests, table, roots, keys and all
// outputs -- in a heap allocation of its exact size, so that one byte read or
// written past any of them stops the program.  Outputs are compared with the
// expected ones byte for byte.
//
//   "SSC1", u32 cases; per case:
//     u64 batches; per batch: u8 kind, u64 n_new, then
//       kind 0 (nodes): u64 off[n_new + 1] (off[0] = 0), the bytes
//       kind 1 (raw digests, nodes without bytes: the table's edges): n_new x 32 bytes
//     u64 n_roots, roots (32 each)
//     u64 n_queries, u8 has_idx, [u32 root_idx[n_queries]], u64 key_off[n_queries + 1], key bytes
//     u32 max_nodes
//     u64 n_nodes, u64 n_unique                      expected after the adds
//     u8 status[], u32 node_count[], u64 proof_off[n_queries + 1], u64 val_rel[], u64 val_len[], proof bytes
#include <stdio.h>
#include <stdlib.h>

#include "statestore_host.h"

namespace {

int g_fail = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                              \
    }                                                        \
  } while (0)

FILE* g_in;

// n elements of T read into a heap allocation of exactly n * sizeof(T) bytes
template <typename T>
T* take(uint64_t n) {
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (n && fread(p, sizeof(T), n, g_in) != n) {
    printf("FAIL: the case file ends early\n");
    exit(2);
  }
  return p;
}

template <typename T>
T one() {
  T* p = take<T>(1);
  const T v = *p;
  free(p);
  return v;
}

template <typename T>
T* exact(const std::vector<T>& v, uint64_t n) {
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (n) memcpy(p, v.data(), n * sizeof(T));
  return p;
}

void run_case(uint32_t c) {
  ssh::Store st;
  ssh::init(st, 1);
  const uint64_t batches = one<uint64_t>();
  for (uint64_t b = 0; b < batches; ++b) {
    const uint8_t kind = one<uint8_t>();
    const uint64_t n_new = one<uint64_t>();
    if (kind == 1) {
      uint8_t* digests = take<uint8_t>(32 * n_new);
      ssh::add_digests(st, digests, n_new);
      free(digests);
      continue;
    }
    uint64_t* off = take<uint64_t>(n_new + 1);
    uint8_t* bytes = take<uint8_t>(off[n_new]);
    ssh::add(st, bytes, off, n_new);
    free(bytes);
    free(off);
  }
  const uint64_t n_roots = one<uint64_t>();
  uint8_t* roots = take<uint8_t>(32 * n_roots);
  const uint64_t nq = one<uint64_t>();
  const uint8_t has_idx = one<uint8_t>();
  uint32_t* ridx = has_idx ? take<uint32_t>(nq) : nullptr;
  uint64_t* koff = take<uint64_t>(nq + 1);
  uint8_t* keys = take<uint8_t>(koff[nq]);
  const uint32_t max_nodes = one<uint32_t>();
  const uint64_t want_nodes = one<uint64_t>(), want_unique = one<uint64_t>();
  uint8_t* w_status = take<uint8_t>(nq);
  uint32_t* w_count = take<uint32_t>(nq);
  uint64_t* w_off = take<uint64_t>(nq + 1);
  uint64_t* w_rel = take<uint64_t>(nq);
  uint64_t* w_len = take<uint64_t>(nq);
  uint8_t* w_proof = take<uint8_t>(w_off[nq]);
  CHECK(st.nodes() == want_nodes);
  CHECK(st.n_unique == want_unique);
  CHECK(st.nodes() <= st.table.size() / 2);

  // exact-size copies of everything the walk and the pack read
  const uint64_t n = st.nodes();
  uint8_t* blob = exact(st.blob, st.n_bytes);
  uint64_t* beg = exact(st.beg, n);
  uint64_t* end = exact(st.end, n);
  uint32_t* dig = exact(st.dig, 8 * n);
  uint32_t* table = exact(st.table, st.table.size());
  const ssh::View v{blob, beg, end, dig, table, (uint32_t)st.table.size(), (uint32_t)n};
  uint8_t* status = static_cast<uint8_t*>(malloc(nq ? nq : 1));
  uint32_t* count = static_cast<uint32_t*>(malloc(nq ? 4 * nq : 1));
  uint32_t* ids = static_cast<uint32_t*>(malloc(nq ? 4 * nq * max_nodes : 1));
  uint64_t* poff = static_cast<uint64_t*>(malloc(8 * (nq + 1)));
  uint64_t* rel = static_cast<uint64_t*>(malloc(nq ? 8 * nq : 1));
  uint64_t* len = static_cast<uint64_t*>(malloc(nq ? 8 * nq : 1));
  // the sizing call, a capacity one byte short, then the exact capacity
  CHECK(ssh::prove(v, roots, ridx, n_roots, keys, koff, nq, max_nodes, status, count, ids, poff, rel, len, nullptr,
                   0) == 0);
  const uint64_t total = poff[nq];
  CHECK(total == w_off[nq]);
  uint8_t* proof = static_cast<uint8_t*>(malloc(total ? total : 1));
  if (total)
    CHECK(ssh::prove(v, roots, ridx, n_roots, keys, koff, nq, max_nodes, status, count, ids, poff, rel, len, proof,
                     total - 1) == -22);
  CHECK(ssh::prove(v, roots, ridx, n_roots, keys, koff, nq, max_nodes, status, count, ids, poff, rel, len, proof,
                   total) == 0);
  CHECK(memcmp(status, w_status, nq) == 0);
  CHECK(memcmp(count, w_count, 4 * nq) == 0);
  CHECK(memcmp(poff, w_off, 8 * (nq + 1)) == 0);
  CHECK(memcmp(rel, w_rel, 8 * nq) == 0);
  CHECK(memcmp(len, w_len, 8 * nq) == 0);
  if (total == w_off[nq]) CHECK(memcmp(proof, w_proof, total) == 0);
  if (g_fail) printf("case %u failed\n", c);
  void* all[] = {roots, ridx, koff, keys, w_status, w_count, w_off, w_rel, w_len, w_proof, blob, beg, end,
                 dig, table, status, count, ids, poff, rel, len, proof};
  for (void* p : all) free(p);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    printf("usage: statestorecheck_asan CASEFILE\n");
    return 2;
  }
  char magic[4];
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SSC1", 4) != 0) {
    printf("FAIL: not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t c = 0; c < cases; ++c) run_case(c);
  fclose(g_in);
  if (g_fail) {
    printf("statestorecheck: %d failures\n", g_fail);
    return 1;
  }
  printf("statestorecheck ok: %u cases\n", cases);
  return 0;
}
