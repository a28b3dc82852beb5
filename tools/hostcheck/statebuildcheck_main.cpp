// Stand-alone run of the batch trie build under AddressSanitizer + UBSan
// (tools/hostcheck/Makefile: statebuildcheck_asan).  A program of its own, never
// loaded into Python; nothing here runs on a GPU.
//
//   statebuildcheck_asan CASEFILE
//
// The case file is written by tests/test_state_build_host.py (layout below,
// little-endian).  Each case is one build over keys and values that lie in heap
// allocations of their exact size; every work array of the build has its exact
// size too (statebuild_host.h), and the outputs are delivered into exact-size
// allocations, so one byte read or written past any of them stops the program.
// Only the node blob keeps the 16 spare bytes the hash reads past the last node.
// Each accepted case is then delivered once more with each capacity one short:
// that must report the sizes and write nothing.
//
//   "SBC1", u32 cases; per case:
//     u64 n, u64 key_off[n + 1], key bytes, u64 val_off[n + 1], value bytes
//     u32 expected code (0, or 1 / 2 / 3: refused for order / an empty value / offsets)
//     u64 expected bad index (refusals)
//     accepted cases: 32 bytes root, u64 n_nodes, u64 n_bytes, u64 node_off[n_nodes + 1], the node bytes,
//                     32 n_nodes bytes of digests
#include <stdio.h>
#include <stdlib.h>

#include "statebuild_host.h"

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
T* blank(uint64_t n, int fill) {
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  memset(p, fill, n ? n * sizeof(T) : 1);
  return p;
}

void run_case(uint32_t number) {
  const uint64_t n = one<uint64_t>();
  uint64_t* koff = take<uint64_t>(n + 1);
  uint8_t* keys = take<uint8_t>(koff[n]);
  uint64_t* voff = take<uint64_t>(n + 1);
  uint8_t* vals = take<uint8_t>(voff[n]);
  const uint32_t want_rc = one<uint32_t>();
  const uint64_t want_bad = one<uint64_t>();
  sbh::Built b;
  const int rc = sbh::build(keys, koff, vals, voff, n, b);
  CHECK((uint32_t)rc == want_rc);
  if (want_rc) {
    CHECK(b.bad_index == want_bad);
    CHECK(b.n_nodes == 0 && b.n_bytes == 0);
  } else {
    uint8_t* root = take<uint8_t>(32);
    const uint64_t n_nodes = one<uint64_t>(), n_bytes = one<uint64_t>();
    uint64_t* off = take<uint64_t>(n_nodes + 1);
    uint8_t* bytes = take<uint8_t>(n_bytes);
    uint8_t* dig = take<uint8_t>(32 * n_nodes);
    uint8_t* g_root = blank<uint8_t>(32, 0);
    uint64_t g_nodes = 0, g_bytes = 0;
    uint8_t* g_blob = blank<uint8_t>(n_bytes, 0);
    uint64_t* g_off = blank<uint64_t>(n_nodes + 1, 0);
    uint8_t* g_dig = blank<uint8_t>(32 * n_nodes, 0);
    CHECK(sbh::deliver(b, g_root, &g_nodes, &g_bytes, g_blob, n_bytes, g_off, n_nodes, g_dig) == sbh::OK);
    CHECK(g_nodes == n_nodes && g_bytes == n_bytes);
    CHECK(memcmp(g_root, root, 32) == 0);
    if (g_nodes == n_nodes && g_bytes == n_bytes) {
      CHECK(memcmp(g_off, off, 8 * (n_nodes + 1)) == 0);
      CHECK(n_bytes == 0 || memcmp(g_blob, bytes, n_bytes) == 0);
      CHECK(n_nodes == 0 || memcmp(g_dig, dig, 32 * n_nodes) == 0);
    }
    // a second build gives the same bytes
    sbh::Built b2;
    CHECK(sbh::build(keys, koff, vals, voff, n, b2) == sbh::OK);
    CHECK(b2.blob == b.blob && b2.off == b.off && b2.dig == b.dig);
    // one byte or one node short: sizes, and not a byte written
    if (n_nodes) {
      for (int which = 0; which < 2; ++which) {
        uint8_t* s_blob = blank<uint8_t>(n_bytes - (which == 0), 0x5a);
        uint64_t* s_off = blank<uint64_t>(n_nodes + (which == 0), 0x5a);
        uint8_t* s_dig = blank<uint8_t>(32 * (n_nodes - (which == 1)), 0x5a);
        uint64_t s_nodes = 0, s_bytes = 0;
        CHECK(sbh::deliver(b, g_root, &s_nodes, &s_bytes, s_blob, n_bytes - (which == 0), s_off,
                           n_nodes - (which == 1), s_dig) == sbh::TOO_SMALL);
        CHECK(s_nodes == n_nodes && s_bytes == n_bytes);
        for (uint64_t k = 0; k + (which == 0) < n_bytes; ++k) CHECK(s_blob[k] == 0x5a);
        for (uint64_t k = 0; k < 32 * (n_nodes - (which == 1)); ++k) CHECK(s_dig[k] == 0x5a);
        free(s_blob);
        free(s_off);
        free(s_dig);
      }
    }
    free(root);
    free(off);
    free(bytes);
    free(dig);
    free(g_root);
    free(g_blob);
    free(g_off);
    free(g_dig);
  }
  free(koff);
  free(keys);
  free(voff);
  free(vals);
  if (g_fail) printf("  ... in case %u\n", number);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    printf("usage: %s CASEFILE\n", argv[0]);
    return 2;
  }
  g_in = fopen(argv[1], "rb");
  if (!g_in) {
    printf("cannot open %s\n", argv[1]);
    return 2;
  }
  char magic[4];
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SBC1", 4) != 0) {
    printf("not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t k = 0; k < cases && !g_fail; ++k) run_case(k);
  fclose(g_in);
  if (g_fail) return 1;
  printf("statebuildcheck: %u cases ok\n", cases);
  return 0;
}
