// Stand-alone run of the sort of state keys under AddressSanitizer + UBSan
// (tools/hostcheck/Makefile: statesortcheck_asan).  A program of its own, never
// loaded into Python; nothing here runs on a GPU.
//
//   statesortcheck_asan CASEFILE
//
// The case file is written by tests/test_state_sort_host.py (layout below,
// little-endian).  The key bytes and the offsets lie in heap allocations of
// their exact size and every work array of the sort has its exact size
// (statesort_host.h), so one byte read past a key at the end of the blob, or
// one record written past an array, stops the program.  Each case runs twice:
// with std::stable_sort per round and with the device's counting passes.
//
//   "SSC1", u32 cases; per case:
//     u64 n, u64 key_off[n + 1], u64 blob_len, the blob's bytes
//     u32 expected code (0; 1 / 2: refused for offsets / a key above 1024 bytes)
//     u64 expected bad index (refusals)
//     accepted cases: u64 m, u32 perm[m], u32 rounds (0: not checked)
#include <stdio.h>
#include <stdlib.h>

#include "statesort_host.h"

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

void run_case(uint32_t number) {
  const uint64_t n = one<uint64_t>();
  uint64_t* koff = take<uint64_t>(n + 1);
  const uint64_t blob_len = one<uint64_t>();
  uint8_t* keys = take<uint8_t>(blob_len);
  const uint32_t want_rc = one<uint32_t>();
  const uint64_t want_bad = one<uint64_t>();
  uint64_t m = 0;
  uint32_t* perm = nullptr;
  uint32_t want_rounds = 0;
  if (!want_rc) {
    m = one<uint64_t>();
    perm = take<uint32_t>(m);
    want_rounds = one<uint32_t>();
  }
  for (int lsd = 0; lsd < 2; ++lsd) {
    ssoh::Sorted s;
    const int rc = ssoh::sort(keys, koff, n, lsd != 0, s);
    CHECK((uint32_t)rc == want_rc);
    if (want_rc) {
      CHECK(s.bad_index == want_bad);
      CHECK(s.perm.empty() && s.m == 0);
    } else if (rc == ssoh::OK) {
      CHECK(s.m == m && s.perm.size() == m);
      CHECK(m == 0 || (s.m == m && memcmp(s.perm.data(), perm, 4 * m) == 0));
      CHECK(want_rounds == 0 || s.rounds == want_rounds);
    }
  }
  free(perm);
  free(koff);
  free(keys);
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
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SSC1", 4) != 0) {
    printf("not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t k = 0; k < cases && !g_fail; ++k) run_case(k);
  fclose(g_in);
  if (g_fail) return 1;
  printf("statesortcheck: %u cases ok\n", cases);
  return 0;
}
