// Stand-alone run of the store prune under AddressSanitizer + UBSan
// (tools/hostcheck/Makefile: stateprunecheck_asan).  A program of its own, never
// loaded into Python; nothing here runs on a GPU.
//
//   stateprunecheck_asan CASEFILE
//
// The case file is written by tests/test_state_prune_host.py (layout below,
// little-endian).  Each case is a store filled by one add call and one set of
// kept roots with the expected outcome.  The add runs on the store's own
// (padded) blob, as hashing needs; the mark and the compaction then run with
// EVERY buffer -- blob without its 16 spare bytes, ranges, digests, table,
// roots, statuses, bitmap, queue and all outputs -- in a heap allocation of its
// exact size, so that one byte read or written past any of them stops the
// program.  Outputs are compared with the expected ones byte for byte; then the
// store itself is pruned, and pruned again, which must change nothing.
//
//   "SPC1", u32 cases; per case:
//     u64 n_nodes, u64 off[n_nodes + 1] (off[0] = 0), the bytes
//     u64 n_roots, roots (32 each)
//     u32 rc (PR_OK or PR_NESTING), u8 status[n_roots]
//     with PR_OK: u64 n_kept, u64 bytes_kept, u64 n_missing, n_kept x 32 digest bytes,
//                 u64 new_off[n_kept + 1], the kept bytes, u64 n_slots
#include <stdio.h>
#include <stdlib.h>

#include "stateprune_host.h"

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

template <typename T>
T* room(uint64_t n) {
  return static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
}

void run_case(uint32_t c) {
  const int before = g_fail;
  ssh::Store st;
  ssh::init(st, 1);
  const uint64_t n_nodes = one<uint64_t>();
  uint64_t* off = take<uint64_t>(n_nodes + 1);
  uint8_t* bytes = take<uint8_t>(off[n_nodes]);
  ssh::add(st, bytes, off, n_nodes);
  free(bytes);
  free(off);
  const uint64_t n_roots = one<uint64_t>();
  uint8_t* roots = take<uint8_t>(32 * n_roots);
  const uint32_t w_rc = one<uint32_t>();
  uint8_t* w_status = take<uint8_t>(n_roots);
  uint64_t w_kept = 0, w_bytes = 0, w_missing = 0, w_slots = 0;
  uint8_t *w_dig = nullptr, *w_blob = nullptr;
  uint64_t* w_off = nullptr;
  if (w_rc == sph::PR_OK) {
    w_kept = one<uint64_t>();
    w_bytes = one<uint64_t>();
    w_missing = one<uint64_t>();
    w_dig = take<uint8_t>(32 * w_kept);
    w_off = take<uint64_t>(w_kept + 1);
    w_blob = take<uint8_t>(w_bytes);
    w_slots = one<uint64_t>();
  }

  // exact-size copies of everything the mark and the compaction read and write
  const uint64_t n = st.nodes();
  uint8_t* blob = exact(st.blob, st.n_bytes);
  uint64_t* beg = exact(st.beg, n);
  uint64_t* end = exact(st.end, n);
  uint32_t* dig = exact(st.dig, 8 * n);
  uint32_t* table = exact(st.table, st.table.size());
  const ssh::View v{blob, beg, end, dig, table, (uint32_t)st.table.size(), (uint32_t)n};
  uint8_t* status = room<uint8_t>(n_roots);
  uint32_t* bits = room<uint32_t>((n + 31) / 32);
  uint32_t* queue = room<uint32_t>(st.n_unique);
  unsigned long long* counts = room<unsigned long long>(pv::TP_COUNTS);
  sph::mark(v, roots, n_roots, status, bits, queue, counts);
  CHECK(memcmp(status, w_status, n_roots) == 0);
  CHECK((counts[pv::TP_OVERFLOW] != 0) == (w_rc == sph::PR_NESTING));
  if (w_rc == sph::PR_OK && counts[pv::TP_OVERFLOW] == 0) {
    const uint64_t kept = counts[pv::TP_TAIL], kb = sph::kept_bytes(v, bits);
    CHECK(kept == w_kept);
    CHECK(kb == w_bytes);
    CHECK(counts[pv::TP_MISSING] == w_missing);
    CHECK(kept <= st.n_unique);
    if (kept == w_kept && kb == w_bytes) {
      uint8_t* nblob = room<uint8_t>(kb);
      uint64_t* nbeg = room<uint64_t>(kept);
      uint64_t* nend = room<uint64_t>(kept);
      uint32_t* ndig = room<uint32_t>(8 * kept);
      sph::compact(v, bits, nblob, nbeg, nend, ndig);
      CHECK(memcmp(ndig, w_dig, 32 * kept) == 0);
      CHECK(memcmp(nbeg, w_off, 8 * kept) == 0);
      CHECK(memcmp(nend, w_off + 1, 8 * kept) == 0);
      CHECK(memcmp(nblob, w_blob, kb) == 0);
      uint32_t* only = room<uint32_t>(8 * kept);   // the reporting call's form: the digests alone
      sph::compact(v, bits, nullptr, nullptr, nullptr, only);
      CHECK(memcmp(only, w_dig, 32 * kept) == 0);
      void* outs[] = {nblob, nbeg, nend, ndig, only};
      for (void* p : outs) free(p);
    }
    // the store itself: pruned, then pruned again
    bool all_ok = true;
    for (uint64_t i = 0; i < n_roots; ++i) all_ok = all_ok && w_status[i] == pv::SP_OK;
    uint64_t k2 = 0, b2 = 0, m2 = 0, bad = ~0ull;
    const int rc = sph::prune(st, roots, n_roots, 1, nullptr, &k2, &b2, &m2, nullptr, 0, &bad);
    CHECK(rc == (all_ok ? sph::PR_OK : sph::PR_ROOT_MISSING));
    if (all_ok) {
      CHECK(st.nodes() == w_kept && st.n_unique == w_kept && st.n_bytes == w_bytes);
      CHECK(st.table.size() == w_slots);
      CHECK(st.blob.size() == w_bytes + 16);
      CHECK(memcmp(st.blob.data(), w_blob, w_bytes) == 0);
      const std::vector<uint8_t> was = st.blob;
      CHECK(sph::prune(st, roots, n_roots, 1, nullptr, &k2, &b2, &m2, nullptr, 0, &bad) == sph::PR_OK);
      CHECK(k2 == w_kept && b2 == w_bytes && m2 == w_missing && st.blob == was && st.table.size() == w_slots);
    } else {
      CHECK(bad < n_roots && w_status[bad] != pv::SP_OK && st.nodes() == n);
    }
  }
  if (g_fail != before) printf("case %u failed\n", c);
  void* all[] = {roots, w_status, w_dig, w_off, w_blob, blob, beg, end, dig, table, status, bits, queue, counts};
  for (void* p : all) free(p);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    printf("usage: stateprunecheck_asan CASEFILE\n");
    return 2;
  }
  char magic[4];
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SPC1", 4) != 0) {
    printf("FAIL: not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t c = 0; c < cases; ++c) run_case(c);
  fclose(g_in);
  if (g_fail) {
    printf("stateprunecheck: %d failures\n", g_fail);
    return 1;
  }
  printf("stateprunecheck ok: %u cases\n", cases);
  return 0;
}
