// Stand-alone run of the reads from the resident trie node store under
// AddressSanitizer + UBSan (tools/hostcheck/Makefile: stategetcheck_asan).  A
// program of its own, never loaded into Python; nothing here runs on a GPU.
//
//   stategetcheck_asan CASEFILE
//
// The case file is written by tests/test_state_get_host.py (layout below,
// little-endian).  A case is a store filled by some add calls and one get call
// with its expected outputs; a value row is one stored value and what the decode
// answers on it.  The adds run on the store's own (padded) blob, as hashing
// needs; the read then runs with EVERY buffer -- blob without its 16 spare
// bytes, ranges, digests, table, roots, keys, each value row and all outputs --
// in a heap allocation of its exact size, so that one byte read or written past
// any of them stops the program.  Outputs are compared with the expected ones
// byte for byte.
//
//   "SGC1", u32 cases; per case:
//     u64 batches; per batch: u64 n_new, u64 off[n_new + 1] (off[0] = 0), the bytes
//     u64 n_roots, roots (32 each)
//     u64 n_queries, u8 has_idx, [u32 root_idx[n_queries]], u64 key_off[n_queries + 1], key bytes
//     i32 decode
//     u8 status[], u8 found[], u64 val_off[n_queries + 1], value bytes           expected
//   u32 values; per value: u64 len, the bytes, u8 ok, u64 payload begin, u64 payload end
#include <stdio.h>
#include <stdlib.h>

#include "stateget_host.h"

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
  ssh::Store st;
  ssh::init(st, 1);
  const uint64_t batches = one<uint64_t>();
  for (uint64_t b = 0; b < batches; ++b) {
    const uint64_t n_new = one<uint64_t>();
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
  const int32_t decode = one<int32_t>();
  uint8_t* w_status = take<uint8_t>(nq);
  uint8_t* w_found = take<uint8_t>(nq);
  uint64_t* w_off = take<uint64_t>(nq + 1);
  uint8_t* w_vals = take<uint8_t>(w_off[nq]);

  const uint64_t n = st.nodes();
  uint8_t* blob = exact(st.blob, st.n_bytes);
  uint64_t* beg = exact(st.beg, n);
  uint64_t* end = exact(st.end, n);
  uint32_t* dig = exact(st.dig, 8 * n);
  uint32_t* table = exact(st.table, st.table.size());
  const ssh::View v{blob, beg, end, dig, table, (uint32_t)st.table.size(), (uint32_t)n};
  uint8_t* status = room<uint8_t>(nq);
  uint8_t* found = room<uint8_t>(nq);
  uint64_t* src = room<uint64_t>(nq);
  uint64_t* voff = room<uint64_t>(nq + 1);
  // the sizing call, a capacity one byte short, then the exact capacity
  CHECK(sgh::get(v, roots, ridx, n_roots, keys, koff, nq, decode, status, found, src, voff, nullptr, 0) == 0);
  const uint64_t total = voff[nq];
  CHECK(total == w_off[nq]);
  uint8_t* vals = room<uint8_t>(total);
  if (total)
    CHECK(sgh::get(v, roots, ridx, n_roots, keys, koff, nq, decode, status, found, src, voff, vals, total - 1) == -22);
  CHECK(sgh::get(v, roots, ridx, n_roots, keys, koff, nq, decode, status, found, src, voff, vals, total) == 0);
  CHECK(memcmp(status, w_status, nq) == 0);
  CHECK(memcmp(found, w_found, nq) == 0);
  CHECK(memcmp(voff, w_off, 8 * (nq + 1)) == 0);
  if (total == w_off[nq]) CHECK(memcmp(vals, w_vals, total) == 0);
  if (g_fail) printf("case %u failed\n", c);
  void* all[] = {roots, ridx, koff, keys, w_status, w_found, w_off, w_vals, blob, beg,
                 end,   dig,  table, status, found, src, voff, vals};
  for (void* p : all) free(p);
}

void run_value(uint32_t i) {
  const uint64_t len = one<uint64_t>();
  uint8_t* value = take<uint8_t>(len);
  const uint8_t ok = one<uint8_t>();
  const uint64_t wb = one<uint64_t>(), we = one<uint64_t>();
  uint64_t pb = 0, pe = 0;
  const bool got = pv::tg_decode(value, 0, len, pb, pe);
  CHECK(got == (ok != 0));
  if (got && ok) CHECK(pb == wb && pe == we && pe <= len);
  if (g_fail) printf("value %u failed\n", i);
  free(value);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
    printf("usage: stategetcheck_asan CASEFILE\n");
    return 2;
  }
  char magic[4];
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SGC1", 4) != 0) {
    printf("FAIL: not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t c = 0; c < cases; ++c) run_case(c);
  const uint32_t values = one<uint32_t>();
  for (uint32_t i = 0; i < values; ++i) run_value(i);
  fclose(g_in);
  if (g_fail) {
    printf("stategetcheck: %d failures\n", g_fail);
    return 1;
  }
  printf("stategetcheck ok: %u cases, %u values\n", cases, values);
  return 0;
}
