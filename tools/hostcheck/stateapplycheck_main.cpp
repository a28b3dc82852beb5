// Stand-alone run of the sets and removals onto a committed root under AddressSanitizer +
// UBSan (tools/hostcheck/Makefile: stateapplycheck_asan).  A program of its own,
// never loaded into Python; nothing here runs on a GPU.
//
//   stateapplycheck_asan CASEFILE
//
// The case file is written by tests/test_state_apply_host.py (layout below,
// little-endian).  Each case is one batch (an empty value removes its key): the store's nodes, the batch's keys
// and values lie in heap allocations of their exact size, the store's arrays are
// copied into exact-size allocations before the walk reads them, and every work
// array of the merge and of the build has its exact size (stateupdate_host.h),
// the merged paths and payloads included, so one byte read or written past any
// of them stops the program.  Only the store's blob and the build's node blob
// keep the 16 spare bytes the hash reads past the last node.
//
//   "SAC1", u32 cases; per case:
//     u64 n_store, u64 store_off[n_store + 1], the store's node bytes
//     32 bytes old root
//     u64 n, u64 key_off[n + 1], key bytes, u64 val_off[n + 1], value bytes
//     u32 expected code (0; 1 / 2 / 3: refused for order / a value / offsets; 5: a walk refused)
//     u64 expected bad index, u32 expected PV_SP_* status (refusals)
//     accepted cases: 32 bytes root, u64 n_nodes, u64 n_bytes, u64 node_off[n_nodes + 1], the node bytes,
//                     32 n_nodes bytes of digests
#include <stdio.h>
#include <stdlib.h>

#include "stateupdate_host.h"

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

template <typename T>
T* exact(const std::vector<T>& v, uint64_t n) {
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (n) memcpy(p, v.data(), n * sizeof(T));
  return p;
}

void run_case(uint32_t number) {
  const uint64_t n_store = one<uint64_t>();
  uint64_t* soff = take<uint64_t>(n_store + 1);
  uint8_t* sbytes = take<uint8_t>(soff[n_store]);
  ssh::Store st;
  ssh::init(st, n_store);
  (void)ssh::add(st, sbytes, soff, n_store);
  uint8_t* old_root = take<uint8_t>(32);
  const uint64_t n = one<uint64_t>();
  uint64_t* koff = take<uint64_t>(n + 1);
  uint8_t* keys = take<uint8_t>(koff[n]);
  uint64_t* voff = take<uint64_t>(n + 1);
  uint8_t* vals = take<uint8_t>(voff[n]);
  const uint32_t want_rc = one<uint32_t>();
  const uint64_t want_bad = one<uint64_t>();
  const uint32_t want_status = one<uint32_t>();
  // the store as the walk reads it: exact-size arrays (the blob with its 16 spare bytes)
  const uint64_t nodes = st.nodes();
  ssh::View v = ssh::view(st);
  uint8_t* x_blob = exact(st.blob, st.n_bytes + 16);
  uint64_t *x_beg = exact(st.beg, nodes), *x_end = exact(st.end, nodes);
  uint32_t *x_dig = exact(st.dig, 8 * nodes), *x_table = exact(st.table, st.table.size());
  v.blob = x_blob;
  v.beg = x_beg;
  v.end = x_end;
  v.dig = x_dig;
  v.table = x_table;
  sbh::Built b;
  suh::Merged m;
  const int rc = suh::update(v, old_root, keys, koff, vals, voff, n, b, m, true);
  CHECK((uint32_t)rc == want_rc);
  if (want_rc) {
    CHECK(m.bad_index == want_bad);
    CHECK(m.status == want_status);
    CHECK(b.n_nodes == 0 && b.n_bytes == 0);
  } else {
    uint8_t* root = take<uint8_t>(32);
    const uint64_t n_nodes = one<uint64_t>(), n_bytes = one<uint64_t>();
    uint64_t* off = take<uint64_t>(n_nodes + 1);
    uint8_t* bytes = take<uint8_t>(n_bytes);
    uint8_t* dig = take<uint8_t>(32 * n_nodes);
    uint8_t* g_root = static_cast<uint8_t*>(calloc(32, 1));
    uint64_t g_nodes = 0, g_bytes = 0;
    uint8_t* g_blob = static_cast<uint8_t*>(calloc(n_bytes ? n_bytes : 1, 1));
    uint64_t* g_off = static_cast<uint64_t*>(calloc(n_nodes + 1, 8));
    uint8_t* g_dig = static_cast<uint8_t*>(calloc(n_nodes ? 32 * n_nodes : 1, 1));
    CHECK(sbh::deliver(b, g_root, &g_nodes, &g_bytes, g_blob, n_bytes, g_off, n_nodes, g_dig) == sbh::OK);
    CHECK(g_nodes == n_nodes && g_bytes == n_bytes);
    CHECK(memcmp(g_root, root, 32) == 0);
    if (g_nodes == n_nodes && g_bytes == n_bytes) {
      CHECK(memcmp(g_off, off, 8 * (n_nodes + 1)) == 0);
      CHECK(n_bytes == 0 || memcmp(g_blob, bytes, n_bytes) == 0);
      CHECK(n_nodes == 0 || memcmp(g_dig, dig, 32 * n_nodes) == 0);
    }
    // a second update gives the same bytes; one node short: sizes, and not a byte written
    sbh::Built b2;
    suh::Merged m2;
    CHECK(suh::update(v, old_root, keys, koff, vals, voff, n, b2, m2, true) == suh::OK);
    CHECK(b2.blob == b.blob && b2.off == b.off && b2.dig == b.dig && m2.ikey == m.ikey && m2.ival == m.ival);
    if (n_nodes) {
      uint8_t* s_dig = static_cast<uint8_t*>(malloc(32 * (n_nodes - 1) + 1));
      memset(s_dig, 0x5a, 32 * (n_nodes - 1) + 1);
      uint64_t s_nodes = 0, s_bytes = 0;
      CHECK(sbh::deliver(b, g_root, &s_nodes, &s_bytes, nullptr, 0, nullptr, n_nodes - 1, s_dig) == sbh::TOO_SMALL);
      CHECK(s_nodes == n_nodes && s_bytes == n_bytes);
      for (uint64_t k = 0; k < 32 * (n_nodes - 1); ++k) CHECK(s_dig[k] == 0x5a);
      free(s_dig);
    }
    // inserted, the new root's nodes are all there: the same batch again from it (its sets re-set, its removals
    // now of absent keys) changes nothing
    suh::add_hashed(st, b);
    sbh::Built b3;
    suh::Merged m3;
    if (n) {
      CHECK(suh::update(ssh::view(st), g_root, keys, koff, vals, voff, n, b3, m3, true) == suh::OK);
      CHECK(memcmp(b3.root, g_root, 32) == 0);
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
  free(x_blob);
  free(x_beg);
  free(x_end);
  free(x_dig);
  free(x_table);
  free(soff);
  free(sbytes);
  free(old_root);
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
  if (fread(magic, 1, 4, g_in) != 4 || memcmp(magic, "SAC1", 4) != 0) {
    printf("not a case file\n");
    return 2;
  }
  const uint32_t cases = one<uint32_t>();
  for (uint32_t k = 0; k < cases && !g_fail; ++k) run_case(k);
  fclose(g_in);
  if (g_fail) return 1;
  printf("stateapplycheck: %u cases ok\n", cases);
  return 0;
}
