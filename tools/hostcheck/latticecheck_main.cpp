// Stand-alone run of the half-size scalar reduction under AddressSanitizer +
// UBSan (tools/hostcheck/Makefile: latticecheck_asan).  A program of its own,
// never loaded into Python; nothing here runs on a GPU.
//
//   latticecheck_asan CASEFILE
//
// The case file is written by tests/test_lattice_lehmer.py: "LAT1", u32 n,
// then n values of h as 32 little-endian bytes each.  Every h goes through the
// Lehmer rounds, the classical loop and half_scalars as built; the three must
// agree in status, |c|, d and sign.  The sanitizers watch the data-dependent
// shift counts of the window extraction and every array index on the way.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define PV_HD static inline
#include "../../indy-plenum_amd/csrc/pv_lattice.h"

using namespace pv;

namespace {

struct Out {
  uint32_t st, c[HS_WORDS], d[HS_WORDS], neg;
};

bool same(const Out& a, const Out& b) {
  return a.st == b.st && a.neg == b.neg && memcmp(a.c, b.c, sizeof a.c) == 0 && memcmp(a.d, b.d, sizeof a.d) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  FILE* in = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  if (!in) {
    printf("usage: latticecheck_asan CASEFILE\n");
    return 2;
  }
  char magic[4];
  uint32_t n = 0;
  if (fread(magic, 1, 4, in) != 4 || memcmp(magic, "LAT1", 4) != 0 || fread(&n, 4, 1, in) != 1) {
    printf("FAIL: not a case file\n");
    return 2;
  }
  int fail = 0;
  uint64_t rounds = 0, inner = 0, fallback = 0;
  for (uint32_t i = 0; i < n; ++i) {
    // h in a heap allocation of its exact size
    uint32_t* h = static_cast<uint32_t*>(malloc(32));
    if (fread(h, 32, 1, in) != 1) {
      printf("FAIL: the case file ends early\n");
      return 2;
    }
    Out a, b, c;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    memset(&c, 0, sizeof c);
    bool neg = false;
    HsStats s;
    memset(&s, 0, sizeof s);
    a.st = half_scalars_lehmer(a.c, a.d, neg, h, &s);
    a.neg = neg;
    neg = false;
    b.st = half_scalars_classic(b.c, b.d, neg, h);
    b.neg = neg;
    neg = false;
    c.st = half_scalars(c.c, c.d, neg, h);
    c.neg = neg;
    if (a.st != HS_HALF) memset(a.c, 0, sizeof a.c + sizeof a.d), a.neg = 0;
    if (b.st != HS_HALF) memset(b.c, 0, sizeof b.c + sizeof b.d), b.neg = 0;
    if (c.st != HS_HALF) memset(c.c, 0, sizeof c.c + sizeof c.d), c.neg = 0;
    if (!same(a, b) || !same(a, c)) {
      printf("FAIL: case %u: lehmer %u, classic %u, as built %u\n", i, a.st, b.st, c.st);
      ++fail;
    }
    if (s.rounds > (uint32_t)HS_MAX_STEPS + 1 || s.inner + s.fallback > (uint32_t)HS_MAX_STEPS + HS_MAX_INNER) {
      printf("FAIL: case %u: %u rounds, %u + %u steps\n", i, s.rounds, s.inner, s.fallback);
      ++fail;
    }
    rounds += s.rounds;
    inner += s.inner;
    fallback += s.fallback;
    free(h);
  }
  fclose(in);
  if (fail) {
    printf("latticecheck: %d failures\n", fail);
    return 1;
  }
  printf("latticecheck ok: %u cases, %llu rounds, %llu inner steps, %llu fallback steps\n", n,
         (unsigned long long)rounds, (unsigned long long)inner, (unsigned long long)fallback);
  return 0;
}
