// The sort of state keys on the host -- test tooling only.  It includes the
// product header indy-plenum_amd/csrc/pv_trie_sort.h unchanged and runs what the
// kernels of pv_state_sort_device run, sequentially and in the same order:
// ts_check_one per key, then per round ts_make per position, a stable sort of the
// records by the composite, ts_flag_one per position and one exclusive scan; at
// the end ts_keep_one and ts_rank give perm.  The sort of a round is a
// std::stable_sort with ts_less, so the word, valid and segment logic is what
// decides the order, not one memcmp; with lsd it is instead the device's
// counting passes over ts_digit (valid, the word's bytes, the segment's bytes
// that ts_seg_digits asks for), which must give the same records.  Every work
// array has its exact size.  Shared by libstatesortcheck.so and
// statesortcheck_asan.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#ifndef PV_HD
#define PV_HD static inline
#endif
#include "../../indy-plenum_amd/csrc/pv_trie_sort.h"

namespace ssoh {

enum { OK = 0, BAD_OFFSET = 1, BAD_LENGTH = 2, UNRESOLVED = 3 };

struct Sorted {
  std::vector<uint32_t> perm;   // m
  uint64_t m = 0, bad_index = 0;
  uint32_t rounds = 0;
};

// one LSD pass by digit p: the stable counting sort the histogram, scan and scatter kernels make
inline void lsd_pass(const std::vector<pv::TsRec>& in, uint32_t p, std::vector<pv::TsRec>& out) {
  uint64_t at[257] = {0};
  for (const pv::TsRec& x : in) ++at[pv::ts_digit(x, p) + 1];
  for (uint32_t d = 0; d < 256; ++d) at[d + 1] += at[d];
  for (const pv::TsRec& x : in) out[at[pv::ts_digit(x, p)]++] = x;
}

inline int sort(const uint8_t* key_blob, const uint64_t* key_off, uint64_t n, bool lsd, Sorted& out) {
  out = Sorted();
  if (n == 0) return OK;
  uint64_t first[2] = {n, n};
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t bad = pv::ts_check_one(key_off, nullptr, i, true);
    if ((bad & pv::TS_BAD_OFFSET) && first[0] == n) first[0] = i;
    if ((bad & pv::TS_BAD_LENGTH) && first[1] == n) first[1] = i;
  }
  for (int k = 0; k < 2; ++k)
    if (first[k] != n) {
      out.bad_index = first[k];
      return k == 0 ? BAD_OFFSET : BAD_LENGTH;
    }
  std::vector<pv::TsRec> rec(n), tmp(n);
  std::vector<uint64_t> x(n + 1);
  for (uint64_t i = 0; i < n; ++i) rec[i] = pv::ts_make(key_blob, key_off, (uint32_t)i, 0, 0);
  uint64_t runs = 1;
  uint32_t r = 0;
  for (;; ++r) {
    if (r >= pv::TS_MAX_ROUNDS) return UNRESOLVED;
    if (r > 0) {
      for (uint64_t k = 0; k < n; ++k) tmp[k] = pv::ts_make(key_blob, key_off, rec[k].idx, pv::ts_rank(x.data(), k), r);
      rec.swap(tmp);
    }
    if (lsd) {
      const uint32_t passes = 9 + (r > 0 ? pv::ts_seg_digits(runs) : 0);
      for (uint32_t p = 0; p < passes; ++p) {
        lsd_pass(rec, p, tmp);
        rec.swap(tmp);
      }
    } else {
      std::stable_sort(rec.begin(), rec.end(), [](const pv::TsRec& a, const pv::TsRec& b) { return pv::ts_less(a, b); });
    }
    uint64_t sum = 0;
    for (uint64_t k = 0; k < n; ++k) {
      const uint64_t f = pv::ts_flag_one(rec.data(), n, k);
      x[k] = sum;
      sum += f;
    }
    x[n] = sum;
    runs = sum & 0xffffffffull;
    if ((sum >> 32) == 0) break;
  }
  out.rounds = r + 1;
  out.m = runs;
  out.perm.assign(runs, 0xffffffffu);
  for (uint64_t k = 0; k < n; ++k)
    if (pv::ts_keep_one(rec.data(), n, k)) out.perm[pv::ts_rank(x.data(), k)] = rec[k].idx;
  return OK;
}

}  // namespace ssoh
