// Sorting state keys, shared by device and host: the step before pv_trie_build.h
// for keys that are not in order yet (pv_state_sort_device and the fused
// pv_state_build_unsorted_device / pv_state_apply_unsorted_device).
//
// Order.  Bytewise with a proper prefix first: the order tb_lcp_one checks, so
// b"ab" < b"ab\x00" < b"ab\x00\x00" < b"ab\x01".  Duplicates.  Of equal keys the
// occurrence with the highest input index stays ("the last of equal keys wins"
// of the host forms).  Nothing is read from the values, no input is written; the
// result is perm[k] = the input index of the k-th kept key, and the kept count.
//
// Rounds over 8-byte words.  In round r key i contributes
//   word  = its bytes [8 r, 8 r + 8) big-endian, zero-padded,
//   valid = clamp(len - 8 r, 0, 8): padding is told from a real 0x00.
// Two keys that agree in every earlier round compare in round r as
// (word, valid): where the words differ inside both keys the bytes decide;
// where one key has ended its padding 0x00 is below or equal to the other's
// byte, and on a tie the smaller valid, the proper prefix, goes first.  A key
// with valid < 8 is finished after that round.
//
// Composite.  (segment, word, valid), one 16-byte record per position with the
// key's input index.  A segment is a run of positions whose keys agree in every
// earlier composite; round 0 has one segment.  Its id is the run's rank (the
// number of runs before it), not the position of its first key: the rank is
// what one exclusive sum scan of the boundary flags gives (the library's scan
// is a sum scan), it orders the runs the same way, and it needs the fewest
// digits (ts_seg_digits), so the common case of few runs sorts fewer passes.
//
// Each round is a stable LSD radix sort of the records by the composite, 8 bits
// per pass (ts_digit): valid, the 8 bytes of word, then the bytes of segment
// that the run count needs.  A pass is a per-block histogram in LDS, one
// exclusive scan of the 256 x blocks table (digit-major, so the scan's order is
// digit, then block), and a scatter.  Stability of the scatter: a block owns the
// TS_TILE consecutive positions of its tile and takes them in TS_ITEMS chunks of
// 256; within a chunk wave w holds positions 64 w .. 64 w + 63.  A record's slot
// is  table[digit][block]  (all smaller digits, and this digit in earlier
// blocks) + the records of this digit in earlier chunks of the tile (a running
// count in LDS) + those in earlier waves of the chunk (per-wave counts in LDS) +
// those in lower lanes of its wave (the ballot match).  Every term counts
// records that come earlier in the input, so ties keep the input order.  No
// global atomics order anything.  As every round is stable and round 0 starts
// from the identity, equal keys stay in input order: the last of a run of equal
// keys is the one with the highest input index.
//
// After a round the flag pass (ts_flag_one) marks the first position of every
// run of equal composites and the positions that are unresolved: valid == 8 in
// a run of more than one.  One scan of the packed flags gives every position
// its run's rank (for the next round's segment), the run count and the
// unresolved count; the host reads that one word and stops at 0.  Then the runs
// of more than one key are exactly the keys equal in full, ts_keep_one keeps the
// last of each run and the rank is its output position: perm and the kept count
// need no further scan.  Every round runs over all n positions.
//
// Cost: one round per 8 bytes that two distinct keys share, plus one when equal
// keys end on a word boundary: 1 for random 32-byte keys, len / 8 (+ 1) for keys
// that differ in their last word only.  Rounds are at most
// ceil(max_len / 8) + 1 <= TS_MAX_ROUNDS; keys above TS_MAX_KEY_BYTES are refused
// (the host forms sort any length).  Temporaries: two records (32 bytes), one
// scan word (8 bytes) per key, and 8 bytes per 8 positions for the digit table.
//
// Bounds.  Every loop is bounded by 8 (a word, a digit), TS_ITEMS or the round
// limit.  Key bytes are read one at a time and only below the key's length, so
// keys may start at any byte offset and nothing past a key is read.
//
// The host twin (tools/hostcheck/statesort_host.h) is these routines called in
// index order with a std::stable_sort on the composite per round.
#pragma once
#include <stdint.h>

#ifndef PV_HD
#define PV_HD __host__ __device__ __forceinline__
#endif

namespace pv {

constexpr uint64_t TS_MAX_KEY_BYTES = 1024;
constexpr uint32_t TS_MAX_ROUNDS = (uint32_t)(TS_MAX_KEY_BYTES / 8) + 1;
constexpr uint32_t TS_BLOCK = 256;   // threads of the histogram and scatter kernels
constexpr uint32_t TS_ITEMS = 8;     // chunks of TS_BLOCK positions per tile
constexpr uint32_t TS_TILE = 2048;   // the scatter kernel's items per block
static_assert(TS_TILE == TS_BLOCK * TS_ITEMS, "a tile is TS_ITEMS chunks");
constexpr uint64_t TS_VAL_MAX = 1ull << 30;   // TB_MAX_VAL_BYTES of pv_trie_build.h

enum : uint32_t { TS_BAD_OFFSET = 1, TS_BAD_LENGTH = 2, TS_BAD_VALUE = 4 };

// One position of the current order.  sv = segment << 4 | valid: segment < 2^28 (TB_MAX_KEYS).
struct alignas(16) TsRec {
  uint64_t word;
  uint32_t sv;
  uint32_t idx;
};

// the checks of input i: both offset arrays monotone (val_off may be null: keys alone), the key
// at most TS_MAX_KEY_BYTES, the value at most 2^30 bytes and, unless empty_ok, not empty
PV_HD uint32_t ts_check_one(const uint64_t* key_off, const uint64_t* val_off, uint64_t i, bool empty_ok) {
  uint32_t bad = 0;
  const uint64_t a = key_off[i], b = key_off[i + 1];
  if (b < a) bad |= TS_BAD_OFFSET;
  else if (b - a > TS_MAX_KEY_BYTES) bad |= TS_BAD_LENGTH;
  if (val_off) {
    const uint64_t va = val_off[i], vb = val_off[i + 1];
    if (vb < va) bad |= TS_BAD_OFFSET;
    else if (vb - va > TS_VAL_MAX || (vb == va && !empty_ok)) bad |= TS_BAD_VALUE;
  }
  return bad;
}

PV_HD uint32_t ts_valid(uint64_t len, uint32_t r) {
  const uint64_t at = 8ull * r;
  if (len <= at) return 0;
  return len - at >= 8 ? 8u : (uint32_t)(len - at);
}

// bytes [8 r, 8 r + 8) of key, big-endian, zero beyond len; byte loads below len only
PV_HD uint64_t ts_word(const uint8_t* key, uint64_t len, uint32_t r) {
  const uint32_t v = ts_valid(len, r);
  uint64_t w = 0;
  for (uint32_t t = 0; t < 8; ++t)
    if (t < v) w |= (uint64_t)key[8ull * r + t] << (56 - 8 * t);
  return w;
}

// round r's record of input idx in segment seg
PV_HD TsRec ts_make(const uint8_t* key_blob, const uint64_t* key_off, uint32_t idx, uint32_t seg, uint32_t r) {
  const uint64_t o = key_off[idx], len = key_off[idx + 1] - o;
  TsRec x;
  x.word = ts_word(key_blob + o, len, r);
  x.sv = seg << 4 | ts_valid(len, r);
  x.idx = idx;
  return x;
}

PV_HD bool ts_same(const TsRec& a, const TsRec& b) { return a.word == b.word && a.sv == b.sv; }

// composite a before composite b: (segment, word, valid)
PV_HD bool ts_less(const TsRec& a, const TsRec& b) {
  if ((a.sv >> 4) != (b.sv >> 4)) return (a.sv >> 4) < (b.sv >> 4);
  if (a.word != b.word) return a.word < b.word;
  return (a.sv & 15u) < (b.sv & 15u);
}

// bytes of segment a round sorts by when its records lie in n_seg runs
PV_HD uint32_t ts_seg_digits(uint64_t n_seg) {
  uint32_t d = 0;
  for (uint64_t top = n_seg ? n_seg - 1 : 0; top && d < 4; top >>= 8) ++d;
  return d;
}

// the 8-bit digit of LSD pass p: 0 = valid, 1 .. 8 = word from its low byte, 9 .. = segment from its low byte
PV_HD uint32_t ts_digit(const TsRec& x, uint32_t p) {
  if (p == 0) return x.sv & 15u;
  if (p <= 8) return (uint32_t)(x.word >> (8 * (p - 1))) & 255u;
  return ((x.sv >> 4) >> (8 * (p - 9))) & 255u;
}

// position k of the sorted records opens a run
PV_HD bool ts_boundary(const TsRec* rec, uint64_t k) { return k == 0 || !ts_same(rec[k - 1], rec[k]); }

// the last position of its run
PV_HD bool ts_keep_one(const TsRec* rec, uint64_t n, uint64_t k) { return k + 1 == n || !ts_same(rec[k], rec[k + 1]); }

// The flag word of position k < n: bit 0 = opens a run; bit 32 = unresolved (valid == 8 in a run of
// more than one).  Summed over [0, k] the low half is the run's rank + 1; over all n the low half
// is the run count and the high half the unresolved count (both at most 2^28: no carry).
PV_HD uint64_t ts_flag_one(const TsRec* rec, uint64_t n, uint64_t k) {
  const bool first = ts_boundary(rec, k), last = ts_keep_one(rec, n, k);
  const bool open = (rec[k].sv & 15u) == 8 && !(first && last);
  return (first ? 1ull : 0ull) | (open ? 1ull << 32 : 0ull);
}

// the rank of position k's run from the exclusive scan x of the flag words (x[n] = the totals)
PV_HD uint32_t ts_rank(const uint64_t* x, uint64_t k) { return (uint32_t)(x[k + 1] & 0xffffffffull) - 1; }

}  // namespace pv
