// SHA3-256 (FIPS 202) for one lane: Keccak-f[1600], rate 136 bytes, domain
// byte 0x06, the last rate byte takes 0x80 (0x86 when both land on one byte).
// A message of len bytes has len / 136 + 1 blocks; the digest is the first 32
// bytes of the state.
//
// Used for the state trie (state/util/utils.py:7-8,156-157: sha3 =
// hashlib.sha3_256): every Patricia-trie node is named by SHA3-256 of its RLP
// (state/trie/pruning_trie.py:334-344).
//
// The state is 25 lanes of 64 bits held as 50 named 32-bit values (l0..l24,
// h0..h24); the 24 rounds are 24 instances of one round template, so every
// rotation amount and round constant is a compile-time constant and no array
// is indexed at run time.  A 64-bit rotate by a constant is two funnel shifts
// (v_alignbit_b32), or a swap of the halves for 32; theta's five-way XOR is
// two v_bitop3_b32, chi's a ^ (~b & c) one.
//
// Keccak lanes are little-endian: message words XOR into the state as loaded,
// no byte swap.  Messages start at arbitrary byte offsets: the block's aligned
// words are loaded as 4-word groups and funnelled by the misalignment, as
// sha256_window / sha256_assemble do.
//
// Over-read convention (the same as the SHA-256 path): a group is loaded iff
// its first word holds a message byte, so a lane reads at most 15 bytes past
// the end of its message and at most 3 bytes before its start (the aligned
// word that holds the first byte).  The blob therefore needs >= 16 readable
// bytes after the last message and a 4-byte aligned base.
#pragma once
#include <stdint.h>
#include "pv_sha256.h"

namespace pv {

constexpr uint32_t SHA3_RATE = 136;        // bytes per block
constexpr int SHA3_RATE_WORDS = 34;
constexpr int SHA3_Y = 36;                 // 9 groups of 4 aligned words

struct Sha3State {
  uint32_t l0, h0, l1, h1, l2, h2, l3, h3, l4, h4;
  uint32_t l5, h5, l6, h6, l7, h7, l8, h8, l9, h9;
  uint32_t l10, h10, l11, h11, l12, h12, l13, h13, l14, h14;
  uint32_t l15, h15, l16, h16, l17, h17, l18, h18, l19, h19;
  uint32_t l20, h20, l21, h21, l22, h22, l23, h23, l24, h24;
};

#if defined(__HIP_DEVICE_COMPILE__)
PV_HD uint32_t chi32(uint32_t a, uint32_t b, uint32_t c) { return (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c, 0xd2); }
#else
PV_HD uint32_t chi32(uint32_t a, uint32_t b, uint32_t c) { return a ^ (~b & c); }
#endif
PV_HD uint32_t xor5_32(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) {
  return xor3_32(xor3_32(a, b, c), d, e);
}

// (ol, oh) = (l, h) rotated left by the constant N
template <int N>
PV_HD void rotl64c(uint32_t& ol, uint32_t& oh, uint32_t l, uint32_t h) {
  if constexpr (N == 0) {
    ol = l;
    oh = h;
  } else if constexpr (N < 32) {
    ol = funnel32_(l, h, 32 - N);
    oh = funnel32_(h, l, 32 - N);
  } else if constexpr (N == 32) {
    ol = h;
    oh = l;
  } else {
    ol = funnel32_(h, l, 64 - N);
    oh = funnel32_(l, h, 64 - N);
  }
}

constexpr uint64_t keccak_rc(int r) {
  switch (r) {
    case 0: return 0x0000000000000001ull;
    case 1: return 0x0000000000008082ull;
    case 2: return 0x800000000000808aull;
    case 3: return 0x8000000080008000ull;
    case 4: return 0x000000000000808bull;
    case 5: return 0x0000000080000001ull;
    case 6: return 0x8000000080008081ull;
    case 7: return 0x8000000000008009ull;
    case 8: return 0x000000000000008aull;
    case 9: return 0x0000000000000088ull;
    case 10: return 0x0000000080008009ull;
    case 11: return 0x000000008000000aull;
    case 12: return 0x000000008000808bull;
    case 13: return 0x800000000000008bull;
    case 14: return 0x8000000000008089ull;
    case 15: return 0x8000000000008003ull;
    case 16: return 0x8000000000008002ull;
    case 17: return 0x8000000000000080ull;
    case 18: return 0x000000000000800aull;
    case 19: return 0x800000008000000aull;
    case 20: return 0x8000000080008081ull;
    case 21: return 0x8000000000008080ull;
    case 22: return 0x0000000080000001ull;
    default: return 0x8000000080008008ull;
  }
}

// lanes are numbered x + 5 y
#define PV_K_C(x, i0, i1, i2, i3, i4)                                         \
  const uint32_t c##x##l = xor5_32(s.l##i0, s.l##i1, s.l##i2, s.l##i3, s.l##i4); \
  const uint32_t c##x##h = xor5_32(s.h##i0, s.h##i1, s.h##i2, s.h##i3, s.h##i4)
// D[x] = C[x - 1] ^ rotl(C[x + 1], 1)
#define PV_K_D(x, m, p)                          \
  uint32_t d##x##l, d##x##h;                     \
  rotl64c<1>(d##x##l, d##x##h, c##p##l, c##p##h); \
  d##x##l ^= c##m##l;                            \
  d##x##h ^= c##m##h
// rho + pi: B[dst] = rotl(A[src] ^ D[src % 5], n)
#define PV_K_RP(src, dst, n, x) \
  uint32_t b##dst##l, b##dst##h; \
  rotl64c<n>(b##dst##l, b##dst##h, s.l##src ^ d##x##l, s.h##src ^ d##x##h)
// chi: A[i] = B[i] ^ (~B[j] & B[k]), j / k the next two lanes of the row
#define PV_K_CHI(i, j, k)                    \
  s.l##i = chi32(b##i##l, b##j##l, b##k##l); \
  s.h##i = chi32(b##i##h, b##j##h, b##k##h)

template <int R>
PV_HD void keccak_round(Sha3State& s) {
  PV_K_C(0, 0, 5, 10, 15, 20);
  PV_K_C(1, 1, 6, 11, 16, 21);
  PV_K_C(2, 2, 7, 12, 17, 22);
  PV_K_C(3, 3, 8, 13, 18, 23);
  PV_K_C(4, 4, 9, 14, 19, 24);
  PV_K_D(0, 4, 1);
  PV_K_D(1, 0, 2);
  PV_K_D(2, 1, 3);
  PV_K_D(3, 2, 4);
  PV_K_D(4, 3, 0);
  PV_K_RP(0, 0, 0, 0);
  PV_K_RP(1, 10, 1, 1);
  PV_K_RP(2, 20, 62, 2);
  PV_K_RP(3, 5, 28, 3);
  PV_K_RP(4, 15, 27, 4);
  PV_K_RP(5, 16, 36, 0);
  PV_K_RP(6, 1, 44, 1);
  PV_K_RP(7, 11, 6, 2);
  PV_K_RP(8, 21, 55, 3);
  PV_K_RP(9, 6, 20, 4);
  PV_K_RP(10, 7, 3, 0);
  PV_K_RP(11, 17, 10, 1);
  PV_K_RP(12, 2, 43, 2);
  PV_K_RP(13, 12, 25, 3);
  PV_K_RP(14, 22, 39, 4);
  PV_K_RP(15, 23, 41, 0);
  PV_K_RP(16, 8, 45, 1);
  PV_K_RP(17, 18, 15, 2);
  PV_K_RP(18, 3, 21, 3);
  PV_K_RP(19, 13, 8, 4);
  PV_K_RP(20, 14, 18, 0);
  PV_K_RP(21, 24, 2, 1);
  PV_K_RP(22, 9, 61, 2);
  PV_K_RP(23, 19, 56, 3);
  PV_K_RP(24, 4, 14, 4);
  PV_K_CHI(0, 1, 2);
  PV_K_CHI(1, 2, 3);
  PV_K_CHI(2, 3, 4);
  PV_K_CHI(3, 4, 0);
  PV_K_CHI(4, 0, 1);
  PV_K_CHI(5, 6, 7);
  PV_K_CHI(6, 7, 8);
  PV_K_CHI(7, 8, 9);
  PV_K_CHI(8, 9, 5);
  PV_K_CHI(9, 5, 6);
  PV_K_CHI(10, 11, 12);
  PV_K_CHI(11, 12, 13);
  PV_K_CHI(12, 13, 14);
  PV_K_CHI(13, 14, 10);
  PV_K_CHI(14, 10, 11);
  PV_K_CHI(15, 16, 17);
  PV_K_CHI(16, 17, 18);
  PV_K_CHI(17, 18, 19);
  PV_K_CHI(18, 19, 15);
  PV_K_CHI(19, 15, 16);
  PV_K_CHI(20, 21, 22);
  PV_K_CHI(21, 22, 23);
  PV_K_CHI(22, 23, 24);
  PV_K_CHI(23, 24, 20);
  PV_K_CHI(24, 20, 21);
  constexpr uint64_t rc = keccak_rc(R);
  if constexpr ((uint32_t)rc != 0) s.l0 ^= (uint32_t)rc;
  if constexpr ((uint32_t)(rc >> 32) != 0) s.h0 ^= (uint32_t)(rc >> 32);
}

#undef PV_K_C
#undef PV_K_D
#undef PV_K_RP
#undef PV_K_CHI

PV_HD void keccak_f1600(Sha3State& s) {
  keccak_round<0>(s);
  keccak_round<1>(s);
  keccak_round<2>(s);
  keccak_round<3>(s);
  keccak_round<4>(s);
  keccak_round<5>(s);
  keccak_round<6>(s);
  keccak_round<7>(s);
  keccak_round<8>(s);
  keccak_round<9>(s);
  keccak_round<10>(s);
  keccak_round<11>(s);
  keccak_round<12>(s);
  keccak_round<13>(s);
  keccak_round<14>(s);
  keccak_round<15>(s);
  keccak_round<16>(s);
  keccak_round<17>(s);
  keccak_round<18>(s);
  keccak_round<19>(s);
  keccak_round<20>(s);
  keccak_round<21>(s);
  keccak_round<22>(s);
  keccak_round<23>(s);
}

PV_HD void sha3_init(Sha3State& s) {
  s.l0 = s.h0 = s.l1 = s.h1 = s.l2 = s.h2 = s.l3 = s.h3 = s.l4 = s.h4 = 0;
  s.l5 = s.h5 = s.l6 = s.h6 = s.l7 = s.h7 = s.l8 = s.h8 = s.l9 = s.h9 = 0;
  s.l10 = s.h10 = s.l11 = s.h11 = s.l12 = s.h12 = s.l13 = s.h13 = s.l14 = s.h14 = 0;
  s.l15 = s.h15 = s.l16 = s.h16 = s.l17 = s.h17 = s.l18 = s.h18 = s.l19 = s.h19 = 0;
  s.l20 = s.h20 = s.l21 = s.h21 = s.l22 = s.h22 = s.l23 = s.h23 = s.l24 = s.h24 = 0;
}

PV_HD uint64_t sha3_blocks(uint64_t mlen) { return mlen / SHA3_RATE + 1; }

// the aligned-word window of block blk of M: 9 groups of 4 words from the
// aligned-down first byte of the block; group g is loaded iff its first word
// holds a message byte, else zero (no load issued)
PV_HD void sha3_window(uint32_t y[SHA3_Y], const uint8_t* m, uint64_t mlen, uint64_t blk) {
  const uint64_t q = (uint64_t)SHA3_RATE * blk;
  const int64_t rem = (int64_t)mlen - (int64_t)q;
  const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(m) + q) & 3u);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(m + q - mis);
#pragma unroll
  for (int g = 0; g < 9; ++g) {
    uint32_t a = 0, b = 0, c = 0, d = 0;
    if ((int64_t)(16 * g) - (int64_t)mis < rem) {
      a = wp[4 * g];
      b = wp[4 * g + 1];
      c = wp[4 * g + 2];
      d = wp[4 * g + 3];
    }
    y[4 * g] = a;
    y[4 * g + 1] = b;
    y[4 * g + 2] = c;
    y[4 * g + 3] = d;
  }
}

// block blk's 34 little-endian words from its window: funnel shift by the
// misalignment, then the padding by selects.  t = the position of the 0x06
// domain byte in this block, clamped to [0, 137]: words below it are data, the
// word holding it keeps its low t % 4 bytes and takes 0x06, words above it are
// zero; the block that holds it (the last) also takes 0x80 in byte 135.
PV_HD void sha3_assemble(uint32_t w[SHA3_RATE_WORDS], const uint32_t y[SHA3_Y], const uint8_t* m, uint64_t mlen,
                         uint64_t blk) {
  const uint64_t q = (uint64_t)SHA3_RATE * blk;
  const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(m) + q) & 3u);
  const uint64_t t64 = mlen - q;   // blk < sha3_blocks(mlen), so q <= mlen
  const int32_t t = t64 > 137 ? 137 : (int32_t)t64;
  const uint32_t rb = 8u * ((uint32_t)t & 3u);
  const uint32_t keep = (1u << rb) - 1u, pad = 0x06u << rb;
#pragma unroll
  for (int k = 0; k < SHA3_RATE_WORDS; ++k) {
    const uint32_t v = funnel32_(y[k + 1], y[k], 8u * mis);
    const uint32_t tv = (v & keep) | pad;
    w[k] = t >= 4 * k + 4 ? v : (t >= 4 * k ? tv : 0u);
  }
  if (t < (int32_t)SHA3_RATE) w[SHA3_RATE_WORDS - 1] ^= 0x80000000u;
}

// state ^= block (lanes 0..16), then the permutation
PV_HD void sha3_absorb(Sha3State& s, const uint32_t w[SHA3_RATE_WORDS]) {
  s.l0 ^= w[0];   s.h0 ^= w[1];   s.l1 ^= w[2];   s.h1 ^= w[3];   s.l2 ^= w[4];   s.h2 ^= w[5];
  s.l3 ^= w[6];   s.h3 ^= w[7];   s.l4 ^= w[8];   s.h4 ^= w[9];   s.l5 ^= w[10];  s.h5 ^= w[11];
  s.l6 ^= w[12];  s.h6 ^= w[13];  s.l7 ^= w[14];  s.h7 ^= w[15];  s.l8 ^= w[16];  s.h8 ^= w[17];
  s.l9 ^= w[18];  s.h9 ^= w[19];  s.l10 ^= w[20]; s.h10 ^= w[21]; s.l11 ^= w[22]; s.h11 ^= w[23];
  s.l12 ^= w[24]; s.h12 ^= w[25]; s.l13 ^= w[26]; s.h13 ^= w[27]; s.l14 ^= w[28]; s.h14 ^= w[29];
  s.l15 ^= w[30]; s.h15 ^= w[31]; s.l16 ^= w[32]; s.h16 ^= w[33];
  keccak_f1600(s);
}

// digest as 8 little-endian words (digest byte order)
PV_HD void sha3_digest(uint32_t out[8], const Sha3State& s) {
  out[0] = s.l0; out[1] = s.h0; out[2] = s.l1; out[3] = s.h1;
  out[4] = s.l2; out[5] = s.h2; out[6] = s.l3; out[7] = s.h3;
}

// SHA3-256(M) as 8 little-endian words
PV_HD void sha3_256_msg(uint32_t out[8], const uint8_t* m, uint64_t mlen) {
  Sha3State s;
  sha3_init(s);
  const uint64_t nb = sha3_blocks(mlen);
  for (uint64_t b = 0; b < nb; ++b) {
    uint32_t y[SHA3_Y], w[SHA3_RATE_WORDS];
    sha3_window(y, m, mlen, b);
    sha3_assemble(w, y, m, mlen, b);
    sha3_absorb(s, w);
  }
  sha3_digest(out, s);
}

}  // namespace pv
