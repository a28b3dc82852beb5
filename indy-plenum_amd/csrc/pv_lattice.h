// Half-size scalars for the cofactorless verification equation
// (Pornin 2020, "Optimized lattice basis reduction in dimension 2, and fast
// Schnorr and EdDSA signature verification", restated for libsodium's exact
// verdicts).
//
// libsodium 1.0.18 accepts iff encode(R') == R (32 bytes) with
// R' = S*B - h*A.  Decoding R to a point P_R
// succeeds exactly for the canonical encodings (y < p, on the curve, and
// x != 0 or sign bit 0 -- x == 0 encodings are on the small-order blocklist
// anyway), so encode(R') == R  <=>  P_R decodes and R' == P_R.  The group
// E(F_p) is cyclic of order 8L; for an ODD d with 0 < d < L,
//     R' == P_R  <=>  d (R' - P_R) == O
//                <=>  (d S mod L) B + c (-A) + d (-P_R) == O
// whenever c == d h (mod 8L): then c A == (d h) A for every curve point A,
// including mixed-order keys, and B has order L.  So the verdict stays
// bit-identical while the variable-base scalars c and d are ~128 bits
// instead of 253: half the doublings.
//
// (c, d) comes from Euclid's algorithm on (8L, h), which walks the lattice
// {(c, d) : c == d h (mod 8L)}: a_i = (r_i, t_i) with r_i == t_i h, r_i
// decreasing, |t_i| increasing, sign(t_i) = (-1)^(i+1).  At the first r_i <
// 2^128, |t_i| <= 8L / r_{i-1} < 2^128.  If t_i is even, a_{i-1} - k a_i
// (t_{i-1} is odd: consecutive t are coprime) with the smallest k that brings
// the r part under the window bound is used.  Signatures for which no vector
// fits 132-bit signed-digit windows (or with a quotient >= 2^32 on the way)
// are DEFERRED to the full-length path: ~0.2 % of random h (tools/lattice_sim
// statistics in DESIGN.md §4); the verdict never depends on which path runs.
#pragma once
#include <stdint.h>
#include <math.h>
#include "pv_scalar.h"

namespace pv {

// |c|, d < HS_MAX so that c + 0x88..8 (33 nibbles) < 2^132: 33 signed radix-16
// digits in [-8, 8), i.e. 32 windows of 4 doublings.
constexpr int HS_WORDS = 5;   // 160-bit |c|, d (plus the digit offset)
constexpr int HS_T = 6;       // |t| during the reduction (< 2^161 after the last step)
constexpr uint32_t HS_NONE = 0, HS_HALF = 1, HS_DEFER = 2;

// 8L = the order of E(F_p), 8 little-endian words
PV_HD uint32_t sc_8L(int i) {
  const uint32_t v[8] = {0xe7ae9f68u, 0xc09318d2u, 0x17bce6b2u, 0xa6f7cef5u, 0u, 0u, 0u, 0x80000000u};
  return v[i];
}

// value of 8 words as a double (relative error < 2^-50: all terms positive)
PV_HD double words_to_f64(const uint32_t r[8]) {
  double x = (double)r[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) x = x * 4294967296.0 + (double)r[k];
  return x;
}

PV_HD bool ge2_128(const uint32_t r[8]) { return (r[4] | r[5] | r[6] | r[7]) != 0; }

// a >= b (8 words)
PV_HD bool ge8(const uint32_t a[8], const uint32_t b[8]) {
  bool gt = false, decided = false;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    if (!decided && a[k] != b[k]) {
      gt = a[k] > b[k];
      decided = true;
    }
  }
  return !decided || gt;
}

PV_HD void add8(uint32_t a[8], const uint32_t b[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = __builtin_addc(a[k], b[k], c, &c);
#else
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c += (uint64_t)a[k] + b[k];
    a[k] = (uint32_t)c;
    c >>= 32;
  }
#endif
}

PV_HD void sub8(uint32_t a[8], const uint32_t b[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned bw = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = __builtin_subc(a[k], b[k], bw, &bw);
#else
  uint32_t br = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t d = (uint64_t)a[k] - b[k] - br;
    a[k] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
#endif
}

// a -= q b over 8 words; returns true iff the exact result is negative (then a
// holds it mod 2^256; callers know it lies in (-b, 0))
PV_HD bool submul8(uint32_t a[8], const uint32_t b[8], uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
  // device: the eight products q b_k are independent (one v_mad_u64_u32 each);
  // their low words and the previous product's high word leave a[k] through two
  // borrow chains (v_subb_co_u32 with carry in/out) instead of 64-bit sign tricks
  uint32_t lo[8], hi[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t p = (uint64_t)q * b[k];
    lo[k] = (uint32_t)p;
    hi[k] = (uint32_t)(p >> 32);
  }
  unsigned b1 = 0, b2 = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned o1, o2;
    const uint32_t t = __builtin_subc(a[k], lo[k], b1, &o1);
    a[k] = __builtin_subc(t, k ? hi[k - 1] : 0u, b2, &o2);
    b1 = o1;
    b2 = o2;
  }
  return (hi[7] | b1 | b2) != 0;
#else
  uint64_t pc = 0;
  uint32_t br = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t p = (uint64_t)q * b[k] + pc;
    pc = p >> 32;
    const uint64_t d = (uint64_t)a[k] - (uint32_t)p - br;
    a[k] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  return (pc + br) != 0;
#endif
}

// t += q u (HS_T words; no overflow by the bounds above)
PV_HD void addmul_t(uint32_t t[HS_T], const uint32_t u[HS_T], uint32_t q) {
#if defined(__HIP_DEVICE_COMPILE__)
  // independent products, their low and (shifted) high words added by two carry chains
  uint32_t lo[HS_T], hi[HS_T];
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    const uint64_t p = (uint64_t)q * u[k];
    lo[k] = (uint32_t)p;
    hi[k] = (uint32_t)(p >> 32);
  }
  unsigned c1 = 0, c2 = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    const uint32_t x = __builtin_addc(t[k], lo[k], c1, &c1);
    t[k] = __builtin_addc(x, k ? hi[k - 1] : 0u, c2, &c2);
  }
#else
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    const uint64_t p = (uint64_t)q * u[k] + t[k] + c;
    t[k] = (uint32_t)p;
    c = p >> 32;
  }
#endif
}

PV_HD void add_t(uint32_t t[HS_T], const uint32_t u[HS_T]) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned cc = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) t[k] = __builtin_addc(t[k], u[k], cc, &cc);
#else
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    c += (uint64_t)t[k] + u[k];
    t[k] = (uint32_t)c;
    c >>= 32;
  }
#endif
}

PV_HD void sub_t(uint32_t t[HS_T], const uint32_t u[HS_T]) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned bw = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) t[k] = __builtin_subc(t[k], u[k], bw, &bw);
#else
  uint32_t br = 0;
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    const uint64_t d = (uint64_t)t[k] - u[k] - br;
    t[k] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
#endif
}

// One exact Euclid step (ra >= rb > 0): q = floor(ra / rb),
// (ra, ta) <- (ra - q rb, ta + q tb).  q is estimated in float64 (within one
// of the true quotient while q < 2^32) and fixed by one conditional add or
// subtract of rb.  false: quotient too large for one 32-bit step (deferred).
// floor(a / b) within one: the device takes the hardware reciprocal and two
// Newton steps (relative error ~2^-50, so below 2^-18 absolute while the
// quotient is < 2^32) instead of the correctly rounded division sequence; the
// callers correct the quotient by one either way
PV_HD double quot_est(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(b);
  r = fma(r, fma(-b, r, 1.0), r);
  r = fma(r, fma(-b, r, 1.0), r);
  return floor(a * r);
#else
  return floor(a / b);
#endif
}

PV_HD bool euclid_step(uint32_t ra[8], uint32_t ta[HS_T], const uint32_t rb[8], const uint32_t tb[HS_T]) {
  const double qd = quot_est(words_to_f64(ra), words_to_f64(rb));
  if (!(qd < 4294967294.0)) return false;
  const uint32_t q = (uint32_t)qd;
  if (submul8(ra, rb, q)) {          // over-estimate by one
    add8(ra, rb);
    addmul_t(ta, tb, q);
    sub_t(ta, tb);
  } else {
    addmul_t(ta, tb, q);
    if (ge8(ra, rb)) {               // under-estimate by one
      sub8(ra, rb);
      add_t(ta, tb);
    }
  }
  return true;
}

// v (nw words) + 0x88..8 (33 nibbles) < 2^132: v fits the signed-digit windows
PV_HD bool fits132(const uint32_t* v, int nw) {
  uint32_t hi = 0;
  for (int k = HS_WORDS; k < nw; ++k) hi |= v[k];
  if (hi) return false;
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c = ((uint64_t)v[k] + 0x88888888u + c) >> 32;
  return (uint64_t)v[4] + 8u + c < 16u;
}

// (ra, ta) <-> (rb, tb)
PV_HD void hs_swap(uint32_t ra[8], uint32_t ta[HS_T], uint32_t rb[8], uint32_t tb[HS_T]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t x = ra[k];
    ra[k] = rb[k];
    rb[k] = x;
  }
#pragma unroll
  for (int k = 0; k < HS_T; ++k) {
    const uint32_t x = ta[k];
    ta[k] = tb[k];
    tb[k] = x;
  }
}

// Euclid on a_{i-1} = (ra, ta), a_i = (rb, tb) down to the first r_i < 2^128,
// one exact full-width step at a time; odd = parity of i.  Two steps per trip
// so the roles alternate without swapping registers; the exit swaps once.
// false: deferred (a quotient too large for one step, or more than 192 steps).
PV_HD bool hs_euclid_classic(uint32_t ra[8], uint32_t ta[HS_T], uint32_t rb[8], uint32_t tb[HS_T], uint32_t& odd) {
  int trips = 0;
#pragma unroll 1
  for (;;) {
    if (!ge2_128(rb)) break;
    if (++trips > 96 || !euclid_step(ra, ta, rb, tb)) return false;  // ra <- r_{i+1}
    odd ^= 1u;
    if (!ge2_128(ra)) {
      hs_swap(ra, ta, rb, tb);
      break;
    }
    if (!euclid_step(rb, tb, ra, ta)) return false;                   // rb <- r_{i+1}
    odd ^= 1u;
  }
  return true;
}

// ---- the same reduction by Lehmer rounds (what half_scalars runs) ----
// A round runs Euclid on the leading 53 bits of (ra, rb) only, collects the
// quotients it can PROVE equal to the full-width ones in a 2x2 cofactor matrix
// of magnitudes below 2^27, and applies the matrix to the long operands once.  The
// partial quotients, the exit (first r_i < 2^128, always reached by an exact
// full-width step) and hence every output word are those of hs_euclid_classic,
// which stays as the host tests' reference (half_scalars_classic below).
//
// With ra = xa 2^s + ea, rb = xb 2^s + eb (0 <= ea, eb < 2^s) and the cofactor
// magnitudes u_j, v_j (u_{-1} = 1, v_{-1} = 0, u_0 = 0, v_0 = 1,
// w_{j+1} = w_{j-1} + q_j w_j), r_j = (-1)^(j+1) (u_j ra - v_j rb), so the
// leading-word remainder x_j = (-1)^(j+1) (u_j xa - v_j xb) brackets the true
// one: r_j / 2^s lies in (x_j - v_j, x_j + v_j) (u_j <= v_j for j >= 0).  The
// quotient q = floor(x_{j-1} / x_j) is the full-width one iff 0 <= r_{j+1} <
// r_j, which follows from (Jebelean's condition, with v for both cofactors)
//     x_{j+1} >= v_{j+1}   and   x_j - x_{j+1} >= v_{j+1} + v_j.
// The first is strengthened to x_{j+1} >= v_{j+1} + T, T = ceil(2^128 / 2^s),
// which proves r_{j+1} >= 2^128: a round never steps to or past the exit.
constexpr int HS_MAX_STEPS = 192;   // the classical loop's 96 trips of two steps
constexpr double HS_COF_CAP = 134217728.0;   // cofactors below 2^27: half the 53-bit window and a bit
constexpr int HS_MAX_INNER = 48;    // v_j >= Fibonacci(j + 1), which passes 2^27 at j = 40
constexpr double HS_QSCALE = 1.0 - 0x1p-44;

// host-side statistics of one reduction (tools/hostcheck; never passed on the device)
struct HsStats {
  uint32_t rounds, inner, fallback, zero_rounds, exit_in_fallback;
  uint8_t k[HS_MAX_STEPS + 1];   // proven steps of each round, in order (0: a fallback step)
};

// out = A x - B y (SUB) or A x + B y over N words, mod 2^(32 N); the callers'
// exact results are non-negative and fit
template <int N, bool SUB>
PV_HD void lincomb(uint32_t out[N], uint32_t A, const uint32_t x[N], uint32_t B, const uint32_t y[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
  // independent products; low and (shifted) high words joined by one carry
  // chain per product, the two sums by a third
  uint32_t pl[N], ph[N], ml[N], mh[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint64_t p = (uint64_t)A * x[k], m = (uint64_t)B * y[k];
    pl[k] = (uint32_t)p;
    ph[k] = (uint32_t)(p >> 32);
    ml[k] = (uint32_t)m;
    mh[k] = (uint32_t)(m >> 32);
  }
  unsigned c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t p = __builtin_addc(pl[k], k ? ph[k - 1] : 0u, c1, &c1);
    const uint32_t m = __builtin_addc(ml[k], k ? mh[k - 1] : 0u, c2, &c2);
    out[k] = SUB ? __builtin_subc(p, m, c3, &c3) : __builtin_addc(p, m, c3, &c3);
  }
#else
  uint64_t cp = 0, cm = 0, c = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint64_t p = (uint64_t)A * x[k] + cp, m = (uint64_t)B * y[k] + cm;
    cp = p >> 32;
    cm = m >> 32;
    if (SUB) {
      const uint64_t d = (uint64_t)(uint32_t)p - (uint32_t)m - c;
      out[k] = (uint32_t)d;
      c = d >> 63;
    } else {
      const uint64_t s = (uint64_t)(uint32_t)p + (uint32_t)m + c;
      out[k] = (uint32_t)s;
      c = s >> 32;
    }
  }
#endif
}

// (hi:lo) << z, upper word; 0 <= z < 32
PV_HD uint32_t shl_hi(uint32_t hi, uint32_t lo, uint32_t z) { return z ? (hi << z) | (lo >> (32u - z)) : hi; }

// floor(x / y) within one from below, for integer-valued x >= y > 0 below 2^53:
// the float64 estimate (relative error < 2^-48 either way) is scaled by
// 1 - 2^-44, so while the quotient is below 2^27 it is q or q - 1, never above
PV_HD double quot53_est(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(y);
  r = fma(r, fma(-y, r, 1.0), r);
  r = fma(r, fma(-y, r, 1.0), r);
  return floor(x * r * HS_QSCALE);
#else
  return floor(x / y * HS_QSCALE);
#endif
}

// One round on the leading 53 bits of ra > rb >= 2^128: the number k of proven
// steps (0: none) and their matrix (u0, v0, u1, v1) = (u_{k-1}, v_{k-1}, u_k,
// v_k).  -1: the inner loop overran its bound (cannot happen; deferred).
// The window, the remainders and the cofactors are integers below 2^53 held in
// float64, where every product, sum and difference below is exact: the GPU has
// no 64-bit divide, and its float64 rate is that of its 32-bit integer adds.
PV_HD int lehmer_round(const uint32_t ra[8], const uint32_t rb[8], uint32_t& u0, uint32_t& v0, uint32_t& u1,
                       uint32_t& v1) {
  // the three leading words of ra (top one non-zero, word index w >= 4) and rb's
  // at the same place, by selects: no indexed access to the register arrays
  uint32_t a2 = ra[7], a1 = ra[6], a0 = ra[5], b2 = rb[7], b1 = rb[6], b0 = rb[5];
  uint32_t w = 7;
#pragma unroll
  for (int k = 4; k >= 2; --k) {
    if (a2 == 0) {
      a2 = a1; a1 = a0; a0 = ra[k];
      b2 = b1; b1 = b0; b0 = rb[k];
      --w;
    }
  }
  u0 = 1; v0 = 0; u1 = 0; v1 = 1;
  if (a2 == 0) return 0;               // ra < 2^128: outside the loop's invariant
  const uint32_t z = (uint32_t)__builtin_clz(a2);
  // the leading 64 bits (shift counts 1..31 only), then their upper 53:
  // s = 32 (w - 1) - z + 11 and T = 2^(128 - s), or 1 once s >= 128
  const uint64_t x64 = ((uint64_t)shl_hi(a2, a1, z) << 32) | shl_hi(a1, a0, z);
  const uint64_t y64 = ((uint64_t)shl_hi(b2, b1, z) << 32) | shl_hi(b1, b0, z);
  const uint64_t T64 = w == 4 ? (uint64_t)(1u << z) << 32 : (w == 5 ? (uint64_t)(1u << z) : 1u);
  double x = (double)(x64 >> 11), y = (double)(y64 >> 11);
  const double T = (T64 >> 11) ? (double)(T64 >> 11) : 1.0;
  if (!(y > 0.0) || x < y) return 0;
  double du0 = 1.0, dv0 = 0.0, du1 = 0.0, dv1 = 1.0;
  int k = 0;
#pragma unroll 1
  for (; k < HS_MAX_INNER; ++k) {
    double q = quot53_est(x, y);
    double rem = x - q * y;                          // q y <= x: exact
    const bool up = rem >= y;
    rem -= up ? y : 0.0;
    q += up ? 1.0 : 0.0;
    const double nv = q * dv1 + dv0;                 // exact below the cap; above it, above it
    // cofactor cap (and with it q < 2^27, where the estimate holds);
    // r_{j+1} >= 2^128 proven; r_{j+1} < r_j proven
    if (!(nv < HS_COF_CAP && rem >= nv + T && y - rem >= nv + dv1)) break;
    const double nu = q * du1 + du0;
    x = y; y = rem;
    du0 = du1; du1 = nu;
    dv0 = dv1; dv1 = nv;
  }
  u0 = (uint32_t)du0; v0 = (uint32_t)dv0; u1 = (uint32_t)du1; v1 = (uint32_t)dv1;
  return k < HS_MAX_INNER ? k : -1;
}

PV_HD bool hs_euclid_lehmer(uint32_t ra[8], uint32_t ta[HS_T], uint32_t rb[8], uint32_t tb[HS_T], uint32_t& odd,
                            HsStats* stats = nullptr) {
  // a_{i-1} = (ra, ta), a_i = (rb, tb) at the top of every trip; every trip
  // takes at least one step, so HS_MAX_STEPS + 1 trips bound the loop
  int steps = 0;
#pragma unroll 1
  for (int trip = 0; trip <= HS_MAX_STEPS; ++trip) {
    if (!ge2_128(rb)) return true;
    if (steps >= HS_MAX_STEPS) return false;         // the classical loop's trips > 96
    uint32_t u0, v0, u1, v1;
    const int k = lehmer_round(ra, rb, u0, v0, u1, v1);
    if (k < 0) return false;
    if (stats) {
      stats->k[stats->rounds] = (uint8_t)k;
      ++stats->rounds;
      stats->inner += (uint32_t)k;
      stats->zero_rounds += k == 0;
    }
    if (k == 0) {
      // nothing proven (a large quotient, leading words too close, or the exit
      // within reach): one exact full-width step, as the classical loop takes it
      if (!euclid_step(ra, ta, rb, tb)) return false;
      hs_swap(ra, ta, rb, tb);
      steps += 1;
      odd ^= 1u;
      if (stats) {
        ++stats->fallback;
        stats->exit_in_fallback += !ge2_128(rb);
      }
      continue;
    }
    // k even: (r_{k-1}, r_k) = (u0 ra - v0 rb, v1 rb - u1 ra); k odd: the
    // negatives.  |t_{k-1}|, |t_k| = u0 ta + v0 tb, u1 ta + v1 tb either way.
    uint32_t na[8], nb[8], sa[HS_T], sb[HS_T];
    if (k & 1) {
      lincomb<8, true>(na, v0, rb, u0, ra);
      lincomb<8, true>(nb, u1, ra, v1, rb);
    } else {
      lincomb<8, true>(na, u0, ra, v0, rb);
      lincomb<8, true>(nb, v1, rb, u1, ra);
    }
    lincomb<HS_T, false>(sa, u0, ta, v0, tb);
    lincomb<HS_T, false>(sb, u1, ta, v1, tb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ra[j] = na[j];
      rb[j] = nb[j];
    }
#pragma unroll
    for (int j = 0; j < HS_T; ++j) {
      ta[j] = sa[j];
      tb[j] = sb[j];
    }
    steps += k;
    odd ^= (uint32_t)k & 1u;
  }
  return false;                                       // trip bound (cannot happen)
}

// The selection after the reduction: a_{i-1} = (ra, ta), a_i = (rb, tb) with
// r_i the first remainder < 2^128, odd = parity of i.
PV_HD uint32_t hs_select(uint32_t c[HS_WORDS], uint32_t d[HS_WORDS], bool& c_neg, uint32_t ra[8], uint32_t ta[HS_T],
                         const uint32_t rb[8], const uint32_t tb[HS_T], uint32_t odd) {
  if (tb[0] & 1u) {
    // a_i itself: r_i < 2^128, |t_i| < 2^128; t_i < 0 iff i even
    c_neg = odd == 0;
#pragma unroll
    for (int k = 0; k < HS_WORDS; ++k) {
      c[k] = rb[k];
      d[k] = tb[k];
    }
    return HS_HALF;
  }
  // t_i even: a_{i-1} - k a_i for the smallest k >= 0 with r <= bound
  // (t_{i-1} odd, opposite sign to t_i, so |t| = |t_{i-1}| + k |t_i|)
  if (!fits132(ra, 8)) {
    if ((rb[0] | rb[1] | rb[2] | rb[3]) == 0) return HS_DEFER;   // r_i = 0 (cannot happen)
    // k ~ (ra - target) / rb rounded up, target 2.5e39 just under the bound
    // 0x77..78 (33 nibbles) = 2.54e39; one more subtraction if it fell short
    const double kd = ceil((words_to_f64(ra) - 2.5e39) / words_to_f64(rb));
    if (!(kd < 4294967294.0)) return HS_DEFER;
    const uint32_t k = kd > 0.0 ? (uint32_t)kd : 0u;
    if (submul8(ra, rb, k)) return HS_DEFER;
    addmul_t(ta, tb, k);
    if (!fits132(ra, 8)) {
      sub8(ra, rb);
      add_t(ta, tb);
    }
    if (!fits132(ra, 8)) return HS_DEFER;
  }
  if (!fits132(ta, HS_T)) return HS_DEFER;
  c_neg = odd == 1;
#pragma unroll
  for (int k = 0; k < HS_WORDS; ++k) {
    c[k] = ra[k];
    d[k] = ta[k];
  }
  return HS_HALF;
}

PV_HD void hs_init(uint32_t ra[8], uint32_t ta[HS_T], uint32_t rb[8], uint32_t tb[HS_T], const uint32_t h[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ra[k] = sc_8L(k);
    rb[k] = h[k];
  }
#pragma unroll
  for (int k = 0; k < HS_T; ++k) ta[k] = tb[k] = 0;
  tb[0] = 1;
}

// h (< L, 8 words) -> |c|, d (HS_WORDS words each) with c == d h (mod 8L),
// d odd and positive, |c|, d within the 132-bit windows; c_neg = sign of c.
// Returns HS_HALF, or HS_DEFER when no such pair was found (see header).
PV_HD uint32_t half_scalars(uint32_t c[HS_WORDS], uint32_t d[HS_WORDS], bool& c_neg, const uint32_t h[8]) {
  uint32_t ra[8], rb[8], ta[HS_T], tb[HS_T];
  hs_init(ra, ta, rb, tb, h);
  uint32_t odd = 1;
  if (!hs_euclid_lehmer(ra, ta, rb, tb, odd)) return HS_DEFER;
  return hs_select(c, d, c_neg, ra, ta, rb, tb, odd);
}

#if !defined(__HIPCC__)
// host builds only: the classical loop (the tests' reference), and the Lehmer
// rounds with their statistics
inline uint32_t half_scalars_classic(uint32_t c[HS_WORDS], uint32_t d[HS_WORDS], bool& c_neg, const uint32_t h[8]) {
  uint32_t ra[8], rb[8], ta[HS_T], tb[HS_T];
  hs_init(ra, ta, rb, tb, h);
  uint32_t odd = 1;
  if (!hs_euclid_classic(ra, ta, rb, tb, odd)) return HS_DEFER;
  return hs_select(c, d, c_neg, ra, ta, rb, tb, odd);
}

inline uint32_t half_scalars_lehmer(uint32_t c[HS_WORDS], uint32_t d[HS_WORDS], bool& c_neg, const uint32_t h[8],
                                    HsStats* stats) {
  uint32_t ra[8], rb[8], ta[HS_T], tb[HS_T];
  hs_init(ra, ta, rb, tb, h);
  uint32_t odd = 1;
  if (!hs_euclid_lehmer(ra, ta, rb, tb, odd, stats)) return HS_DEFER;
  return hs_select(c, d, c_neg, ra, ta, rb, tb, odd);
}
#endif

// v + 0x88..8 (33 nibbles), in place: the offset form whose nibble w minus 8
// is signed digit w (callers guarantee fits132)
PV_HD void hs_offset(uint32_t v[HS_WORDS]) {
  uint64_t c = 0;
#pragma unroll
  for (int k = 0; k < HS_WORDS; ++k) {
    c += (uint64_t)v[k] + (k < 4 ? 0x88888888u : 0x8u);
    v[k] = (uint32_t)c;
    c >>= 32;
  }
}

// s' = d * S mod L (d: HS_WORDS words, S: 8 words)
PV_HD void sc_mul_small(uint32_t out[8], const uint32_t d[HS_WORDS], const uint32_t S[8]) {
  uint32_t x[16];
  uint64_t carry = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    uint64_t acc = carry & 0xffffffffu;
    uint64_t acchi = carry >> 32;
#pragma unroll
    for (int i = 0; i < HS_WORDS; ++i) {
      const int j = k - i;
      if (j >= 0 && j < 8) {
        const uint64_t p = mul32x32(d[i], S[j]);
        acc += p & 0xffffffffu;
        acchi += p >> 32;
      }
    }
    acchi += acc >> 32;
    x[k] = (uint32_t)acc;
    carry = acchi;
  }
  sc_reduce64(out, x);
}

}  // namespace pv
