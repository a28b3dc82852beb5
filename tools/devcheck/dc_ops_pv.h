// One case of each curve25519-side primitive, words in and words out: the
// body shared by the device check (devcheck.hip: one case per lane, compiled
// for gfx950 with the product's flags, so the asm MAD chains, the
// __builtin_addc / subc carry chains, v_rcp_f64 and the DPP quad moves) and by
// its host twins (tools/hostcheck/hostcheck.cpp: g++, the plain C++ branches of
// the same headers, bound checks on).  Only the product headers' functions are
// called; nothing here computes.
//
// Lane ops:  dc_op_<name>(in, out), IW words in and OW words out per case.
// Quad ops:  dc_qop_<name>(in, out, role): IW / OW words per QUAD, coordinate l
//            of a point at words 10 l .. 10 l + 9 (device: the lane's own
//            coordinate, QL = 1; host: all four, QL = 4).
#pragma once
#include <stdint.h>

// X(name, words in, words out)
#define DC_LANE_OPS(X)                                                                                      \
  X(fe_mul, 20, 10) X(fe_sq, 10, 10) X(fe_sq2x, 10, 10) X(fe_mul2, 40, 20) X(fe_mul3, 60, 30)              \
  X(fe_sq2, 20, 20) X(fe_mul_l, 20, 10) X(fe_sq_l, 10, 10) X(fe_sq2x_l, 10, 10) X(fe_sqn, 11, 10)          \
  X(fe_invert, 10, 10) X(fe_pow22523, 10, 10) X(fe_carry, 10, 10) X(fe_carry_even, 10, 10)                 \
  X(fe_sub, 20, 10) X(fe_sub4, 20, 10) X(fe_neg, 10, 10) X(fe_frombytes_w, 8, 10) X(fe_tobytes_w, 10, 8)   \
  X(fe_iszero, 10, 1) X(fe_isnegative, 10, 1) X(sc_reduce64, 16, 8) X(sc_muladd, 24, 8)                    \
  X(sc_mul_small, 13, 8) X(half_scalars, 8, 12) X(lattice_one, 33, 21)
#define DC_QUAD_OPS(X) X(q_dbl, 40, 40) X(q_to_cached, 40, 40) X(q_add, 81, 40) X(q_sum_is_identity, 80, 4)

namespace pv {

PV_HD void dc_ld(fe& f, const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 10; ++i) f.v[i] = p[i];
}
PV_HD void dc_st(uint32_t* p, const fe& f) {
#pragma unroll
  for (int i = 0; i < 10; ++i) p[i] = f.v[i];
}

// ------------------------------------------------------------------ field
PV_HD void dc_op_fe_mul(const uint32_t* in, uint32_t* out) {
  fe f, g, h;
  dc_ld(f, in); dc_ld(g, in + 10);
  fe_mul(h, f, g);
  dc_st(out, h);
}
PV_HD void dc_op_fe_mul_l(const uint32_t* in, uint32_t* out) {
  fe f, g, h;
  dc_ld(f, in); dc_ld(g, in + 10);
  fe_mul_l(h, f, g);
  dc_st(out, h);
}
PV_HD void dc_op_fe_sq(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_sq(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_sq_l(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_sq_l(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_sq2x(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_sq2x(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_sq2x_l(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_sq2x_l(h, f);
  dc_st(out, h);
}
// (f0, g0, f1, g1) -> (f0 g0, f1 g1)
PV_HD void dc_op_fe_mul2(const uint32_t* in, uint32_t* out) {
  fe f0, g0, f1, g1, h0, h1;
  dc_ld(f0, in); dc_ld(g0, in + 10); dc_ld(f1, in + 20); dc_ld(g1, in + 30);
  fe_mul2(h0, f0, g0, h1, f1, g1);
  dc_st(out, h0); dc_st(out + 10, h1);
}
PV_HD void dc_op_fe_mul3(const uint32_t* in, uint32_t* out) {
  fe f0, g0, f1, g1, f2, g2, h0, h1, h2;
  dc_ld(f0, in); dc_ld(g0, in + 10); dc_ld(f1, in + 20); dc_ld(g1, in + 30); dc_ld(f2, in + 40); dc_ld(g2, in + 50);
  fe_mul3(h0, f0, g0, h1, f1, g1, h2, f2, g2);
  dc_st(out, h0); dc_st(out + 10, h1); dc_st(out + 20, h2);
}
PV_HD void dc_op_fe_sq2(const uint32_t* in, uint32_t* out) {
  fe f0, f1, h0, h1;
  dc_ld(f0, in); dc_ld(f1, in + 10);
  fe_sq2(h0, f0, h1, f1);
  dc_st(out, h0); dc_st(out + 10, h1);
}
// in[10] = the number of squarings (1 .. 64)
PV_HD void dc_op_fe_sqn(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  int n = (int)in[10];
  n = n < 1 ? 1 : (n > 64 ? 64 : n);
  fe_sqn(h, f, n);
  dc_st(out, h);
}
PV_HD void dc_op_fe_invert(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_invert(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_pow22523(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_pow22523(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_carry(const uint32_t* in, uint32_t* out) {
  fe f;
  dc_ld(f, in);
  fe_carry(f);
  dc_st(out, f);
}
PV_HD void dc_op_fe_carry_even(const uint32_t* in, uint32_t* out) {
  fe f;
  dc_ld(f, in);
  fe_carry_even(f);
  dc_st(out, f);
}
PV_HD void dc_op_fe_sub(const uint32_t* in, uint32_t* out) {
  fe f, g, h;
  dc_ld(f, in); dc_ld(g, in + 10);
  fe_sub(h, f, g);
  dc_st(out, h);
}
PV_HD void dc_op_fe_sub4(const uint32_t* in, uint32_t* out) {
  fe f, g, h;
  dc_ld(f, in); dc_ld(g, in + 10);
  fe_sub4(h, f, g);
  dc_st(out, h);
}
PV_HD void dc_op_fe_neg(const uint32_t* in, uint32_t* out) {
  fe f, h;
  dc_ld(f, in);
  fe_neg(h, f);
  dc_st(out, h);
}
PV_HD void dc_op_fe_frombytes_w(const uint32_t* in, uint32_t* out) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = in[i];
  fe h;
  fe_frombytes_w(h, w);
  dc_st(out, h);
}
PV_HD void dc_op_fe_tobytes_w(const uint32_t* in, uint32_t* out) {
  fe f;
  dc_ld(f, in);
  uint32_t w[8];
  fe_tobytes_w(w, f);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = w[i];
}
PV_HD void dc_op_fe_iszero(const uint32_t* in, uint32_t* out) {
  fe f;
  dc_ld(f, in);
  out[0] = fe_iszero(f) ? 1u : 0u;
}
PV_HD void dc_op_fe_isnegative(const uint32_t* in, uint32_t* out) {
  fe f;
  dc_ld(f, in);
  out[0] = fe_isnegative(f);
}

// ------------------------------------------------------- scalars, lattice
PV_HD void dc_op_sc_reduce64(const uint32_t* in, uint32_t* out) {
  uint32_t x[16], r[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[i];
  sc_reduce64(r, x);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = r[i];
}
// (a, b, c) -> a b + c mod L
PV_HD void dc_op_sc_muladd(const uint32_t* in, uint32_t* out) {
  uint32_t a[8], b[8], c[8], r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = in[i];
    b[i] = in[8 + i];
    c[i] = in[16 + i];
  }
  sc_muladd(r, a, b, c);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = r[i];
}
// (d: HS_WORDS words, S: 8 words) -> d S mod L
PV_HD void dc_op_sc_mul_small(const uint32_t* in, uint32_t* out) {
  uint32_t d[HS_WORDS], S[8], r[8];
#pragma unroll
  for (int i = 0; i < HS_WORDS; ++i) d[i] = in[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) S[i] = in[HS_WORDS + i];
  sc_mul_small(r, d, S);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = r[i];
}
// h (8 words) -> status, |c| (5 words), d (5 words), c_neg; c = d = 0 unless HS_HALF
PV_HD void dc_op_half_scalars(const uint32_t* in, uint32_t* out) {
  uint32_t h[8], c[HS_WORDS], d[HS_WORDS];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] = in[i];
#pragma unroll
  for (int i = 0; i < HS_WORDS; ++i) c[i] = d[i] = 0;
  bool neg = false;
  const uint32_t st = half_scalars(c, d, neg, h);
  out[0] = st;
#pragma unroll
  for (int i = 0; i < HS_WORDS; ++i) {
    out[1 + i] = st == HS_HALF ? c[i] : 0u;
    out[1 + HS_WORDS + i] = st == HS_HALF ? d[i] : 0u;
  }
  out[11] = (st == HS_HALF && neg) ? 1u : 0u;
}
// (digest: 16 words, signature: 64 bytes as 16 words, force_full) -> record
// (HREC_WORDS words; the words lattice_one leaves unwritten are 0), status
PV_HD void dc_op_lattice_one(const uint32_t* in, uint32_t* out) {
  uint32_t rec[HREC_WORDS];
#pragma unroll
  for (int i = 0; i < HREC_WORDS; ++i) rec[i] = 0;
  const uint32_t st = lattice_one(rec, true, in, reinterpret_cast<const uint8_t*>(in + 16), in[32] != 0);
#pragma unroll
  for (int i = 0; i < HREC_WORDS; ++i) out[i] = rec[i];
  out[HREC_WORDS] = st;
}

// ------------------------------------------------------------- lane quads
PV_HD void dc_qld(qfe& P, const uint32_t* in, const QRole& q) {
#pragma unroll
  for (int j = 0; j < QL; ++j) dc_ld(P.l[j], in + 10 * qrole(j, q).l);
}
PV_HD void dc_qst(uint32_t* out, const qfe& P, const QRole& q) {
#pragma unroll
  for (int j = 0; j < QL; ++j) dc_st(out + 10 * qrole(j, q).l, P.l[j]);
}
PV_HD void dc_qop_q_dbl(const uint32_t* in, uint32_t* out, const QRole& q) {
  qfe P;
  dc_qld(P, in, q);
  q_dbl(P, q);
  dc_qst(out, P, q);
}
PV_HD void dc_qop_q_to_cached(const uint32_t* in, uint32_t* out, const QRole& q) {
  qfe P, e;
  dc_qld(P, in, q);
  q_to_cached(e, P, q);
  dc_qst(out, e, q);
}
// (P, e in add order with lanes 0 / 1 already swapped when neg, neg) -> P +- E
PV_HD void dc_qop_q_add(const uint32_t* in, uint32_t* out, const QRole& q) {
  qfe P, e;
  dc_qld(P, in, q);
  dc_qld(e, in + 40, q);
  q_add(P, e, in[80] != 0, q);
  dc_qst(out, P, q);
}
// (Q0, e1 in add order) -> [Q0 + E1 == O] on every lane of the quad
PV_HD void dc_qop_q_sum_is_identity(const uint32_t* in, uint32_t* out, const QRole& q) {
  qfe P, e;
  dc_qld(P, in, q);
  dc_qld(e, in + 40, q);
  const uint32_t id = q_sum_is_identity(P, e, q) ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < QL; ++j) out[qrole(j, q).l] = id;
}

}  // namespace pv
