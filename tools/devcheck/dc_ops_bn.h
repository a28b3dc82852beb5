// One case of each BN254 Fp / Fp2 primitive, limbs in and limbs out (10 signed
// 28-bit limbs as words): the body shared by the device check (devcheck.hip,
// where bn::mul / bn::sqr are the generated asm chains of pv_bn254_asm.h) and
// its host twins (tools/hostcheck/bn254check.cpp, the C++ column sums with the
// column-bound check).  See dc_ops_pv.h.
#pragma once
#include <stdint.h>

// X(name, words in, words out)
#define DC_BN_OPS(X)                                                                                     \
  X(bn_mul, 20, 10) X(bn_sqr, 10, 10) X(bn_norm, 10, 10) X(bn_reduce, 10, 10) X(bn_canon, 10, 10)       \
  X(bn_add_mul, 30, 10) X(bn_sub_mul, 30, 10) X(bn_f2mul, 40, 20) X(bn_f2sqr, 20, 20)

namespace bn {

PV_HD fp dc_ld(const uint32_t* p) {
  fp r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (int32_t)p[i];
  return r;
}
PV_HD void dc_st(uint32_t* p, const fp& a) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = (uint32_t)a.l[i];
}

PV_HD void dc_op_bn_mul(const uint32_t* in, uint32_t* out) { dc_st(out, mul(dc_ld(in), dc_ld(in + 10))); }
PV_HD void dc_op_bn_sqr(const uint32_t* in, uint32_t* out) { dc_st(out, sqr(dc_ld(in))); }
PV_HD void dc_op_bn_norm(const uint32_t* in, uint32_t* out) { dc_st(out, norm(dc_ld(in))); }
PV_HD void dc_op_bn_reduce(const uint32_t* in, uint32_t* out) { dc_st(out, reduce(dc_ld(in))); }
PV_HD void dc_op_bn_canon(const uint32_t* in, uint32_t* out) { dc_st(out, canon(dc_ld(in))); }
// (a, b, c) -> (a + b) c and (a - b) c: a lazy sum straight into a multiply
PV_HD void dc_op_bn_add_mul(const uint32_t* in, uint32_t* out) {
  dc_st(out, mul(add(dc_ld(in), dc_ld(in + 10)), dc_ld(in + 20)));
}
PV_HD void dc_op_bn_sub_mul(const uint32_t* in, uint32_t* out) {
  dc_st(out, mul(sub(dc_ld(in), dc_ld(in + 10)), dc_ld(in + 20)));
}
// (x.a, x.b, y.a, y.b) -> x y
PV_HD void dc_op_bn_f2mul(const uint32_t* in, uint32_t* out) {
  const fp2 r = f2mul(fp2{dc_ld(in), dc_ld(in + 10)}, fp2{dc_ld(in + 20), dc_ld(in + 30)});
  dc_st(out, r.a);
  dc_st(out + 10, r.b);
}
PV_HD void dc_op_bn_f2sqr(const uint32_t* in, uint32_t* out) {
  const fp2 r = f2sqr(fp2{dc_ld(in), dc_ld(in + 10)});
  dc_st(out, r.a);
  dc_st(out + 10, r.b);
}

}  // namespace bn
