// DEVICE CHECK of the arithmetic primitives (test tooling only -- never linked
// into or loaded by the product, see tests/test_gpu_devcheck.py).
//
// For nearly every primitive the GPU compiles other code than the host build
// that tools/hostcheck checks against Python integers: the v_mad_u64_u32 asm
// chains of pv_field.h / pv_madchains.h / pv_bn254_asm.h, the two-chain
// __builtin_addc / subc forms and the v_rcp_f64 quotient estimate of
// pv_lattice.h, the DPP quad_perm moves of pv_quad.h.  This translation unit
// includes the product headers unchanged, is compiled with the product's flags
// (indy-plenum_amd/build.py build_devcheck), and runs each primitive on chosen
// operands, one case per lane (one point per lane quad for pv_quad.h), storing
// the raw result words.  The op bodies are dc_ops_pv.h / dc_ops_bn.h, shared
// with the host twins so that both sides run the same calls.
//
// Every op `name` of the lists there has one kernel k_<name> and one wrapper
//   int dc_<name>(const uint32_t* in, uint64_t n, uint32_t* out)
// over n cases (n quads for the quad ops) of IW words in and OW words out each,
// packed case after case.  The wrapper allocates, copies, launches, waits,
// copies back and frees on device 0 and returns the first non-zero HIP status
// (0 = ok); after an error nothing more is launched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../indy-plenum_amd/csrc/pv_verify_core.h"
#include "../../indy-plenum_amd/csrc/pv_quad.h"
#include "../../indy-plenum_amd/csrc/pv_bn254.h"
#include "dc_ops_pv.h"
#include "dc_ops_bn.h"

namespace {

constexpr int DC_BLOCK = 64;   // one wave per block; 16 whole quads

typedef void (*dc_kernel)(const uint32_t*, uint64_t, uint32_t*);

// n cases of iw words in / ow words out through kernel k with `lanes` lanes per case
int dc_run(dc_kernel k, const uint32_t* in, uint64_t n, int iw, int ow, uint32_t* out, int lanes) {
  if (n == 0) return 0;
  if (n > (1u << 24)) return (int)hipErrorInvalidValue;
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t ib = (size_t)n * iw * sizeof(uint32_t), ob = (size_t)n * ow * sizeof(uint32_t);
  e = hipMalloc(&din, ib);
  if (e == hipSuccess) e = hipMalloc(&dout, ob);
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(dout, 0xa5, ob);   // a word no lane wrote shows
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((n * lanes + DC_BLOCK - 1) / DC_BLOCK);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(DC_BLOCK), 0, 0, din, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  // frees only (no launch) after an error; their status does not mask the first one
  const hipError_t f0 = din ? hipFree(din) : hipSuccess;
  const hipError_t f1 = dout ? hipFree(dout) : hipSuccess;
  if (e != hipSuccess) return (int)e;
  if (f0 != hipSuccess) return (int)f0;
  return (int)f1;
}

}  // namespace

// lane i runs case i
#define DC_LANE_KERNEL(NS, name, IW, OW)                                                                  \
  __global__ void __launch_bounds__(64) k_##name(const uint32_t* in, uint64_t n, uint32_t* out) {        \
    const uint64_t i = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;                                    \
    if (i >= n) return;                                                                                  \
    NS::dc_op_##name(in + i * IW, out + i * OW);                                                         \
  }                                                                                                      \
  extern "C" int dc_##name(const uint32_t* in, uint64_t n, uint32_t* out) {                              \
    return dc_run(k_##name, in, n, IW, OW, out, 1);                                                      \
  }
#define DC_PV_KERNEL(name, IW, OW) DC_LANE_KERNEL(pv, name, IW, OW)
#define DC_BN_KERNEL(name, IW, OW) DC_LANE_KERNEL(bn, name, IW, OW)

// lanes 4 i .. 4 i + 3 run quad i: a quad is in range or out as a whole, so
// every lane a quad_perm move reads is active
#define DC_QUAD_KERNEL(name, IW, OW)                                                                      \
  __global__ void __launch_bounds__(64) k_##name(const uint32_t* in, uint64_t n, uint32_t* out) {        \
    const uint64_t t = (uint64_t)blockIdx.x * DC_BLOCK + threadIdx.x;                                    \
    const uint64_t i = t >> 2;                                                                           \
    if (i >= n) return;                                                                                  \
    pv::dc_qop_##name(in + i * IW, out + i * OW, pv::qrole_of((uint32_t)(t & 3)));                       \
  }                                                                                                      \
  extern "C" int dc_##name(const uint32_t* in, uint64_t n, uint32_t* out) {                              \
    return dc_run(k_##name, in, n, IW, OW, out, 4);                                                      \
  }

DC_LANE_OPS(DC_PV_KERNEL)
DC_BN_OPS(DC_BN_KERNEL)
DC_QUAD_OPS(DC_QUAD_KERNEL)
