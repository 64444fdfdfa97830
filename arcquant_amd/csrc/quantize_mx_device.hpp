// The MXFP4 block rule (include/arcq.h "MXFP4"), stated once for every kernel that emits blocks: the row quantisers of quantize_mx.hip
// and the quantising epilogues of gemm_mx.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"

namespace arcq {

// Smallest e with amax <= 6 * 2^e, clamped to [-127, 127]; 0 for amax == 0.  Exact, from the fp32 bits of amax (a widened
// bf16): amax = m * 2^E with m in [1, 2) -> 6 * 2^e = 1.5 * 2^(e+2) >= m * 2^E  <=>  e >= E - 2 when m <= 1.5, else E - 1.
// Subnormal amax (< 2^-126) always lands on the clamp.
__device__ __forceinline__ int mx_block_exponent(float amax) {
  const uint32_t u = __float_as_uint(amax);
  const int ef = (int)(u >> 23);
  if (u == 0) return 0;
  if (ef == 0) return -127;
  const int E = ef - 127;
  const int e = (u & 0x7fffffu) <= 0x400000u ? E - 2 : E - 1;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

struct MxBlock {
  uint4 packed;   // 32 codes
  uint32_t s8;    // E8M0 byte = e + 127
};

// 32 values -> codes.  v * 2^-e is exact (ldexp) and |v * 2^-e| <= 6, so the saturating RNE conversion of
// quantize_device.hpp never saturates.  kResid: v[] is overwritten with the residual v - deq(code) * 2^e, exact in bf16.
template <bool kResid>
__device__ __forceinline__ MxBlock mx_quantize_block(float (&v)[32]) {
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
  const int e = mx_block_exponent(amax);
  uint32_t w[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t x = 0;
    x = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(x, __builtin_ldexpf(v[8 * d + 0], -e), __builtin_ldexpf(v[8 * d + 1], -e), 1.0f, 0);
    x = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(x, __builtin_ldexpf(v[8 * d + 2], -e), __builtin_ldexpf(v[8 * d + 3], -e), 1.0f, 1);
    x = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(x, __builtin_ldexpf(v[8 * d + 4], -e), __builtin_ldexpf(v[8 * d + 5], -e), 1.0f, 2);
    x = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(x, __builtin_ldexpf(v[8 * d + 6], -e), __builtin_ldexpf(v[8 * d + 7], -e), 1.0f, 3);
    w[d] = x;
  }
  if (kResid) {
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float q = e2m1_to_f32((w[i >> 3] >> (4 * (i & 7))) & 0xfu);
      // exact: a multiple of ulp_bf16(v) with |res| <= |v|.  Formed at half scale: deq(code) * 2^e itself is 2^128 for code 4.0 at
      // e = 126 (amax >= 1.75 * 2^127 rounds up to it), +inf in fp32.  Halving a widened bf16 and doubling the result are exact.
      v[i] = 2.0f * (0.5f * v[i] - __builtin_ldexpf(q, e - 1));
    }
  }
  MxBlock b;
  b.packed = make_uint4(w[0], w[1], w[2], w[3]);
  b.s8 = (uint32_t)(e + 127);
  return b;
}

// One block of an activation row: codes + scale byte at block b; in the outlier tail also the quantised residual at block br.
__device__ __forceinline__ void mx_store_x_block(uint8_t* qrow, uint8_t* srow, int b, int br, bool tail, float (&v)[32]) {
  if (!tail) {
    const MxBlock q = mx_quantize_block<false>(v);
    *reinterpret_cast<uint4*>(qrow + (size_t)b * 16) = q.packed;
    srow[b] = (uint8_t)q.s8;
  } else {
    const MxBlock q = mx_quantize_block<true>(v);
    *reinterpret_cast<uint4*>(qrow + (size_t)b * 16) = q.packed;
    srow[b] = (uint8_t)q.s8;
    const MxBlock r = mx_quantize_block<false>(v);
    *reinterpret_cast<uint4*>(qrow + (size_t)br * 16) = r.packed;
    srow[br] = (uint8_t)r.s8;
  }
}

// The padding blocks [K/32, Bp) of a row (K = KQ + KE, Bp = round_up(K, 128) / 32: at most two): code 0, scale 2^0; thread t writes block K/32 + t.
__device__ __forceinline__ void mx_store_padding(uint8_t* qrow, uint8_t* srow, int K, int Bp, int t) {
  const int pb = (K >> 5) + t;
  if (pb < Bp) {
    *reinterpret_cast<uint4*>(qrow + (size_t)pb * 16) = make_uint4(0, 0, 0, 0);
    srow[pb] = 127;
  }
}

}  // namespace arcq
