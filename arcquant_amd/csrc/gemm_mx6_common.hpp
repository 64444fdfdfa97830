// What the MXFP6 GEMM units share (gemm_mx6.hip: the reference-layout weight; gemm_mx6_rw.hip: the repacked weight): the e3m2 operand
// fragment of the scaled MFMA, its split into large and small codes, and the pointer types of a 24-byte block.  One text, so that a
// fragment cannot depend on which layout the weight came in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_common.hpp"
#include "quantize_mx6_device.hpp"

namespace arcq {

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef i32x4 i32x4_a8 __attribute__((aligned(8)));      // a 16-byte load from an address that is only 8-byte aligned
typedef i32x2 i32x2_a8 __attribute__((aligned(8)));

constexpr int kMx6Fmt = 3;                                // cbsz / blgp of e3m2 (4: e2m1)
constexpr int kMx6StepBytes = 96;                         // 128 e3m2 codes

__device__ __forceinline__ i32x8 frag6(uint2 a, uint2 b, uint2 c) {
  i32x8 f = {(int)a.x, (int)a.y, (int)b.x, (int)b.y, (int)c.x, (int)c.y, 0, 0};     // e3m2: the instruction reads the first six dwords only
  return f;
}
__device__ __forceinline__ i32x8 frag6(i32x4 lo, i32x2 hi) {
  i32x8 f = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, 0, 0};
  return f;
}
// an e3m2 fragment as two: the codes of magnitude >= 2 and the others (quantize_mx6_device.hpp mx6_split_fragment)
__device__ __forceinline__ void split6(const i32x8& f, i32x8& hi, i32x8& lo) {
  const uint32_t w[6] = {(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[3], (uint32_t)f[4], (uint32_t)f[5]};
  uint32_t h[6], l[6];
  mx6_split_fragment(w, h, l);
  hi = i32x8{(int)h[0], (int)h[1], (int)h[2], (int)h[3], (int)h[4], (int)h[5], 0, 0};
  lo = i32x8{(int)l[0], (int)l[1], (int)l[2], (int)l[3], (int)l[4], (int)l[5], 0, 0};
}

}  // namespace arcq
