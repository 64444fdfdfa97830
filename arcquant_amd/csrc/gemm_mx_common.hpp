// What the MXFP4 GEMM units share (gemm_mx.hip: the reference-layout weight; gemm_mx_rw.hip, gemm_mx_tile_rw.hip and gemm_mx_slice_rw.hip: the
// repacked weight; the tiled and the quantising kernels share more: gemm_mx_tile_common.hpp): the parameter
// block, the operand fragment of the block-scaled fp4 MFMA and the epilogues.  One text, so that a result cannot depend on which
// layout the weight came in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"

namespace arcq {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct MxArgs {
  const uint8_t* A;
  const uint8_t* B;       // the units over the repacked weight: MRW (arcq.h "MXFP4 repacked weight")
  const uint8_t* SFA;
  const uint8_t* SFB;     // the units over the repacked weight: MRSF
  void* D;
  int M, N, Kp;
  float alpha_host;
  const float* alpha_dev;
  const uint16_t* bias;
  const uint16_t* residual;
  int out_dtype;
  uint8_t* QACT;      // kEpiSiluMulQuant: codes [M, Kp2/2] and scale bytes [M, Kp2/32] of the quantised activation, KQ2 = N/2, K2 = KQ2 + KE
  uint8_t* SFACT;
  int KE;
};
constexpr int kEpiSiluMulQuant = 2;

__device__ __forceinline__ i32x8 frag(uint4 u) {
  i32x8 f = {(int)u.x, (int)u.y, (int)u.z, (int)u.w, 0, 0, 0, 0};     // fp4: the instruction reads the first four dwords only
  return f;
}
__device__ __forceinline__ i32x8 frag(i32x4 u) {
  i32x8 f = {u.x, u.y, u.z, u.w, 0, 0, 0, 0};
  return f;
}

// alpha * acc (+ bias) (+ residual) -> D[m, n] with arcq_gemm_nvfp4's roundings (gemm_common.hpp finish4)
__device__ __forceinline__ void mx_store(const MxArgs& p, float alpha, int m, int n, float acc) {
  const size_t o = (size_t)m * (size_t)p.N + (size_t)n;
  float d = alpha * acc;
  const bool f32 = p.out_dtype == ARCQ_OUT_F32;
  if (p.bias) d = (f32 ? d : bf16_bits_to_f32(f32_to_bf16_bits(d))) + bf16_bits_to_f32(p.bias[n]);
  if (p.residual) d = (f32 ? d : bf16_bits_to_f32(f32_to_bf16_bits(d))) + bf16_bits_to_f32(p.residual[o]);
  if (f32) reinterpret_cast<float*>(p.D)[o] = d;
  else reinterpret_cast<uint16_t*>(p.D)[o] = (uint16_t)f32_to_bf16_bits(d);
}

// bf16 bits of the value mx_store writes for a bf16 output without residual: bf16(alpha * acc), then + bias -> bf16
__device__ __forceinline__ uint32_t mx_y_bits(float alpha, float acc, bool has_bias, float bias) {
  const uint32_t y = f32_to_bf16_bits(alpha * acc);
  return has_bias ? f32_to_bf16_bits(bf16_bits_to_f32(y) + bias) : y;
}

// lane <- the lane of its DPP quad at position kPerm[lane & 3] (quad_perm; every lane of the quad must be active)
template <int kCtrl>
__device__ __forceinline__ uint32_t dpp_quad(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xf, 0xf, true);
}
constexpr int kQuadSwap1 = 0xB1;   // quad_perm:[1,0,3,2]: the gate / up partner
constexpr int kQuadSwap2 = 0x4E;   // quad_perm:[2,3,0,1]: the neighbouring pair

// SiLU*up of TWO output rows r0, r1 held by a (gate, up) lane pair: y0 / y1 = this lane's bf16 outputs (its own column) in those rows.
// The even lane (gate column) computes row r0 and the odd lane (up column) row r1 -- one activation per lane, none computed twice:
// each sends the value the other needs in ONE exchange.  A second exchange brings in the activation of the next column pair, so that
// lanes 0 and 1 of a quad each hold two adjacent activations of their row: returns them packed (valid where (lane & 2) == 0, for
// row r0 in even lanes and r1 in odd lanes, columns n/2 and n/2 + 1 of lane 0's n).
__device__ __forceinline__ uint32_t mx_silu_pair(uint32_t y0, uint32_t y1, bool odd) {
  const uint32_t got = dpp_quad<kQuadSwap1>(odd ? y0 : y1);
  const uint32_t act = silu_mul_bf16(odd ? got : y0, odd ? y1 : got);
  return act | (dpp_quad<kQuadSwap2>(act) << 16);
}

// The K split of every M <= kMxSmallM kernel, and with it the order of every sum: wave w takes the K steps s = w (mod kMxSmallWaves) in
// ascending order, the partial sums are added w = 0 .. kMxSmallWaves - 1
constexpr int kMxSmallM = 64;
constexpr int kMxSmallWaves = 8;

}  // namespace arcq
