// Row sources of the fused quantisers, shared by quantize.hip (NVFP4) and quantize_mx.hip (MXFP4): the RMSNorm row (sum of squares in
// the reference's association order, rstd) and act = silu(gate) * up computed on the fly.  ONE statement of each, so that the two quant
// types normalise and activate identically, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "quantize_device.hpp"

namespace arcq {

__device__ __forceinline__ uint4 silu_mul_chunk(const uint4 g, const uint4 u) {
  const uint32_t gw[4] = {g.x, g.y, g.z, g.w}, uw[4] = {u.x, u.y, u.z, u.w};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = silu_mul_bf16(gw[j] & 0xffffu, uw[j] & 0xffffu) | (silu_mul_bf16(gw[j] >> 16, uw[j] >> 16) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}
// eight activations from sixteen interleaved values (g0, u0, g1, u1, ...): every dword is one (gate, up) pair
__device__ __forceinline__ uint4 silu_mul_pairs(const uint4 lo, const uint4 hi) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = silu_mul_bf16(w[2 * j] & 0xffffu, w[2 * j] >> 16) | (silu_mul_bf16(w[2 * j + 1] & 0xffffu, w[2 * j + 1] >> 16) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}
// chunk c (8 activations) of a row: kSiluHalves: gate at g[8c..], up at u[8c..]; kSiluPairs: pairs at g[16c..]
enum : int { kSiluNone = 0, kSiluHalves = 1, kSiluPairs = 2 };
template <int kSilu>
__device__ __forceinline__ uint4 silu_act_chunk(const uint16_t* g, const uint16_t* u, int64_t c) {
  if (kSilu == kSiluPairs)
    return silu_mul_pairs(*reinterpret_cast<const uint4*>(g + c * 16), *reinterpret_cast<const uint4*>(g + c * 16 + 8));
  return silu_mul_chunk(*reinterpret_cast<const uint4*>(g + c * 8), *reinterpret_cast<const uint4*>(u + c * 8));
}
template <int kSilu>
__device__ __forceinline__ uint32_t silu_act_elem(const uint16_t* g, const uint16_t* u, uint32_t i) {
  if (kSilu == kSiluPairs) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(g + 2 * i);
    return silu_mul_bf16(w & 0xffffu, w >> 16);
  }
  return silu_mul_bf16(g[i], u[i]);
}

// Stages one row (KQ = 16 bdx elements, bdx <= 512) in the padded LDS layout and returns in part[k] the partial sum of squares of
// virtual thread v = tid + 256 k of the reference's block (rmsnorm.cu:113-128): its 16-byte chunks v and bdx + v, the 16 squares
// accumulated sequentially.  256 threads.
__device__ __forceinline__ void rms_stage_row(uint16_t* row_lds, const uint16_t* xrow, int bdx, float (&part)[2]) {
  const int tid = threadIdx.x;
  part[0] = part[1] = 0.0f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {                              // bdx <= 512: virtual threads tid and tid + 256
    const int v = tid + k * 256;
    if (v < bdx) {
      float acc = 0.0f;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int c = it * bdx + v;
        uint4 d = *reinterpret_cast<const uint4*>(xrow + (size_t)c * 8);
        lds_put_chunk(row_lds, c, d);
        const uint32_t w4[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float a = bf16_bits_to_f32(w4[j] & 0xffffu), b = bf16_bits_to_f32(w4[j] >> 16);
          acc = acc + a * a;
          acc = acc + b * b;
        }
      }
      part[k] = acc;
    }
  }
}

// The strides 128 .. 1 of the reduction tree below, by ONE whole wave: lane `tid` (0 .. 63) passes the stride-256 sums of columns tid, tid + 64, tid + 128 and
// tid + 192; lane 0 returns the row's sum of squares (other lanes: not the sum).
__device__ __forceinline__ float rms_tree_wave(float x0, float x1, float x2, float x3, int bdx, const int tid) {
  const float y0 = (tid + 128 < bdx) ? x0 + x2 : x0;                 // stride 128: columns tid and tid + 64
  const float y1 = (tid + 192 < bdx) ? x1 + x3 : x1;
  float z = (tid + 64 < bdx) ? y0 + y1 : y0;                         // stride 64
  const float up = __shfl_down(z, 32, 64);
  if (tid < 32 && tid + 32 < bdx) z = z + up;                        // stride 32
  float val = tid < 32 ? z : 0.0f;
  val += __shfl_down(val, 16, 64);                                       // lane 0's cone = reference's
  val += dpp_row_shl<8>(val);                                            // strides 8 .. 1 stay inside lane 0's row of 16 (DPP)
  val += dpp_row_shl<4>(val);
  val += dpp_row_shl<2>(val);
  val += dpp_row_shl<1>(val);
  return val;
}
// rstd of a row from its sum of squares
__device__ __forceinline__ float rms_rstd_of(float sumsq, int KQ, float eps) {
  const float var = sumsq / (float)KQ + eps;                             // rmsnorm.cu:157
  return (float)(1.0 / sqrt((double)var));                               // oracle assumption A4
}

// Sum of squares of one row in the reference's association order (rmsnorm.cu:113-154), so that the
// fp32 result is bit-identical to the oracle's: virtual thread v in [0, bdx = KQ/16) owns the 16-byte
// chunks v and bdx + v and accumulates their 16 squares sequentially (the caller passes the partial sums of
// v = tid and v = tid + 256); then the fixed tree s[v] += s[v + stride], stride = 256 ... 32, and a 32-lane shuffle.
// The same tree with TWO barriers instead of seven: the stride-256 step adds two values this thread computed itself;
// strides 128 and 64 only ever feed s[0..63], so wave 0 evaluates them for its 64 columns from four LDS reads;
// stride 32 and below are shuffles.  `s` is an LDS array of >= 512 floats.  Returns rstd = 1 / sqrt(total / KQ + eps) in every
// thread: thread 0 forms it (the correctly rounded double-precision evaluation is ~35 half-rate instructions -- done by all 256
// threads of all resident workgroups it was ~2 us of the 18.5 us launch at 4096 x 4096) and publishes it with the second barrier.
__device__ __forceinline__ float rms_rstd_tree(float* s, int bdx, float p_lo, float p_hi, int KQ, float eps) {
  const int tid = threadIdx.x;
  const float s256 = (tid + 256 < bdx) ? p_lo + p_hi : p_lo;           // stride 256
  if (tid < bdx) s[tid] = s256;
  __syncthreads();                                                     // (also publishes the staged row)
  if (tid < 64) {
    const float val = rms_tree_wave(s[tid], s[tid + 64], s[tid + 128], s[tid + 192], bdx, tid);
    if (tid == 0) s[256] = rms_rstd_of(val, KQ, eps);
  }
  __syncthreads();
  return s[256];
}
// The same row, the same sums, by ONE wave and without a barrier (the prologue of gemm_mx_linear_rw.hip, where every wave of the workgroup
// has a row of its own): lane l plays the virtual threads l, l + 64, ... (<= 8 of them), so the strides 256, 128 and 64 add values the
// lane holds itself.  Stages the row in the padded LDS layout as rms_stage_row does and returns rstd in every lane.
__device__ __forceinline__ float rms_stage_row_wave(uint16_t* row_lds, const uint16_t* xrow, int bdx, int KQ, float eps, const int lane) {
  float p[8];
#pragma unroll
  for (int half = 0; half < 2; ++half) {                       // two batches of eight chunk loads (32 VGPRs) in flight; KQ <= 4096 needs one
    uint4 d[4][2];
    if (256 * half < bdx) {                                    // (uniform)
#pragma unroll
      for (int k = 0; k < 4; ++k)                                // clamped, so that the loads leave together (a clamped chunk is not used);
#pragma unroll
        for (int it = 0; it < 2; ++it)                           // 32-bit offsets from the wave's uniform row pointer
          d[k][it] = *reinterpret_cast<const uint4*>(xrow + (uint32_t)min(it * bdx + lane + 64 * (4 * half + k), 2 * bdx - 1) * 8u);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = lane + 64 * (4 * half + k);
      float acc = 0.0f;
      if (v < bdx) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          lds_put_chunk(row_lds, it * bdx + v, d[k][it]);
          const uint32_t w4[4] = {d[k][it].x, d[k][it].y, d[k][it].z, d[k][it].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float a = bf16_bits_to_f32(w4[j] & 0xffffu), b = bf16_bits_to_f32(w4[j] >> 16);
            acc = acc + a * a;
            acc = acc + b * b;
          }
        }
      }
      p[4 * half + k] = acc;
    }
  }
  float s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = (lane + 64 * k + 256 < bdx) ? p[k] + p[k + 4] : p[k];      // stride 256
  const float val = rms_tree_wave(s[0], s[1], s[2], s[3], bdx, lane);
  float rstd = 0.0f;
  if (lane == 0) rstd = rms_rstd_of(val, KQ, eps);                        // (one lane: the double-precision evaluation is ~35 half-rate instructions)
  return __shfl(rstd, 0, 64);
}

}  // namespace arcq
