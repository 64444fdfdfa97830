// Reorder + MXFP4 quantise kernels for gfx950 (activation with ARC residual / weight with duplicate).
//
// Format (include/arcq.h, DESIGN.md "MXFP4"): blocks of 32 elements, one E8M0 scale byte each, e2m1 codes packed two per
// byte (low nibble = even element).  Augmented K is the fake path's concatenation: positions [0, KQ) hold the reordered row,
// [KQ, K) the residual (x) or a copy (w) of reordered channels [KQ-KE, KQ), [K, Kp) padding (code 0, scale byte 127),
// Kp = round_up(K, 128) so that every K step of the scaled MFMA is full.
//
// Work decomposition: the row structure of quantize.hip -- one workgroup per row (grid-strided), the row staged in LDS with
// the padded layout of quantize_device.hpp (one pad dword per 16 elements, conflict-free gathers for any permutation),
// decode-sized inputs additionally split along the row over blockIdx.y.  Thread t owns 32-element blocks t, t + 256, ...
// of the reordered row: gather 32 values, exponent from the bits, codes, 16-byte store + 1 scale byte; blocks in the
// outlier tail also emit the residual / duplicate block at KQ/32 + (b - (KQ-KE)/32).
//
// Fused row sources (mx_fused_rows_kernel): the row that is quantised is the RMSNorm of X (arcq_mx_rmsnorm_quantize_x) or
// silu(gate) * up (arcq_mx_silu_mul_quantize_x) instead of X itself, formed by the functions of quantize_source_device.hpp that the
// NVFP4 quantisers use.  MXFP4 has no per-tensor scale, so there is no abs-max pass: each is ONE launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "quantize_device.hpp"
#include "quantize_mx_device.hpp"
#include "quantize_source_device.hpp"

namespace arcq {

constexpr int kMxThreads = 256;

template <bool kModeW>
__global__ __launch_bounds__(kMxThreads) void mx_quantize_rows_kernel(const uint16_t* __restrict__ X, const int16_t* __restrict__ idx,
                                                                      uint8_t* __restrict__ Q, uint8_t* __restrict__ SF, int rows, int KQ,
                                                                      int KE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* row_lds = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  const int K = KQ + KE;
  const int Kp = (K + 127) & ~127;
  const int B = KQ >> 5;                 // source blocks of the reordered row
  const int P = (KQ - KE) >> 5;          // first block of the outlier tail
  const int Bp = Kp >> 5;                // scale bytes per row
  const int chunks = KQ >> 3;
  // blockIdx.y owns a range of the row's blocks (every workgroup stages the whole row: the gather may touch any channel)
  const int b_per = (B + (int)gridDim.y - 1) / (int)gridDim.y;
  const int b_begin = (int)blockIdx.y * b_per;
  const int b_end = min(B, b_begin + b_per);
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const uint16_t* xrow = X + (size_t)row * KQ;
    for (int c = tid; c < chunks; c += kMxThreads) lds_put_chunk(row_lds, c, *reinterpret_cast<const uint4*>(xrow + (size_t)c * 8));
    __syncthreads();
    uint8_t* qrow = Q + (size_t)row * (Kp >> 1);
    uint8_t* srow = SF + (size_t)row * Bp;
    for (int b = b_begin + tid; b < b_end; b += kMxThreads) {
      float v[32];
#pragma unroll
      for (int h = 0; h < 2; ++h) {        // two 16-index loads per half block
        const uint4 i0 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16);
        const uint4 i1 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16 + 8);
        const uint32_t iw[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t pw = lds_pad_pair(iw[j]);
          v[16 * h + 2 * j] = bf16_bits_to_f32(row_lds[pw & 0xffffu]);
          v[16 * h + 2 * j + 1] = bf16_bits_to_f32(row_lds[pw >> 16]);
        }
      }
      const bool tail = b >= P;
      const int br = B + (b - P);          // residual / duplicate block
      if (kModeW) {
        const MxBlock q = mx_quantize_block<false>(v);
        *reinterpret_cast<uint4*>(qrow + (size_t)b * 16) = q.packed;
        srow[b] = (uint8_t)q.s8;
        if (tail) {
          *reinterpret_cast<uint4*>(qrow + (size_t)br * 16) = q.packed;
          srow[br] = (uint8_t)q.s8;
        }
      } else {
        mx_store_x_block(qrow, srow, b, br, tail, v);
      }
    }
    if (blockIdx.y == 0) mx_store_padding(qrow, srow, K, Bp, tid);     // (by the workgroup of the row's first range)
    __syncthreads();   // row_lds is rewritten by the next row
  }
}

// ------------------------------------------------------------------------------------------------------------ fused sources
// kSrc = kMxSrcRms: the row is bf16(x[i] * wn[i] * rstd), arcq_rmsnorm_quantize_x's normalised row (same sum-of-squares order, same
//        rstd, same product order); the norm weight is staged in LDS once per workgroup (scattered 2-byte global loads cost 2.6x the
//        whole kernel in quantize.hip).  Every workgroup of a split row forms the row's rstd itself (the row is an L2 hit).
// kSrc = kMxSrcSiluHalves / kMxSrcSiluPairs: the row is silu(gate) * up with torch's roundings (silu_mul_bf16).  kDirect (rows split
//        over blockIdx.y): the row is NOT staged -- each of the gridDim.y workgroups would recompute all of it, one exp per element --
//        the gather computes its own elements from global memory, each activation exactly once.
enum : int { kMxSrcRms = 0, kMxSrcSiluHalves = kSiluHalves, kMxSrcSiluPairs = kSiluPairs };

template <int kSrc, bool kDirect>
__global__ __launch_bounds__(kMxThreads) void mx_fused_rows_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Xup, int64_t ldx,
                                                                   const uint16_t* __restrict__ Wn, float eps, const int16_t* __restrict__ idx,
                                                                   uint8_t* __restrict__ Q, uint8_t* __restrict__ SF, int rows, int KQ, int KE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* row_lds = reinterpret_cast<uint16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + lds_row_bytes(KQ));                                    // kMxSrcRms: 512 floats of reduction scratch
  uint16_t* wn_lds = reinterpret_cast<uint16_t*>(smem + lds_row_bytes(KQ) + 512 * sizeof(float));   // ... and the norm weight
  constexpr bool kRms = kSrc == kMxSrcRms;
  static_assert(!(kRms && kDirect), "the RMSNorm row needs the whole row in every workgroup");
  const int tid = threadIdx.x;
  const int K = KQ + KE;
  const int Kp = (K + 127) & ~127;
  const int B = KQ >> 5, P = (KQ - KE) >> 5, Bp = Kp >> 5;
  const int chunks = KQ >> 3;
  const int b_per = (B + (int)gridDim.y - 1) / (int)gridDim.y;
  const int b_begin = (int)blockIdx.y * b_per;
  const int b_end = min(B, b_begin + b_per);
  if (kRms) {
    for (int c = tid; c < chunks; c += kMxThreads) lds_put_chunk(wn_lds, c, *reinterpret_cast<const uint4*>(Wn + (size_t)c * 8));
    // visible after the barriers of the first row's reduction
  }
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const uint16_t* xrow = X + (size_t)row * ldx;
    const uint16_t* urow = kRms ? nullptr : Xup + (size_t)row * ldx;
    float rstd = 1.0f;
    if constexpr (kRms) {
      float part[2];
      rms_stage_row(row_lds, xrow, KQ >> 4, part);
      rstd = rms_rstd_tree(red, KQ >> 4, part[0], part[1], KQ, eps);
    } else if constexpr (!kDirect) {
      for (int c = tid; c < chunks; c += kMxThreads) lds_put_chunk(row_lds, c, silu_act_chunk<kSrc>(xrow, urow, c));
      __syncthreads();
    }
    uint8_t* qrow = Q + (size_t)row * (Kp >> 1);
    uint8_t* srow = SF + (size_t)row * Bp;
    for (int b = b_begin + tid; b < b_end; b += kMxThreads) {
      float v[32];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint4 i0 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16);
        const uint4 i1 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16 + 8);
        const uint32_t iw[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float a, c;
          if constexpr (kDirect) {
            a = bf16_bits_to_f32(silu_act_elem<kSrc>(xrow, urow, iw[j] & 0xffffu));
            c = bf16_bits_to_f32(silu_act_elem<kSrc>(xrow, urow, iw[j] >> 16));
          } else {
            const uint32_t pw = lds_pad_pair(iw[j]), pa = pw & 0xffffu, pb = pw >> 16;
            a = bf16_bits_to_f32(row_lds[pa]);
            c = bf16_bits_to_f32(row_lds[pb]);
            if (kRms) {                                   // rmsnorm.cu:165-171: (x * w) * rstd in fp32, then bf16
              a = round_to_bf16(a * bf16_bits_to_f32(wn_lds[pa]) * rstd);
              c = round_to_bf16(c * bf16_bits_to_f32(wn_lds[pb]) * rstd);
            }
          }
          v[16 * h + 2 * j] = a;
          v[16 * h + 2 * j + 1] = c;
        }
      }
      mx_store_x_block(qrow, srow, b, B + (b - P), b >= P, v);
    }
    if (blockIdx.y == 0) mx_store_padding(qrow, srow, K, Bp, tid);     // (by the workgroup of the row's first range)
    if (!kDirect) __syncthreads();   // row_lds (and the reduction scratch) are rewritten by the next row
  }
}

// (the grid of every launch here is quant_grid over the row's 32-element blocks)
template <bool kModeW>
static int mx_launch(const void* X, const int16_t* idx, uint8_t* Q, uint8_t* SF, int64_t rows, int64_t KQ, int64_t KE, hipStream_t stream,
                     const char* who) {
  QuantRule r{who};
  r.family = kQuantMx;
  if (const int rc = quant_checks(r, QuantArgs{X, nullptr, idx, Q, SF, rows, KQ, KE})) return rc < 0 ? rc : ARCQ_OK;
  return launch_kernel<mx_quantize_rows_kernel<kModeW>>(quant_grid(rows, KQ / 32), dim3(kMxThreads), (int)lds_row_bytes((size_t)KQ), stream, who, (const uint16_t*)X,
                                                        idx, Q, SF, (int)rows, (int)KQ, (int)KE);
}

int mx_quantize_x(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, hipStream_t stream) {
  return mx_launch<false>(X, idx, QX, SFX, M, KQ, KE, stream, "arcq_mx_quantize_x");
}
int mx_quantize_w(const void* W, const int16_t* idx, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE, hipStream_t stream) {
  return mx_launch<true>(W, idx, QW, SFW, N, KQ, KE, stream, "arcq_mx_quantize_w");
}

template <int kSrc, bool kDirect>
static int mx_fused_launch(const void* X, const void* Xup, int64_t ldx, const void* Wn, float eps, const int16_t* idx, uint8_t* Q, uint8_t* SF,
                           int64_t rows, int64_t KQ, int64_t KE, hipStream_t stream, const char* who) {
  const size_t lds = kDirect ? 0 : lds_row_bytes((size_t)KQ) + (kSrc == kMxSrcRms ? 512 * sizeof(float) + lds_row_bytes((size_t)KQ) : 0);
  return launch_kernel<mx_fused_rows_kernel<kSrc, kDirect>>(quant_grid(rows, KQ / 32), dim3(kMxThreads), (int)lds, stream, who, (const uint16_t*)X,
                                                            (const uint16_t*)Xup, ldx, (const uint16_t*)Wn, eps, idx, Q, SF, (int)rows, (int)KQ, (int)KE);
}

int mx_rmsnorm_quantize_x(const void* X, const void* Wn, float eps, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ,
                          int64_t KE, hipStream_t stream) {
  QuantRule r{"arcq_mx_rmsnorm_quantize_x"};
  // 2048 <= KQ <= 8192: the reduction tree of rms_rstd_tree is defined for 128 .. 512 virtual threads (arcq_rmsnorm_quantize_x's range)
  r.family = kQuantMxFused; r.extra = true; r.kq_min = 2048; r.kq_max = 8192;
  if (const int rc = quant_checks(r, QuantArgs{X, Wn, idx, QX, SFX, M, KQ, KE})) return rc < 0 ? rc : ARCQ_OK;
  return mx_fused_launch<kMxSrcRms, false>(X, nullptr, KQ, Wn, eps, idx, QX, SFX, M, KQ, KE, stream, r.who);
}

int mx_silu_mul_quantize_x(const void* GU, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, int layout,
                           hipStream_t stream) {
  const char* who = "arcq_mx_silu_mul_quantize_x";
  QuantRule r{who};
  r.family = kQuantMxFused; r.layout = true;
  if (const int rc = quant_checks(r, QuantArgs{GU, nullptr, idx, QX, SFX, M, KQ, KE, ARCQ_VARIANT_G16, layout})) return rc < 0 ? rc : ARCQ_OK;
  const uint16_t* G = reinterpret_cast<const uint16_t*>(GU);
  const bool pairs = layout == ARCQ_GU_PAIRS;
  const uint16_t* U = pairs ? G : G + KQ;
  if (quant_grid(M, KQ / 32).y > 1)                           // rows split over workgroups: the direct gather
    return pairs ? mx_fused_launch<kMxSrcSiluPairs, true>(G, U, 2 * KQ, nullptr, 0.f, idx, QX, SFX, M, KQ, KE, stream, who)
                 : mx_fused_launch<kMxSrcSiluHalves, true>(G, U, 2 * KQ, nullptr, 0.f, idx, QX, SFX, M, KQ, KE, stream, who);
  return pairs ? mx_fused_launch<kMxSrcSiluPairs, false>(G, U, 2 * KQ, nullptr, 0.f, idx, QX, SFX, M, KQ, KE, stream, who)
               : mx_fused_launch<kMxSrcSiluHalves, false>(G, U, 2 * KQ, nullptr, 0.f, idx, QX, SFX, M, KQ, KE, stream, who);
}

}  // namespace arcq
