// The quantising MXFP4 gate|up GEMM for M <= kMxSmallM over a weight repacked into MFMA operand order (arcq.h "MXFP4 repacked weight"):
// mx_slice_quant_kernel's work (gemm_mx.hip) with B from (MRW, MRSF).  A workgroup owns FOUR adjacent row blocks -- 64 y-columns, one
// 32-block of activations per row -- and 16 rows of A (grid N/64 x ceil(M / 16): the weight is read once per 16 rows of M, once in all for
// M <= 16; four A fragments per workgroup, as mx_rw_kernel has them, would carry 16 accumulator quads and 16 + 4 x 4 fragments in flight
// per wave, past the 128 registers that let two workgroups share a CU).  The 8 waves split K as mx_small_kernel and mx_rw_kernel do: wave
// w takes the steps s = w (mod 8) in ascending order, one 16x16x128 MFMA per step and row block into one accumulator, and the partial
// sums are added w = 0 .. 7 -- every (m, n) sum is mx_slice_quant_kernel's, bit for bit -- then the shared ending
// (gemm_mx_slice_finish.inc) quantises through mx_quantize_act_block.  Per round of 32 steps a wave fetches, for each of its row blocks,
// ONE MRSF dword per lane (its scale byte in the round's four steps of this wave) and four contiguous 1 KB spans of MRW, all
// non-temporal: each weight byte is used once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_tile_common.hpp"

namespace arcq {

constexpr int kMxSliceRwUnroll = 4;                             // steps of loads in flight per wave = the bytes of an MRSF dword
static_assert(kMxSmallWaves * kMxSliceRwUnroll == kMxRwRoundSteps, "a wave's loop iteration is one MRSF round");

__global__ __launch_bounds__(64 * kMxSmallWaves, 4) void mx_slice_rw_quant_kernel(MxArgs p) {   // <= 128 VGPRs: two workgroups per CU
  __shared__ __attribute__((aligned(16))) float part[kMxSmallWaves][kMxSliceFrags][64][4];
  __shared__ __attribute__((aligned(16))) uint8_t act[16 * kMxSliceActRowBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kMxSliceCols, m0 = blockIdx.y * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7, rounds = (steps + kMxRwRoundSteps - 1) / kMxRwRoundSteps;
  const int r16 = lane & 15, q = lane >> 4;
  // every address below is inside its operand: N % 128 == 0 (the four row blocks exist), steps are clamped to steps - 1, rows to M - 1,
  // and the MRSF dword of a partial round exists (the array is padded to whole rounds)
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowb + q * 16;
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const size_t wblock = (size_t)steps * 1024, sblock = (size_t)rounds * (kMxSmallWaves * 256);      // bytes of one row block
  const uint8_t* gW = p.B + (size_t)blockIdx.x * kMxSliceFrags * wblock + (size_t)lane * 16;
  const uint8_t* gSW = p.SFB + (size_t)blockIdx.x * kMxSliceFrags * sblock + (size_t)wave * 256 + (size_t)lane * 4;
  const int sh = 8 * q;
  f32x4 acc[kMxSliceFrags];
#pragma unroll
  for (int j = 0; j < kMxSliceFrags; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave, round = 0; s0 < steps; s0 += kMxRwRoundSteps, ++round) {
    i32x4 a[kMxSliceRwUnroll], b[kMxSliceRwUnroll][kMxSliceFrags];
    uint32_t sa[kMxSliceRwUnroll], sb[kMxSliceFrags];
#pragma unroll
    for (int j = 0; j < kMxSliceFrags; ++j)
      sb[j] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSW + (size_t)j * sblock + (size_t)round * (kMxSmallWaves * 256)));
#pragma unroll
    for (int u = 0; u < kMxSliceRwUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMAs of a step past the end are skipped
#pragma unroll
      for (int j = 0; j < kMxSliceFrags; ++j) b[u][j] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gW + (size_t)j * wblock + (size_t)s * 1024));
      a[u] = *reinterpret_cast<const i32x4*>(gA + (size_t)s * 64);
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + (size_t)s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMxSliceRwUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps) {
#pragma unroll
        for (int j = 0; j < kMxSliceFrags; ++j)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u]), frag(b[u][j]), acc[j], 4, 4, 0, (int)(sa[u] >> sh), 0,
                                                                    (int)(sb[j] >> (8 * u)));
      }
  }
#include "gemm_mx_slice_finish.inc"
}

// p.B / p.SFB = MRW / MRSF; 1 <= M <= kMxSmallM, N % 128 == 0
int gemm_mx_slice_rw_quantize(const MxArgs& p, const char* who, hipStream_t stream) {
  return launch_kernel<mx_slice_rw_quant_kernel>(dim3((unsigned)(p.N / kMxSliceCols), (unsigned)((p.M + 15) / 16)), dim3(64 * kMxSmallWaves), 0,
                                                 stream, who, p);
}

}  // namespace arcq
