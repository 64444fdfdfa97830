// MXFP4 GEMM for gfx950 on the block-scaled fp4 MFMA (v_mfma_scale_f32_{32x32x64,16x16x128}_f8f6f4, cbsz = blgp = 4).
//
//   D[m,n] = alpha * sum_{k < Kp} deq(A[m,k]) * deq(B[n,k])      A [M, Kp/2], B [N, Kp/2] e2m1, SFA / SFB [rows, Kp/32] E8M0
//
// Every product of two e2m1 codes and two power-of-two scales is exact, so the instruction takes the packed codes and the
// scale bytes as they are stored: no dequantisation instruction, the matrix pipe at the fp4 rate.
//
// Operand map of the fp4 form (pinned by tests/test_mx_gpu.py::test_lane_map_exact with exact integer data):
//   16x16x128: lane l supplies row l & 15, K elements [32 (l >> 4), +32) = 16 bytes, and the scale byte of that 32-block;
//   32x32x64:  lane l supplies row l & 31, K elements [32 (l >> 5), +32) and the scale byte of that block.
//   The scale operand is a VGPR; op_sel picks one of its bytes for the whole wave, so each lane shifts its byte down and
//   op_sel stays 0.  C/D as every gfx950 MFMA: 32x32 reg r of lane l = D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31],
//   16x16 reg r of lane l = D[4 (l >> 4) + r][l & 15]  (row = A's row, column = B's row).
//
// Two configurations:
//   mx_tile_kernel   M > kMxSmallM: 128 x 128 tiles, 4 waves of 64 x 64 (2 x 2 MFMA 32x32x64), K steps of 128 staged through
//                    LDS (XOR-swizzled 64-byte rows: the 16-byte fragment reads are bank-conflict free), double-buffered: the
//                    global loads of step s + 1 are in flight while step s computes.
//   mx_small_kernel  M <= kMxSmallM: one 16-column slice of B per workgroup (each weight byte is read by ONE workgroup
//                    when M <= 16), 8 waves splitting K, four K steps of loads in flight per wave, 16x16x128 MFMA, partial
//                    sums added in LDS in a fixed order.
//
// Both kernels take the epilogue as a template parameter.  kEpiSiluMul (arcq_gemm_mxfp4_silu_mul): B's rows interleave gate and up
// (g0, u0, g1, u1, ...), D = bf16 [M, N/2] receives silu(y_gate) * y_up with torch's roundings, y being the bf16 value the plain epilogue
// would store (never written).  A lane holds ONE output column, so gate and up of a pair sit in neighbouring lanes of a DPP quad (N % 16
// == 0: a quad of lanes is inside or outside n < N as a whole); see mx_silu_pair.
//
// kEpiSiluMulQuant (arcq_gemm_mxfp4_silu_mul_quantize): the same activations are not stored but quantised where they are, to the
// MXFP4-ARC operand of the next GEMM (QACT, SFACT = arcq_mx_quantize_x of ACT with the identity reorder_index).  A block's E8M0 scale
// needs the 32 values of the block and nothing else, and 32 adjacent activations are 64 adjacent y-columns: a 128-column tile holds two
// whole blocks per row (N % 128 == 0: no ragged column tile).  The activations of a tile go through the LDS the K loop has finished
// with, one thread then quantises one (row, block) with the quantisers' own mx_store_x_block -- residual blocks of the outlier tail
// and the row's padding blocks included.  M <= kMxSmallM: mx_slice_quant_kernel, mx_small_kernel's K split and sum order over a
// 64-column slice (one block per row) instead of a 16-column one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_tile_common.hpp"

namespace arcq {

// ---------------------------------------------------------------------------------------------------------------- tiled
// (geometry, LDS image and mx_quantize_act_block: gemm_mx_tile_common.hpp; the statements: gemm_mx_tile_body.inc, shared with
// gemm_mx_tile_rw.hip, which stages B from the repacked weight)
template <int kEpi>
__global__ __launch_bounds__(256) void mx_tile_kernel(MxArgs p) {
  constexpr bool kRepackedB = false;
#include "gemm_mx_tile_body.inc"
}

// ---------------------------------------------------------------------------------------------------------------- small M
constexpr int kMxSmallUnroll = 4;

template <int kEpi>
__global__ __launch_bounds__(64 * kMxSmallWaves) void mx_small_kernel(MxArgs p) {
  __shared__ float part[kMxSmallWaves][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  const int r16 = lane & 15, q = lane >> 4;
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowb + q * 16;
  const uint8_t* gB = p.B + (size_t)(n0 + r16) * rowb + q * 16;                     // N % 16 == 0: always in range
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const uint8_t* gSB = p.SFB + (size_t)(n0 + r16) * rows;
  const int sh = 8 * q;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave; s0 < steps; s0 += kMxSmallWaves * kMxSmallUnroll) {
    i32x4 a[kMxSmallUnroll], b[kMxSmallUnroll];
    uint32_t sa[kMxSmallUnroll], sb[kMxSmallUnroll];
#pragma unroll
    for (int u = 0; u < kMxSmallUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMA of a step past the end is skipped
      b[u] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gB + (size_t)s * 64));
      sb[u] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSB + (size_t)s * 4));
      a[u] = *reinterpret_cast<const i32x4*>(gA + (size_t)s * 64);
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + (size_t)s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMxSmallUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps)
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u]), frag(b[u]), acc, 4, 4, 0, (int)(sa[u] >> sh), 0,
                                                               (int)(sb[u] >> sh));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][lane][r] = acc[r];
  __syncthreads();
  if (wave != 0) return;
  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  const int n = n0 + r16;
  float t[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t[r] = part[0][lane][r];
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) t[r] += part[w][lane][r];
  }
  if constexpr (kEpi == kEpiSiluMul) {
    const bool odd = lane & 1;
    const float bias = p.bias ? bf16_bits_to_f32(p.bias[n]) : 0.0f;
    uint16_t* act = reinterpret_cast<uint16_t*>(p.D) + (n >> 1);
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, t[r], p.bias, bias), mx_y_bits(alpha, t[r + 1], p.bias, bias), odd);
      const int m = m0 + 4 * q + r + (odd ? 1 : 0);
      if (!(lane & 2) && m < p.M) *reinterpret_cast<uint32_t*>(act + (size_t)m * (size_t)(p.N >> 1)) = pk;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 4 * q + r;
      if (m < p.M) mx_store(p, alpha, m, n, t[r]);
    }
  }
}

// kEpiSiluMulQuant for M <= kMxSmallM.  mx_small_kernel's 16 y-columns are 8 activations, a quarter of a block; this kernel gives a
// workgroup 64 y-columns = one block per row: one A fragment against four B fragments per K step.  Every (m, n) sum is mx_small_kernel's:
// wave w takes the steps s = w (mod 8) in ascending order, the eight partial sums are added w = 0 .. 7.  Waves 0 .. 3 each finish one
// 16-column fragment and put its activations into LDS (rows of 64 bytes padded to 80: 20 r mod 64 is a different multiple of 4 for each
// of the 16 rows); 16 threads then quantise one row's block each.
constexpr int kMxSliceUnroll = 2;

__global__ __launch_bounds__(64 * kMxSmallWaves) void mx_slice_quant_kernel(MxArgs p) {
  __shared__ __attribute__((aligned(16))) float part[kMxSmallWaves][kMxSliceFrags][64][4];
  __shared__ __attribute__((aligned(16))) uint8_t act[16 * kMxSliceActRowBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kMxSliceCols, m0 = blockIdx.y * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  const int r16 = lane & 15, q = lane >> 4;
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowb + q * 16;
  const uint8_t* gB = p.B + (size_t)(n0 + r16) * rowb + q * 16;                     // N % 128 == 0: always in range
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const uint8_t* gSB = p.SFB + (size_t)(n0 + r16) * rows;
  const int sh = 8 * q;
  f32x4 acc[kMxSliceFrags];
#pragma unroll
  for (int j = 0; j < kMxSliceFrags; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave; s0 < steps; s0 += kMxSmallWaves * kMxSliceUnroll) {
    i32x4 a[kMxSliceUnroll], b[kMxSliceUnroll][kMxSliceFrags];
    uint32_t sa[kMxSliceUnroll], sb[kMxSliceUnroll][kMxSliceFrags];
#pragma unroll
    for (int u = 0; u < kMxSliceUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMAs of a step past the end are skipped
#pragma unroll
      for (int j = 0; j < kMxSliceFrags; ++j) {
        b[u][j] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gB + (size_t)j * 16 * rowb + (size_t)s * 64));
        sb[u][j] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSB + (size_t)j * 16 * rows + (size_t)s * 4));
      }
      a[u] = *reinterpret_cast<const i32x4*>(gA + (size_t)s * 64);
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + (size_t)s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMxSliceUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps) {
#pragma unroll
        for (int j = 0; j < kMxSliceFrags; ++j)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u]), frag(b[u][j]), acc[j], 4, 4, 0, (int)(sa[u] >> sh), 0,
                                                                    (int)(sb[u][j] >> sh));
      }
  }
#include "gemm_mx_slice_finish.inc"
}

template <int kEpi>
static int mx_launch_gemm(const MxArgs& p, const char* who, hipStream_t stream) {
  if (p.M <= kMxSmallM) {
    const dim3 block(64 * kMxSmallWaves);
    const unsigned rows16 = (unsigned)((p.M + 15) / 16);
    if constexpr (kEpi == kEpiSiluMulQuant) return launch_kernel<mx_slice_quant_kernel>(dim3((unsigned)(p.N / kMxSliceCols), rows16), block, 0, stream, who, p);
    else return launch_kernel<mx_small_kernel<kEpi>>(dim3((unsigned)(p.N / 16), rows16), block, 0, stream, who, p);
  }
  return launch_kernel<mx_tile_kernel<kEpi>>(dim3((unsigned)((p.N + kMxTile - 1) / kMxTile), (unsigned)((p.M + kMxTile - 1) / kMxTile)), dim3(256), 0, stream, who, p);
}

int gemm_mx(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t Kp,
            float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return mx_launch_gemm<kEpiPlain>(p, "arcq_gemm_mxfp4", stream);
}

// ACT = bf16 [M, N/2]; the same contraction, kernel choice and accumulation order as gemm_mx
int gemm_mx_silu_mul(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* ACT, int64_t M, int64_t N, int64_t Kp,
                     float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = ACT;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = nullptr; p.out_dtype = ARCQ_OUT_BF16;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return mx_launch_gemm<kEpiSiluMul>(p, "arcq_gemm_mxfp4_silu_mul", stream);
}

// (QACT, SFACT) = mx_quantize_x(ACT of gemm_mx_silu_mul, identity, KQ2 = N/2, KE); ACT is never written.  N % 128 == 0.
int gemm_mx_silu_mul_quantize(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, uint8_t* QACT, uint8_t* SFACT, int64_t M,
                              int64_t N, int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = nullptr;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = nullptr; p.out_dtype = ARCQ_OUT_BF16;
  p.QACT = QACT; p.SFACT = SFACT; p.KE = (int)KE;
  return mx_launch_gemm<kEpiSiluMulQuant>(p, "arcq_gemm_mxfp4_silu_mul_quantize", stream);
}

}  // namespace arcq
