// MXFP6 decode GEMM (M <= kMxSmallM) with e3m2 activations over a weight repacked into MFMA operand order (arcq.h "MXFP6 repacked weight").
//
//   kBFmt = ARCQ_MX_B_E3M2:  MRW is the layout MRW6.  Row block b (16 rows) and step t (128 K elements) own the 1536 adjacent bytes at
//         (b * T + t) * 1536, T = Kp / 128: bytes [0, 1024) are [lane 0..63][16], bytes 0..15 of the lane's 24-byte block, bytes
//         [1024, 1536) are [lane][8], bytes 16..23 of it.  Lane 16 q + r holds row 16 b + r, K elements [128 t + 32 q, +32): bytes
//         [96 t + 24 q, +24) of that QW row, unchanged -- the six-register operand of one 16x16x128 scaled MFMA as frag6 builds it.  A
//         wave's fetch of a step is ONE global_load_dwordx4 over a contiguous 1 KB and ONE global_load_dwordx2 over a contiguous 512 B,
//         both naturally aligned (mx6_small_kernel: 16 pieces of 16 weight rows, 8-byte aligned only).
//   kBFmt = ARCQ_MX_B_E2M1:  MRW is MXFP4's repacked weight as it is (arcq.h "MXFP4 repacked weight"): 1 KB per (b, t), one dwordx4.
//   MRSF  is MXFP4's in both forms: [row block][round = t / 32][wave = t % 8][lane][u = (t / 8) % 4], one dword per (round, wave, lane),
//         the steps of a partial last round padded; a padding byte is never multiplied (the MFMAs of a step past the end are skipped).
//
// mx6_rw_kernel<kBFmt, kF>: mx_rw_kernel's work split.  The grid is N / 16 workgroups of 8 waves; a workgroup owns ONE row block and
// reads it exactly once, whatever M is; wave w takes the steps s = w (mod 8) in ascending order and multiplies each B fragment against
// all kF = ceil(M / 16) A fragments into kF accumulator quads.  The activations keep their row-major form and come from global memory,
// 24 bytes per lane and step at an 8-byte-aligned address (dwordx4 + dwordx2, mx6_small_kernel's fetch); rows are clamped to M - 1 and
// steps to steps - 1, so no address leaves its operand.
//
// The e3m2 x e3m2 split is on the WEIGHT side.  The instruction cuts products 14 bits below the largest of their 32-block (gemm_mx6.hip,
// "Two MFMAs per e3m2 pair"), so one operand is split into its codes of magnitude >= 2 and the others and each half multiplied by its
// own MFMA into the same accumulator.  mx6_split_fragment works on any e3m2 fragment and the argument is symmetric: B's large codes are
// multiples of 1/2 and A's codes multiples of 1/16, so those products are multiples of 2^-5 below 28 * 28 < 2^10; B's small codes are
// below 2, products multiples of 2^-8 below 2 * 28 < 2^6: both sets fit the 14 bits, nothing is cut.  Splitting B costs one split per
// wave and step whatever kF is; splitting A (mx6_small_kernel) would cost kF of them.  An e2m1 B needs no split and keeps one MFMA.
//
// Steps in flight.  A step is 6 (B; 4 for e2m1) + 6 kF (A) + kF (A's scale dwords) registers.  kF <= 2 keeps the four steps of an MRSF
// dword in flight; kF = 3, 4 fetch them as two pairs (four steps at kF = 4 are 136 registers, above the 128 that two 512-thread
// workgroups per CU allow).  VGPR counts per instantiation: DESIGN.md 3.7; none spills.
//
// Summation order per output, which tests/test_mx6_gpu.py::gamma counts.  Wave w accumulates its steps in ascending order, ceil(steps / 8)
// accumulations against an e2m1 weight, twice that against an e3m2 weight (B's large codes, then its small ones, per step); the eight
// partial sums go to LDS and are added w = 0 .. 7 (7 additions; wave f adds those of A fragment f); then alpha and mx_store
// (gemm_mx_common.hpp).  Against an e2m1 weight this is mx6_small_kernel's sum bit for bit; against an e3m2 weight the products are the
// same but grouped by B's codes instead of A's, so the result agrees within the bound, not bit for bit.
// Row offsets are size_t throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx6_common.hpp"

namespace arcq {

constexpr int kMx6RwRound = kMxSmallWaves * 4;                  // steps of one MRSF round: a dword's four bytes per wave
constexpr int kMx6RwTileBytes = 1536;                           // one (row block, step) of MRW6: 1024 + 512
constexpr int kMx6RwRoundSfBytes = kMxSmallWaves * 256;

int64_t gemm_mx6_repacked_w_bytes(int64_t N, int64_t Kp) { return (N <= 0 || Kp <= 0 || (N % 16) || (Kp % 128)) ? 0 : N * (Kp / 4 * 3); }
int gemm_mx6_repacked_supported(int64_t M, int64_t N, int64_t Kp) { return gemm_mx_repacked_supported(M, N, Kp); }

template <int kBFmt, int kF>
__global__ __launch_bounds__(64 * kMxSmallWaves, 4) void mx6_rw_kernel(MxArgs p) {   // 4 waves per SIMD = two workgroups per CU: <= 128 VGPRs
  constexpr bool kB6 = kBFmt == ARCQ_MX_B_E3M2;
  constexpr int kBCbsz = kB6 ? kMx6Fmt : 4;
  constexpr int kTile = kB6 ? kMx6RwTileBytes : 1024;
  constexpr int kDepth = kF <= 2 ? 4 : 2;                        // steps of loads in flight per wave
  __shared__ __attribute__((aligned(16))) float part[kMxSmallWaves][kF][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const size_t rowa = (size_t)(p.Kp >> 2) * 3, rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7, rounds = (steps + kMx6RwRound - 1) / kMx6RwRound;
  const int r16 = lane & 15, q = lane >> 4;
  // every address below is inside its operand: steps are clamped to steps - 1, rows to M - 1, and the MRSF dword of a partial round exists
  const uint8_t* gW = p.B + (size_t)blockIdx.x * (size_t)steps * kTile;
  const uint8_t* gSW = p.SFB + ((size_t)blockIdx.x * (size_t)rounds * kMxSmallWaves + (size_t)wave) * 256 + (size_t)lane * 4;
  const uint8_t* gA[kF];
  const uint8_t* gSA[kF];
#pragma unroll
  for (int f = 0; f < kF; ++f) {
    const size_t m = (size_t)min(16 * f + r16, p.M - 1);
    gA[f] = p.A + m * rowa + q * 24;
    gSA[f] = p.SFA + m * rows;
  }
  const int sh = 8 * q;
  f32x4 acc[kF];
#pragma unroll
  for (int f = 0; f < kF; ++f) acc[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave, round = 0; s0 < steps; s0 += kMx6RwRound, ++round) {
    const uint32_t sb = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSW + (size_t)round * kMx6RwRoundSfBytes));
#pragma unroll
    for (int u0 = 0; u0 < 4; u0 += kDepth) {
      if (u0 > 0 && s0 + u0 * kMxSmallWaves >= steps) break;      // (uniform in the wave) nothing left of this round
      i32x8 a[kDepth][kF], b[kDepth];
      uint32_t sa[kDepth][kF];
#pragma unroll
      for (int u = 0; u < kDepth; ++u) {
        const size_t s = (size_t)min(s0 + (u0 + u) * kMxSmallWaves, steps - 1);      // clamped loads; the MFMAs of a step past the end are skipped
        const uint8_t* pb = gW + s * kTile;
        if constexpr (kB6)
          b[u] = frag6(ARCQ_WLOAD(reinterpret_cast<const i32x4*>(pb + lane * 16)), ARCQ_WLOAD(reinterpret_cast<const i32x2*>(pb + 1024 + lane * 8)));
        else
          b[u] = frag(ARCQ_WLOAD(reinterpret_cast<const i32x4*>(pb + lane * 16)));
#pragma unroll
        for (int f = 0; f < kF; ++f) {
          const uint8_t* pa = gA[f] + s * kMx6StepBytes;
          a[u][f] = frag6(*reinterpret_cast<const i32x4_a8*>(pa), *reinterpret_cast<const i32x2_a8*>(pa + 16));
          sa[u][f] = *reinterpret_cast<const uint32_t*>(gSA[f] + s * 4);
        }
      }
#pragma unroll
      for (int u = 0; u < kDepth; ++u)
        if (s0 + (u0 + u) * kMxSmallWaves < steps) {
          const int sbu = (int)(sb >> (8 * (u0 + u)));
          if constexpr (kB6) {             // e3m2 x e3m2: B's large codes first, then its small ones (header)
            i32x8 bh, bl;
            split6(b[u], bh, bl);
#pragma unroll
            for (int f = 0; f < kF; ++f) {
              acc[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[u][f], bh, acc[f], kMx6Fmt, kBCbsz, 0, (int)(sa[u][f] >> sh), 0, sbu);
              acc[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[u][f], bl, acc[f], kMx6Fmt, kBCbsz, 0, (int)(sa[u][f] >> sh), 0, sbu);
            }
          } else {
#pragma unroll
            for (int f = 0; f < kF; ++f)
              acc[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[u][f], b[u], acc[f], kMx6Fmt, kBCbsz, 0, (int)(sa[u][f] >> sh), 0, sbu);
          }
        }
    }
  }
#pragma unroll
  for (int f = 0; f < kF; ++f) *reinterpret_cast<f32x4*>(part[wave][f][lane]) = acc[f];
  __syncthreads();
  if (wave >= kF) return;                                        // wave f finishes A fragment f: rows [16 f, 16 f + 16)
  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  const int n = n0 + r16, m0 = 16 * wave;
  f32x4 t = *reinterpret_cast<const f32x4*>(part[0][wave][lane]);
#pragma unroll
  for (int w = 1; w < kMxSmallWaves; ++w) {
    const f32x4 o = *reinterpret_cast<const f32x4*>(part[w][wave][lane]);
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] += o[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * q + r;
    if (m < p.M) mx_store(p, alpha, m, n, t[r]);
  }
}

template <int kBFmt>
static int mx6_rw_launch(const MxArgs& p, hipStream_t stream) {
  const char* who = "arcq_gemm_mxfp6_repacked";
  const dim3 grid((unsigned)(p.N / 16)), block(64 * kMxSmallWaves);
  switch ((p.M + 15) / 16) {
    case 1: return launch_kernel<mx6_rw_kernel<kBFmt, 1>>(grid, block, 0, stream, who, p);
    case 2: return launch_kernel<mx6_rw_kernel<kBFmt, 2>>(grid, block, 0, stream, who, p);
    case 3: return launch_kernel<mx6_rw_kernel<kBFmt, 3>>(grid, block, 0, stream, who, p);
    default: return launch_kernel<mx6_rw_kernel<kBFmt, 4>>(grid, block, 0, stream, who, p);
  }
}

int gemm_mx6_repacked(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
                      int b_format, float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype,
                      hipStream_t stream) {
  if (!gemm_mx6_repacked_supported(M, N, Kp))
    return fail(ARCQ_ERR_SHAPE, "arcq_gemm_mxfp6_repacked: need 1 <= M <= %d, N %% 16 == 0 and K %% 128 == 0 (M=%lld N=%lld K=%lld)", kMxSmallM,
                (long long)M, (long long)N, (long long)Kp);
  MxArgs p;
  p.A = A; p.B = MRW; p.SFA = SFA; p.SFB = MRSF; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return b_format == ARCQ_MX_B_E3M2 ? mx6_rw_launch<ARCQ_MX_B_E3M2>(p, stream) : mx6_rw_launch<ARCQ_MX_B_E2M1>(p, stream);
}

}  // namespace arcq
