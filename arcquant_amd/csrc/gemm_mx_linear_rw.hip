// MXFP4 fused decode linear (arcq.h "MXFP4 fused decode linear"): the activation quantiser of M <= 16 token rows as the
// prologue of the repacked decode GEMM.  The K loop and the epilogues are mx_rw_kernel's (gemm_mx_rw.hip) over (MRW, MRSF) with one A
// fragment; the A operand is read from an LDS image that the workgroup's own prologue writes, not from global A / SFA.  Nothing
// quantised is written to global memory.
//
// Prologue.  A pass quantises R rows at once (R = 8, 4, 2 or 1: what the LDS budget leaves, mx_linear_rows): wave w stages row w of the
// pass (and once per workgroup all waves the norm weight) in the padded LDS layout of quantize_device.hpp and, kMxLinRms, forms the
// row's sum of squares and rstd alone, without a barrier (rms_stage_row_wave, quantize_source_device.hpp: the quantisers' tree).  After ONE
// barrier the R x KQ / 32 blocks of the pass are dealt to the 512 threads: a thread gathers its block through reorder_index -- the row
// bf16(x * wn * rstd) formed exactly as mx_fused_rows_kernel forms it -- and runs mx_quantize_block on it (primary block, in the outlier
// tail also the residual block; the padding blocks [K, Kp) are code 0, scale byte 127).  M = 4 rows of 3584 are 448 blocks: one pass,
// one block per thread.
//
// LDS image.  codes  [step][q 0..3][row 0..15][16 B]: block b = 4 step + q of row m.  Lane 16 q + r of a wave reads ONE aligned
//                    16-byte slot per step and the 64 lanes read 1 KB in lane order -- no bank conflict.
//             scales [step][row 0..15][4 B]: the dword of the row's four scale bytes in that step, byte q the block's (what the lane
//                    shifts down, as mx_rw_kernel shifts the dword it loads from SFA).
// Rows >= M of the image are never written and never read: lanes r >= M read row M - 1 (mx_rw_kernel's clamp), their sums are not stored.
//
// Who pays for the prologue.  The grid is persistent: min(N / 16, kMxLinCUs * kMxLinPerCU) workgroups, workgroup g takes the row blocks
// g, g + grid, ...; it quantises once and multiplies every row block of its own from the same image.  The weight and scale loads of a
// round are requested one round ahead -- the first round of the first row block before the prologue starts, the first round of the next
// row block under the last MFMAs and the end of this one -- so the prologue runs under the latency of the first loads.
//
// Every (m, n) sum is mx_rw_kernel's, bit for bit, whatever the grid: wave w multiplies the steps s = w (mod 8) in ascending order, one
// MFMA per step into one accumulator; the eight partial sums are added w = 0 .. 7; then the shared epilogue (gemm_mx_common.hpp).  The
// partial sums of consecutive row blocks alternate between two LDS buffers, so that a row block costs ONE barrier: wave 0 finishes row
// block i while the other waves multiply row block i + 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_common.hpp"
#include "quantize_device.hpp"
#include "quantize_mx_device.hpp"
#include "quantize_source_device.hpp"

namespace arcq {

constexpr int kMxLinThreads = 64 * kMxSmallWaves;
constexpr int kMxLinUnroll = 4;                                 // steps of loads in flight per wave = the bytes of an MRSF dword
constexpr int kMxLinRound = kMxSmallWaves * kMxLinUnroll;
constexpr int kMxLinTileBytes = 1024;
constexpr int kMxLinRoundSfBytes = kMxSmallWaves * 256;
constexpr int kMxLinPartBytes = 2 * kMxSmallWaves * 64 * 4 * (int)sizeof(float);   // two buffers of eight partial tiles
constexpr int kMxLinRstdBytes = kMxSmallWaves * (int)sizeof(float);
constexpr int kMxLinCUs = 256;
constexpr int kMxLinPerCU = 2;                                  // workgroups resident per CU: 4 waves per SIMD, <= 80 KB of LDS each
constexpr int64_t kMxLinLdsMax = 160 * 1024 / kMxLinPerCU;

enum : int { kMxLinRms = 0, kMxLinPlain = 1 };

// The LDS budget (arcq.h states it): the image, and behind it the prologue's staging (R rows and the norm weight) and the K loop's
// partial sums in ONE region (the first partial sums are written after the prologue's last barrier).  R is the largest of 8, 4, 2, 1
// that fits; 0: none does.
static int64_t mx_linear_lds_of(bool rms, int64_t KQ, int64_t KE, int rows) {
  const int64_t steps = (KQ + KE + 127) / 128, stage = (rows + (rms ? 1 : 0)) * (int64_t)lds_row_bytes((size_t)KQ);
  return steps * (kMxLinTileBytes + 64) + kMxLinRstdBytes + (stage > kMxLinPartBytes ? stage : kMxLinPartBytes);
}
static int mx_linear_rows(bool rms, int64_t KQ, int64_t KE) {
  for (int r = kMxSmallWaves; r >= 1; r >>= 1)
    if (mx_linear_lds_of(rms, KQ, KE, r) <= kMxLinLdsMax) return r;
  return 0;
}
int64_t gemm_mx_linear_lds_bytes(int kind, int64_t KQ, int64_t KE) {
  const bool rms = kind == ARCQ_SRC_RMSNORM;
  const int r = mx_linear_rows(rms, KQ, KE);
  return mx_linear_lds_of(rms, KQ, KE, r ? r : 1);
}
static bool mx_linear_shape_ok(int kind, int64_t N, int64_t KQ, int64_t KE) {
  const bool rms = kind == ARCQ_SRC_RMSNORM;
  return (rms || kind == ARCQ_SRC_PLAIN) && N > 0 && (N % 16) == 0 && KQ > 0 && (KQ % 64) == 0 && (KE % 64) == 0 && KE >= 0 && KE <= KQ &&
         KQ <= 32767 && (!rms || (KQ >= 2048 && KQ <= 8192));
}
int gemm_mx_linear_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE) {
  return M >= 1 && M <= 16 && mx_linear_shape_ok(kind, N, KQ, KE) && N <= INT32_MAX / 2 && gemm_mx_linear_lds_bytes(kind, KQ, KE) <= kMxLinLdsMax;
}
// workgroups of a launch (a pure host function): the resident set, or one per row block when there are fewer; 0 for no such launch.
// A library built with -DARCQ_MX_LINEAR_GRID_KNOB (make EXTRA=...; never the product build) reads another resident set from the
// environment variable ARCQ_MX_LINEAR_WGS: the grid experiment DESIGN.md 3.6 records.  Any grid gives the same results.
int64_t gemm_mx_linear_workgroups(int kind, int64_t N, int64_t KQ, int64_t KE) {
  if (!gemm_mx_linear_supported(kind, 1, N, KQ, KE)) return 0;
#ifdef ARCQ_MX_LINEAR_GRID_KNOB
  static const int cap = env_int("ARCQ_MX_LINEAR_WGS", kMxLinCUs * kMxLinPerCU);
#else
  constexpr int cap = kMxLinCUs * kMxLinPerCU;
#endif
  const int64_t nb = N / 16, c = cap < 1 ? 1 : cap;
  return nb < c ? nb : c;
}

struct MxLinArgs {
  MxArgs g;               // B / SFB = MRW / MRSF, D, M, N, Kp, alpha, bias, residual, out_dtype; A / SFA unused
  const uint16_t* X;      // bf16 [M, KQ]
  const uint16_t* Wn;     // kMxLinRms: bf16 [KQ]
  const int16_t* idx;
  float eps;
  int KQ, KE;
  int rows;               // R: rows quantised per pass
};

// block b of image row m
__device__ __forceinline__ void mx_lin_put(uint8_t* img, uint8_t* scl, int m, int b, const MxBlock& q) {
  *reinterpret_cast<uint4*>(img + (size_t)(b >> 2) * kMxLinTileBytes + (size_t)(((b & 3) << 4) + m) * 16) = q.packed;
  scl[(((b >> 2) << 4) + m) * 4 + (b & 3)] = (uint8_t)q.s8;
}

template <int kSrc, int kEpi>
__global__ __launch_bounds__(kMxLinThreads, 4) void mx_linear_kernel(MxLinArgs a) {   // 4 waves per SIMD = two workgroups per CU: <= 128 VGPRs
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kRms = kSrc == kMxLinRms;
  const MxArgs& p = a.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: row and round addresses in SGPRs)
  const int steps = p.Kp >> 7, rounds = (steps + kMxLinRound - 1) / kMxLinRound;
  const int nb = p.N >> 4, stride = (int)gridDim.x;
  uint8_t* img = smem;
  uint8_t* scl = smem + (size_t)steps * kMxLinTileBytes;
  float* rstd_s = reinterpret_cast<float*>(scl + (size_t)steps * 64);   // rstd of the rows of a pass
  unsigned char* post = scl + (size_t)steps * 64 + kMxLinRstdBytes;    // staging, then the partial sums

  // the loads of one round of row block rb (inside MRW / MRSF: steps are clamped to steps - 1 and the MRSF dword of a partial round exists)
  auto load_round = [&](int rb, int round, i32x4(&b)[kMxLinUnroll], uint32_t& sb) {
    const uint8_t* gW = p.B + (size_t)rb * (size_t)steps * kMxLinTileBytes + (size_t)lane * 16;
    const uint8_t* gSW = p.SFB + ((size_t)rb * (size_t)rounds * kMxSmallWaves + (size_t)wave) * 256 + (size_t)lane * 4;
    sb = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSW + (size_t)round * kMxLinRoundSfBytes));
#pragma unroll
    for (int u = 0; u < kMxLinUnroll; ++u) {
      const int s = min(wave + round * kMxLinRound + u * kMxSmallWaves, steps - 1);
      b[u] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gW + (size_t)s * kMxLinTileBytes));
    }
  };
  int rb = blockIdx.x;                                            // < nb: the grid has at most nb workgroups
  i32x4 b[kMxLinUnroll];
  uint32_t sb;
  load_round(rb, 0, b, sb);                                       // in flight under the prologue

  // ------------------------------------------------------------------------------------------------------------ prologue
  {
    const int KQ = a.KQ, KE = a.KE, K = KQ + KE, R = a.rows;
    const int B = KQ >> 5, P = (KQ - KE) >> 5, Bp = p.Kp >> 5, chunks = KQ >> 3;
    const size_t rowb = lds_row_bytes((size_t)KQ);
    const uint16_t* wn_lds = reinterpret_cast<const uint16_t*>(post + (size_t)R * rowb);
    if (kRms) {
      uint16_t* w = reinterpret_cast<uint16_t*>(post + (size_t)R * rowb);
      for (int c = tid; c < chunks; c += kMxLinThreads) lds_put_chunk(w, c, *reinterpret_cast<const uint4*>(a.Wn + (size_t)c * 8));
      // visible after the first pass's barrier
    }
    for (int m0 = 0; m0 < p.M; m0 += R) {
      const int nrow = min(R, p.M - m0);
      if (wave < nrow) {                                          // (R <= the waves of the workgroup)
        uint16_t* row = reinterpret_cast<uint16_t*>(post + (size_t)wave * rowb);
        const uint16_t* xrow = a.X + (size_t)(m0 + wave) * (size_t)KQ;
        if constexpr (kRms) {
          int l = lane;
          asm volatile("" : "+v"(l));                             // the chunk offsets are formed here, per pass: hoisted out of the pass loop they spill
          const float rstd = rms_stage_row_wave(row, xrow, KQ >> 4, KQ, a.eps, l);
          if (lane == 0) rstd_s[wave] = rstd;
        } else {
          for (int c = lane; c < chunks; c += 64) lds_put_chunk(row, c, *reinterpret_cast<const uint4*>(xrow + (size_t)c * 8));
        }
      }
      __syncthreads();
      for (int task = tid; task < nrow * B; task += kMxLinThreads) {
        const int r = task / B, blk = task - r * B, m = m0 + r;
        const uint16_t* row_lds = reinterpret_cast<const uint16_t*>(post + (size_t)r * rowb);
        const float rstd = kRms ? rstd_s[r] : 1.0f;
        float v[32];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint4 i0 = *reinterpret_cast<const uint4*>(a.idx + (size_t)blk * 32 + h * 16);
          const uint4 i1 = *reinterpret_cast<const uint4*>(a.idx + (size_t)blk * 32 + h * 16 + 8);
          const uint32_t iw[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t pw = lds_pad_pair(iw[j]), pa = pw & 0xffffu, pb = pw >> 16;
            float x0 = bf16_bits_to_f32(row_lds[pa]), x1 = bf16_bits_to_f32(row_lds[pb]);
            if (kRms) {                                           // (x * w) * rstd in fp32, then bf16: mx_fused_rows_kernel's statement
              x0 = round_to_bf16(x0 * bf16_bits_to_f32(wn_lds[pa]) * rstd);
              x1 = round_to_bf16(x1 * bf16_bits_to_f32(wn_lds[pb]) * rstd);
            }
            v[16 * h + 2 * j] = x0;
            v[16 * h + 2 * j + 1] = x1;
          }
        }
        if (blk < P) {                                            // mx_store_x_block's rule, into the image
          mx_lin_put(img, scl, m, blk, mx_quantize_block<false>(v));
        } else {
          mx_lin_put(img, scl, m, blk, mx_quantize_block<true>(v));
          mx_lin_put(img, scl, m, B + (blk - P), mx_quantize_block<false>(v));
        }
      }
      if (tid < 4 * nrow) {                                       // mx_store_padding's rule: at most three blocks per row
        const int pb = (K >> 5) + (tid & 3);
        if (pb < Bp) {
          MxBlock z;
          z.packed = make_uint4(0, 0, 0, 0);
          z.s8 = 127;
          mx_lin_put(img, scl, m0 + (tid >> 2), pb, z);
        }
      }
      __syncthreads();                                            // the image rows are written; the staged rows are rewritten by the next pass
    }
  }

  // ------------------------------------------------------------------------------------------------------------ K loops
  const int r16 = lane & 15, q = lane >> 4, sh = 8 * q;
  const int rc = min(r16, p.M - 1);
  const uint8_t* la = img + (size_t)((q << 4) + rc) * 16;
  const uint8_t* ls = scl + (size_t)rc * 4;
  float* part = reinterpret_cast<float*>(post);                   // [2][waves][64][4]
  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  for (int buf = 0; rb < nb; rb += stride, buf ^= 1) {
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int round = 0; round < rounds; ++round) {
      i32x4 bn[kMxLinUnroll];
      uint32_t sbn = sb;
#pragma unroll
      for (int u = 0; u < kMxLinUnroll; ++u) bn[u] = b[u];
      const bool last = round + 1 == rounds;
      const int nrb = last ? rb + stride : rb;
      if (nrb < nb) load_round(nrb, last ? 0 : round + 1, bn, sbn);   // (uniform over the workgroup)
      const int s0 = wave + round * kMxLinRound;
#pragma unroll
      for (int u = 0; u < kMxLinUnroll; ++u) {
        const int s = s0 + u * kMxSmallWaves;
        if (s < steps) {
          const i32x4 av = *reinterpret_cast<const i32x4*>(la + (size_t)s * kMxLinTileBytes);
          const uint32_t sa = *reinterpret_cast<const uint32_t*>(ls + (size_t)s * 64);
          acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(av), frag(b[u]), acc, 4, 4, 0, (int)(sa >> sh), 0, (int)(sb >> (8 * u)));
        }
      }
#pragma unroll
      for (int u = 0; u < kMxLinUnroll; ++u) b[u] = bn[u];
      sb = sbn;
    }
    float* pt = part + (size_t)buf * (kMxSmallWaves * 256);
    *reinterpret_cast<f32x4*>(pt + (wave * 64 + lane) * 4) = acc;
    __syncthreads();
    if (wave != 0) continue;                                       // wave 0 finishes the row block's 16 x 16 tile (rows < M)
    const int n = rb * 16 + r16;
    f32x4 t = *reinterpret_cast<const f32x4*>(pt + lane * 4);
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(pt + (w * 64 + lane) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] += o[r];
    }
    if constexpr (kEpi == kEpiSiluMul) {
      const bool odd = lane & 1;
      const float bias = p.bias ? bf16_bits_to_f32(p.bias[n]) : 0.0f;
      uint16_t* act = reinterpret_cast<uint16_t*>(p.D) + (n >> 1);
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, t[r], p.bias, bias), mx_y_bits(alpha, t[r + 1], p.bias, bias), odd);
        const int m = 4 * q + r + (odd ? 1 : 0);
        if (!(lane & 2) && m < p.M) *reinterpret_cast<uint32_t*>(act + (size_t)m * (size_t)(p.N >> 1)) = pk;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * q + r;
        if (m < p.M) mx_store(p, alpha, m, n, t[r]);
      }
    }
  }
}

template <int kSrc, int kEpi>
static int mx_linear_launch(const MxLinArgs& a, int kind, const char* who, hipStream_t stream) {
  const int64_t lds = gemm_mx_linear_lds_bytes(kind, a.KQ, a.KE);
  const dim3 grid((unsigned)gemm_mx_linear_workgroups(kind, a.g.N, a.KQ, a.KE)), block(kMxLinThreads);
  return launch_kernel<mx_linear_kernel<kSrc, kEpi>>(grid, block, LdsBytes((int)lds, (int)kMxLinLdsMax), stream, who, a);
}

int gemm_mx_linear(int kind, bool silu, const void* X, const void* Wn, float eps, const int16_t* idx, const uint8_t* MRW, const uint8_t* MRSF, void* D,
                   int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host, const float* alpha_dev, const void* bias, const void* residual,
                   int out_dtype, const char* who, hipStream_t stream) {
  if (!gemm_mx_linear_supported(kind, M, N, KQ, KE))
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: no fused kernel for this shape (see arcq_mx_linear_fused_supported; M=%lld N=%lld KQ=%lld KE=%lld)", who,
                (long long)M, (long long)N, (long long)KQ, (long long)KE);
  MxLinArgs a;
  MxArgs& p = a.g;
  p.A = nullptr; p.SFA = nullptr; p.B = MRW; p.SFB = MRSF; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)((KQ + KE + 127) / 128 * 128);
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  a.X = (const uint16_t*)X; a.Wn = (const uint16_t*)Wn; a.idx = idx; a.eps = eps; a.KQ = (int)KQ; a.KE = (int)KE;
  a.rows = mx_linear_rows(kind == ARCQ_SRC_RMSNORM, KQ, KE);
  if (kind == ARCQ_SRC_RMSNORM)
    return silu ? mx_linear_launch<kMxLinRms, kEpiSiluMul>(a, kind, who, stream) : mx_linear_launch<kMxLinRms, kEpiPlain>(a, kind, who, stream);
  if (silu) return fail(ARCQ_ERR_UNSUPPORTED, "%s: the plain source has no SiLU form", who);   // (no entry point asks for it)
  return mx_linear_launch<kMxLinPlain, kEpiPlain>(a, kind, who, stream);
}

}  // namespace arcq
