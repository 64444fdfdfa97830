// MXFP4 decode GEMM (M <= kMxSmallM) over a weight repacked into MFMA operand order (arcq.h "MXFP4 repacked weight").
//
//   MRW   [N/16 row blocks][Kp/128 steps][lane 0..63][16 bytes]: lane 16 q + r of step t in row block b holds row 16 b + r, K elements
//         [128 t + 32 q, +32) -- the B operand of one 16x16x128 MFMA as the instruction takes it.  A wave's load is ONE contiguous 1 KB span.
//   MRSF  [row block][round = t / 32][wave = t % 8][lane][u = (t / 8) % 4]: the dword of (round, wave, lane) holds that lane's scale byte
//         in the four steps wave `wave` multiplies in that round.  A wave's load is ONE contiguous 256-byte span per round; the steps of a
//         partial last round that do not exist hold padding bytes, which nothing multiplies.
//
// mx_rw_kernel: a workgroup owns ONE row block and reads it once, for every M <= 64: 8 waves split K as mx_small_kernel's do, each B
// fragment is multiplied against all kF = ceil(M / 16) A fragments (up to four accumulator quads per wave).  mx_small_kernel fetches the same
// step as 16 half-lines of 16 different weight rows plus 16 scale dwords of 16 different lines, and for M > 16 its grid re-reads the
// weight ceil(M / 16) times.  The activations keep their row-major form and are read from global memory, a fragment per lane and step
// (they are small, shared by every workgroup and stay in L2).
//
// Every (m, n) sum is mx_small_kernel's, bit for bit: wave w takes the steps s = w (mod 8) in ascending order, one MFMA per step into
// one accumulator; the eight partial sums are added w = 0 .. 7; then the shared epilogue (gemm_mx_common.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_common.hpp"

namespace arcq {

constexpr int kMxRwFrags = kMxSmallM / 16;                      // A fragments of 16 rows
constexpr int kMxRwUnroll = 4;                                  // steps of loads in flight per wave = the bytes of an MRSF dword
constexpr int kMxRwRound = kMxSmallWaves * kMxRwUnroll;         // steps of one MRSF round
constexpr int kMxRwTileBytes = 1024;
constexpr int kMxRwRoundSfBytes = kMxSmallWaves * 256;

int64_t gemm_mx_repacked_w_bytes(int64_t N, int64_t Kp) { return (N <= 0 || Kp <= 0 || (N % 16) || (Kp % 128)) ? 0 : N * (Kp / 2); }
int64_t gemm_mx_repacked_sf_bytes(int64_t N, int64_t Kp) {
  if (N <= 0 || Kp <= 0 || (N % 16) || (Kp % 128)) return 0;
  return (N / 16) * ((Kp / 128 + kMxRwRound - 1) / kMxRwRound) * kMxRwRoundSfBytes;
}
int gemm_mx_repacked_supported(int64_t M, int64_t N, int64_t Kp) {
  return M >= 1 && M <= kMxSmallM && N > 0 && Kp > 0 && (N % 16) == 0 && (Kp % 128) == 0;
}

// kF = ceil(M / 16): the A fragments a launch multiplies, a template parameter so that M <= 16 carries one accumulator quad and the
// registers of one fragment per step in flight, not four
template <int kEpi, int kF>
__global__ __launch_bounds__(64 * kMxSmallWaves, 4) void mx_rw_kernel(MxArgs p) {   // 4 waves per SIMD = two workgroups per CU: <= 128 VGPRs
  __shared__ __attribute__((aligned(16))) float part[kMxSmallWaves][kF][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7, rounds = (steps + kMxRwRound - 1) / kMxRwRound;
  const int r16 = lane & 15, q = lane >> 4;
  // every address below is inside its operand: steps are clamped to steps - 1, rows to M - 1, and the MRSF dword of a partial round exists
  // (the array is padded to whole rounds)
  const uint8_t* gW = p.B + (size_t)blockIdx.x * (size_t)steps * kMxRwTileBytes + (size_t)lane * 16;
  const uint8_t* gSW = p.SFB + ((size_t)blockIdx.x * (size_t)rounds * kMxSmallWaves + (size_t)wave) * 256 + (size_t)lane * 4;
  const uint8_t* gA[kF];
  const uint8_t* gSA[kF];
#pragma unroll
  for (int f = 0; f < kF; ++f) {
    const size_t m = (size_t)min(16 * f + r16, p.M - 1);
    gA[f] = p.A + m * rowb + q * 16;
    gSA[f] = p.SFA + m * rows;
  }
  const int sh = 8 * q;
  f32x4 acc[kF];
#pragma unroll
  for (int f = 0; f < kF; ++f) acc[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave, round = 0; s0 < steps; s0 += kMxRwRound, ++round) {
    i32x4 a[kMxRwUnroll][kF], b[kMxRwUnroll];
    uint32_t sa[kMxRwUnroll][kF];
    const uint32_t sb = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSW + (size_t)round * kMxRwRoundSfBytes));
#pragma unroll
    for (int u = 0; u < kMxRwUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMAs of a step past the end are skipped
      b[u] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gW + (size_t)s * kMxRwTileBytes));
#pragma unroll
      for (int f = 0; f < kF; ++f) {
        a[u][f] = *reinterpret_cast<const i32x4*>(gA[f] + (size_t)s * 64);
        sa[u][f] = *reinterpret_cast<const uint32_t*>(gSA[f] + (size_t)s * 4);
      }
    }
#pragma unroll
    for (int u = 0; u < kMxRwUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps) {
#pragma unroll
        for (int f = 0; f < kF; ++f)
          acc[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u][f]), frag(b[u]), acc[f], 4, 4, 0, (int)(sa[u][f] >> sh), 0,
                                                                    (int)(sb >> (8 * u)));
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

template <int kEpi>
static int mx_rw_launch(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
                        float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, const char* who,
                        hipStream_t stream) {
  if (!gemm_mx_repacked_supported(M, N, Kp))
    return fail(ARCQ_ERR_SHAPE, "%s: need 1 <= M <= %d, N %% 16 == 0 and K %% 128 == 0 (M=%lld N=%lld K=%lld)", who, kMxSmallM, (long long)M, (long long)N,
                (long long)Kp);
  MxArgs p;
  p.A = A; p.B = MRW; p.SFA = SFA; p.SFB = MRSF; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  const dim3 grid((unsigned)(N / 16)), block(64 * kMxSmallWaves);
  switch ((M + 15) / 16) {
    case 1: return launch_kernel<mx_rw_kernel<kEpi, 1>>(grid, block, 0, stream, who, p);
    case 2: return launch_kernel<mx_rw_kernel<kEpi, 2>>(grid, block, 0, stream, who, p);
    case 3: return launch_kernel<mx_rw_kernel<kEpi, 3>>(grid, block, 0, stream, who, p);
    default: return launch_kernel<mx_rw_kernel<kEpi, kMxRwFrags>>(grid, block, 0, stream, who, p);
  }
}

int gemm_mx_repacked(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
                     float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream) {
  return mx_rw_launch<kEpiPlain>(A, MRW, SFA, MRSF, D, M, N, Kp, alpha_host, alpha_dev, bias, residual, out_dtype, "arcq_gemm_mxfp4_repacked", stream);
}

// ACT = bf16 [M, N/2]; the same contraction and accumulation order as gemm_mx_repacked
int gemm_mx_repacked_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N,
                              int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream) {
  return mx_rw_launch<kEpiSiluMul>(A, MRW, SFA, MRSF, ACT, M, N, Kp, alpha_host, alpha_dev, bias, nullptr, ARCQ_OUT_BF16,
                                   "arcq_gemm_mxfp4_repacked_silu_mul", stream);
}

}  // namespace arcq
