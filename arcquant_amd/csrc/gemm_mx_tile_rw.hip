// The tiled MXFP4 GEMM (M > kMxSmallM) over a weight repacked into MFMA operand order (arcq.h "MXFP4 repacked weight"): mx_tile_kernel
// of gemm_mx.hip -- 128 x 128 tiles, 4 waves, the 32x32x64 scaled fp4 MFMA, K steps of 128 through two LDS buffers, the three epilogues
// -- with its B operand staged from (MRW, MRSF) instead of (B, SFB).  The statements are gemm_mx_tile_body.inc under kRepackedB = true;
// what a step's compute() reads from LDS is byte for byte what mx_tile_kernel stages, so every result is arcq_gemm_mxfp4's,
// arcq_gemm_mxfp4_silu_mul's and arcq_gemm_mxfp4_silu_mul_quantize's on the un-repacked weight, bit for bit.  With it a layer that keeps
// ONLY the repacked copy serves every M.  In a translation unit of its own, so that gemm_mx.hip and gemm_mx_rw.hip compile what they
// compiled before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_tile_common.hpp"

namespace arcq {

template <int kEpi>
__global__ __launch_bounds__(256) void mx_tile_rw_kernel(MxArgs p) {
  constexpr bool kRepackedB = true;
#include "gemm_mx_tile_body.inc"
}

static int mx_tile_rw_launch(const MxArgs& p, int epilogue, const char* who, hipStream_t stream) {
  const dim3 grid((unsigned)((p.N + kMxTile - 1) / kMxTile), (unsigned)((p.M + kMxTile - 1) / kMxTile)), block(256);
  switch (epilogue) {
    case kEpiSiluMul: return launch_kernel<mx_tile_rw_kernel<kEpiSiluMul>>(grid, block, 0, stream, who, p);
    case kEpiSiluMulQuant: return launch_kernel<mx_tile_rw_kernel<kEpiSiluMulQuant>>(grid, block, 0, stream, who, p);
    default: return launch_kernel<mx_tile_rw_kernel<kEpiPlain>>(grid, block, 0, stream, who, p);
  }
}

// Which kernel serves a call over the repacked weight: 1 = the decode kernels of gemm_mx_rw.hip / gemm_mx_slice_rw.hip (M <= kMxSmallM),
// 2 = mx_tile_rw_kernel, 0 = no such shape
int gemm_mx_rw_route(int64_t M, int64_t N, int64_t Kp) {
  if (M < 1 || N <= 0 || Kp <= 0 || (N % 16) || (Kp % 128)) return 0;
  return M <= kMxSmallM ? 1 : 2;
}

static MxArgs mx_rw_args(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
                         float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype) {
  MxArgs p;
  p.A = A; p.B = MRW; p.SFA = SFA; p.SFB = MRSF; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return p;
}

// Any M >= 1 over (MRW, MRSF): the decode kernel up to kMxSmallM rows (the call IS gemm_mx_repacked), the tile kernel above
int gemm_mx_rw(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
               float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream) {
  if (M <= kMxSmallM) return gemm_mx_repacked(A, MRW, SFA, MRSF, D, M, N, Kp, alpha_host, alpha_dev, bias, residual, out_dtype, stream);
  return mx_tile_rw_launch(mx_rw_args(A, MRW, SFA, MRSF, D, M, N, Kp, alpha_host, alpha_dev, bias, residual, out_dtype), kEpiPlain,
                           "arcq_gemm_mxfp4_rw", stream);
}

int gemm_mx_rw_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N, int64_t Kp,
                        float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream) {
  if (M <= kMxSmallM) return gemm_mx_repacked_silu_mul(A, MRW, SFA, MRSF, ACT, M, N, Kp, alpha_host, alpha_dev, bias, stream);
  return mx_tile_rw_launch(mx_rw_args(A, MRW, SFA, MRSF, ACT, M, N, Kp, alpha_host, alpha_dev, bias, nullptr, ARCQ_OUT_BF16), kEpiSiluMul,
                           "arcq_gemm_mxfp4_rw_silu_mul", stream);
}

// (QACT, SFACT) as gemm_mx_silu_mul_quantize writes them; N % 128 == 0
int gemm_mx_rw_silu_mul_quantize(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, uint8_t* QACT, uint8_t* SFACT,
                                 int64_t M, int64_t N, int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE,
                                 hipStream_t stream) {
  MxArgs p = mx_rw_args(A, MRW, SFA, MRSF, nullptr, M, N, Kp, alpha_host, alpha_dev, bias, nullptr, ARCQ_OUT_BF16);
  p.QACT = QACT; p.SFACT = SFACT; p.KE = (int)KE;
  if (M <= kMxSmallM) return gemm_mx_slice_rw_quantize(p, "arcq_gemm_mxfp4_rw_silu_mul_quantize", stream);
  return mx_tile_rw_launch(p, kEpiSiluMulQuant, "arcq_gemm_mxfp4_rw_silu_mul_quantize", stream);
}

}  // namespace arcq
