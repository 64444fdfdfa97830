// extern "C" entry points of the MXFP4 path (declared in include/arcq.h): layout helpers and argument validation.  Every
// shape, NULL and alignment check runs before the first HIP call.
#include <hip/hip_runtime.h>

#include "arcq_internal.hpp"

using namespace arcq;

extern "C" {

int64_t arcq_mx_k_padded(int64_t K) { return K <= 0 ? 0 : (K + 127) / 128 * 128; }
int64_t arcq_mx_sf_bytes(int64_t rows, int64_t K) { return rows <= 0 ? 0 : rows * (arcq_mx_k_padded(K) / 32); }

int arcq_mx_quantize_x(const void* X, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE,
                       void* stream) {
  return mx_quantize_x(X, reorder_index, QX, SFX, M, KQ, KE, (hipStream_t)stream);
}

int arcq_mx_quantize_w(const void* W, const int16_t* reorder_index, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE,
                       void* stream) {
  return mx_quantize_w(W, reorder_index, QW, SFW, N, KQ, KE, (hipStream_t)stream);
}

int arcq_gemm_mxfp4(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t K,
                    float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  (void)workspace;
  (void)workspace_bytes;
  GemmRule r{"arcq_gemm_mxfp4"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = (int64_t)65535 * 128; r.epi_align = 2;
  const int rc = gemm_checks(r, A, B, SFA, SFB, D, nullptr, M, N, K, bias, residual, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx(A, B, SFA, SFB, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, (hipStream_t)stream);
}

int arcq_mx_rmsnorm_quantize_x(const void* X, const void* Wn, float eps, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, int64_t M,
                               int64_t KQ, int64_t KE, void* stream) {
  return mx_rmsnorm_quantize_x(X, Wn, eps, reorder_index, QX, SFX, M, KQ, KE, (hipStream_t)stream);
}

int arcq_mx_silu_mul_quantize_x(const void* GU, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE,
                                int layout, void* stream) {
  return mx_silu_mul_quantize_x(GU, reorder_index, QX, SFX, M, KQ, KE, layout, (hipStream_t)stream);
}

int arcq_gemm_mxfp4_silu_mul(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* ACT, int64_t M, int64_t N, int64_t K,
                             float alpha_host, const float* alpha_dev, const void* bias, void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_silu_mul"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = (int64_t)65535 * 128; r.epi_align = 2; r.d = "ACT";
  const int rc = gemm_checks(r, A, B, SFA, SFB, ACT, nullptr, M, N, K, bias, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_silu_mul(A, B, SFA, SFB, ACT, M, N, K, alpha_host, alpha_dev, bias, (hipStream_t)stream);
}

int arcq_gemm_mxfp4_silu_mul_quantize(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, uint8_t* QACT, uint8_t* SFACT,
                                      int64_t M, int64_t N, int64_t K, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE,
                                      void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_silu_mul_quantize"};
  r.k_mult = 128; r.n_mult = 128; r.max_m = (int64_t)65535 * 128; r.epi_align = 2; r.d = "QACT";
  // the quantiser's own shape rules on KQ2 = N / 2 (arcq_mx_quantize_x), reported with the divisibility rules
  if (N >= 0 && (N % 128 == 0) && (KE < 0 || (KE % 64) || KE > N / 2 || N / 2 > 32767))
    return fail(ARCQ_ERR_SHAPE, "%s: need KE %% 64 == 0 and 0 <= KE <= N/2 <= 32767 (N=%lld KE=%lld)", r.who, (long long)N, (long long)KE);
  // a NULL SFACT is reported where gemm_checks reports a NULL output; the scale bytes need no alignment
  const int rc = gemm_checks(r, A, B, SFA, SFB, SFACT ? QACT : nullptr, nullptr, M, N, K, bias, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_silu_mul_quantize(A, B, SFA, SFB, QACT, SFACT, M, N, K, alpha_host, alpha_dev, bias, KE, (hipStream_t)stream);
}

int64_t arcq_mx_repacked_w_bytes(int64_t N, int64_t K) { return gemm_mx_repacked_w_bytes(N, K); }
int64_t arcq_mx_repacked_sf_bytes(int64_t N, int64_t K) { return gemm_mx_repacked_sf_bytes(N, K); }
int arcq_gemm_mxfp4_repacked_supported(int64_t M, int64_t N, int64_t K) { return gemm_mx_repacked_supported(M, N, K); }

// M beyond the decode kernel is reported once the divisibility rules hold, ahead of out_dtype; everything else is gemm_checks' order
static int mx_repacked_max_m(const GemmRule& r, int64_t M, int64_t N, int64_t K) {
  if (M > r.max_m && N >= 0 && K > 0 && (K % r.k_mult) == 0 && (N % r.n_mult) == 0)
    return fail(ARCQ_ERR_SHAPE, "%s: need M <= %lld over the repacked weight (M=%lld)", r.who, (long long)r.max_m, (long long)M);
  return ARCQ_OK;
}

int arcq_gemm_mxfp4_repacked(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t K,
                             float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_repacked"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = 64; r.epi_align = 2; r.b = "MRW"; r.sfb = "MRSF";
  if (int rc = mx_repacked_max_m(r, M, N, K)) return rc;
  const int rc = gemm_checks(r, A, MRW, SFA, MRSF, D, nullptr, M, N, K, bias, residual, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_repacked(A, MRW, SFA, MRSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, (hipStream_t)stream);
}

int arcq_gemm_mxfp4_repacked_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N,
                                      int64_t K, float alpha_host, const float* alpha_dev, const void* bias, void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_repacked_silu_mul"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = 64; r.epi_align = 2; r.b = "MRW"; r.sfb = "MRSF"; r.d = "ACT";
  if (int rc = mx_repacked_max_m(r, M, N, K)) return rc;
  const int rc = gemm_checks(r, A, MRW, SFA, MRSF, ACT, nullptr, M, N, K, bias, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_repacked_silu_mul(A, MRW, SFA, MRSF, ACT, M, N, K, alpha_host, alpha_dev, bias, (hipStream_t)stream);
}

// ---- every M over the repacked weight alone: the namesakes' rules and order, the weight operands named MRW / MRSF
int arcq_gemm_mxfp4_rw_route(int64_t M, int64_t N, int64_t K) { return gemm_mx_rw_route(M, N, K); }

int arcq_gemm_mxfp4_rw(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t K,
                       float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_rw"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = (int64_t)65535 * 128; r.epi_align = 2; r.b = "MRW"; r.sfb = "MRSF";
  const int rc = gemm_checks(r, A, MRW, SFA, MRSF, D, nullptr, M, N, K, bias, residual, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_rw(A, MRW, SFA, MRSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, (hipStream_t)stream);
}

int arcq_gemm_mxfp4_rw_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N,
                                int64_t K, float alpha_host, const float* alpha_dev, const void* bias, void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_rw_silu_mul"};
  r.k_mult = 128; r.n_mult = 16; r.max_m = (int64_t)65535 * 128; r.epi_align = 2; r.b = "MRW"; r.sfb = "MRSF"; r.d = "ACT";
  const int rc = gemm_checks(r, A, MRW, SFA, MRSF, ACT, nullptr, M, N, K, bias, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_rw_silu_mul(A, MRW, SFA, MRSF, ACT, M, N, K, alpha_host, alpha_dev, bias, (hipStream_t)stream);
}

int arcq_gemm_mxfp4_rw_silu_mul_quantize(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, uint8_t* QACT, uint8_t* SFACT,
                                         int64_t M, int64_t N, int64_t K, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE,
                                         void* stream) {
  GemmRule r{"arcq_gemm_mxfp4_rw_silu_mul_quantize"};
  r.k_mult = 128; r.n_mult = 128; r.max_m = (int64_t)65535 * 128; r.epi_align = 2; r.b = "MRW"; r.sfb = "MRSF"; r.d = "QACT";
  // the KE rule and the NULL SFACT: where arcq_gemm_mxfp4_silu_mul_quantize reports them
  if (N >= 0 && (N % 128 == 0) && (KE < 0 || (KE % 64) || KE > N / 2 || N / 2 > 32767))
    return fail(ARCQ_ERR_SHAPE, "%s: need KE %% 64 == 0 and 0 <= KE <= N/2 <= 32767 (N=%lld KE=%lld)", r.who, (long long)N, (long long)KE);
  const int rc = gemm_checks(r, A, MRW, SFA, MRSF, SFACT ? QACT : nullptr, nullptr, M, N, K, bias, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_rw_silu_mul_quantize(A, MRW, SFA, MRSF, QACT, SFACT, M, N, K, alpha_host, alpha_dev, bias, KE, (hipStream_t)stream);
}

// ---- MXFP4 fused decode linear (arcq.h): the quantiser's rules (quant_checks, family kQuantMxLinear) and the repacked GEMM's
// (gemm_checks, no_a) reported in ONE order -- every shape fault, out_dtype, empty, every NULL, unsupported, every alignment -- by
// running the two validators three times over stand-in operands that let one kind of fault through at a time: a valid aligned
// stand-in for every pointer (shape faults only), then one wherever the operand is not NULL (NULL faults only), then the operands.
// (An M or N beyond the parameter block's int is gemm_checks' "shape too large", ARCQ_ERR_UNSUPPORTED, in the first pass.)
static const void* const kMxLinStandIn = reinterpret_cast<const void*>(uintptr_t{256});
static const void* there(const void* p) { return p ? kMxLinStandIn : nullptr; }

static int mx_linear_checks(const char* who, int kind, bool silu, const void* X, const void* Wn, const int16_t* idx, const uint8_t* MRW, const uint8_t* MRSF,
                            void* D, int64_t M, int64_t N, int64_t KQ, int64_t KE, const void* bias, const void* residual, int out_dtype) {
  const bool rms = kind == ARCQ_SRC_RMSNORM;
  QuantRule q{who};
  q.family = kQuantMxLinear;
  if (rms) { q.extra = true; q.kq_min = 2048; q.kq_max = 8192; }
  GemmRule g{who};
  g.k_mult = 128; g.n_mult = 16; g.max_m = 0; g.epi_align = 2; g.b = "MRW"; g.sfb = "MRSF"; g.d = silu ? "ACT" : "D"; g.no_a = true;
  const void* const s = kMxLinStandIn;
  if (const int rc = quant_checks(q, QuantArgs{s, rms ? s : nullptr, s, nullptr, nullptr, M, KQ, KE}); rc < 0) return rc;   // (1: M == 0, N's rules still apply)
  const int64_t Kp = arcq_mx_k_padded(KQ + KE);
  if (const int rc = gemm_checks(g, nullptr, s, nullptr, s, s, nullptr, M, N, Kp, nullptr, nullptr, out_dtype)) return rc;   // 1: nothing to do
  if (const int rc = quant_checks(q, QuantArgs{there(X), rms ? there(Wn) : nullptr, there(idx), nullptr, nullptr, M, KQ, KE})) return rc;
  if (const int rc = gemm_checks(g, nullptr, there(MRW), nullptr, there(MRSF), there(D), nullptr, M, N, Kp, nullptr, nullptr, out_dtype)) return rc;
  if (!gemm_mx_linear_supported(kind, M, N, KQ, KE))
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: no fused kernel for this shape: need 1 <= M <= 16 and %lld <= %d bytes of LDS (M=%lld N=%lld KQ=%lld KE=%lld)",
                who, (long long)gemm_mx_linear_lds_bytes(kind, KQ, KE), 81920, (long long)M, (long long)N, (long long)KQ, (long long)KE);
  if (const int rc = quant_checks(q, QuantArgs{X, rms ? Wn : nullptr, idx, nullptr, nullptr, M, KQ, KE})) return rc;
  return gemm_checks(g, nullptr, MRW, nullptr, MRSF, D, nullptr, M, N, Kp, bias, residual, out_dtype);
}

int arcq_mx_linear_fused_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE) { return gemm_mx_linear_supported(kind, M, N, KQ, KE); }
int64_t arcq_mx_linear_fused_workgroups(int kind, int64_t N, int64_t KQ, int64_t KE) { return gemm_mx_linear_workgroups(kind, N, KQ, KE); }
int64_t arcq_mx_linear_fused_lds_bytes(int kind, int64_t KQ, int64_t KE) {
  return (KQ <= 0 || KE < 0 || KQ > 32767 || KE > KQ) ? 0 : gemm_mx_linear_lds_bytes(kind, KQ, KE);
}

int arcq_mx_linear_rmsnorm_repacked(const void* X, const void* Wn, float eps, const int16_t* reorder_index, const uint8_t* MRW, const uint8_t* MRSF,
                                    void* D, int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host, const float* alpha_dev, const void* bias,
                                    const void* residual, int out_dtype, void* stream) {
  const char* who = "arcq_mx_linear_rmsnorm_repacked";
  if (const int rc = mx_linear_checks(who, ARCQ_SRC_RMSNORM, false, X, Wn, reorder_index, MRW, MRSF, D, M, N, KQ, KE, bias, residual, out_dtype))
    return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_linear(ARCQ_SRC_RMSNORM, false, X, Wn, eps, reorder_index, MRW, MRSF, D, M, N, KQ, KE, alpha_host, alpha_dev, bias, residual, out_dtype,
                        who, (hipStream_t)stream);
}

int arcq_mx_linear_rmsnorm_silu_repacked(const void* X, const void* Wn, float eps, const int16_t* reorder_index, const uint8_t* MRW, const uint8_t* MRSF,
                                         void* ACT, int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host, const float* alpha_dev,
                                         const void* bias, void* stream) {
  const char* who = "arcq_mx_linear_rmsnorm_silu_repacked";
  if (const int rc = mx_linear_checks(who, ARCQ_SRC_RMSNORM, true, X, Wn, reorder_index, MRW, MRSF, ACT, M, N, KQ, KE, bias, nullptr, ARCQ_OUT_BF16))
    return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_linear(ARCQ_SRC_RMSNORM, true, X, Wn, eps, reorder_index, MRW, MRSF, ACT, M, N, KQ, KE, alpha_host, alpha_dev, bias, nullptr,
                        ARCQ_OUT_BF16, who, (hipStream_t)stream);
}

int arcq_mx_linear_quantize_repacked(const void* X, const int16_t* reorder_index, const uint8_t* MRW, const uint8_t* MRSF, void* D, int64_t M, int64_t N,
                                     int64_t KQ, int64_t KE, float alpha_host, const float* alpha_dev, const void* bias, const void* residual,
                                     int out_dtype, void* stream) {
  const char* who = "arcq_mx_linear_quantize_repacked";
  if (const int rc = mx_linear_checks(who, ARCQ_SRC_PLAIN, false, X, nullptr, reorder_index, MRW, MRSF, D, M, N, KQ, KE, bias, residual, out_dtype))
    return rc < 0 ? rc : ARCQ_OK;
  return gemm_mx_linear(ARCQ_SRC_PLAIN, false, X, nullptr, 0.0f, reorder_index, MRW, MRSF, D, M, N, KQ, KE, alpha_host, alpha_dev, bias, residual,
                        out_dtype, who, (hipStream_t)stream);
}

}  // extern "C"
