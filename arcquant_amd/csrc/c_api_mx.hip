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
  const char* who = "arcq_gemm_mxfp4";
  (void)workspace;
  (void)workspace_bytes;
  if (M < 0 || N < 0 || K <= 0 || (K % 128) || (N % 16))
    return fail(ARCQ_ERR_SHAPE, "%s: need M,N >= 0, K %% 128 == 0 and N %% 16 == 0 (M=%lld N=%lld K=%lld)", who, (long long)M, (long long)N,
                (long long)K);
  if (out_dtype != ARCQ_OUT_BF16 && out_dtype != ARCQ_OUT_F32) return fail(ARCQ_ERR_SHAPE, "%s: bad out_dtype %d", who, out_dtype);
  if (M == 0 || N == 0) return ARCQ_OK;
  if (!A || !B || !SFA || !SFB || !D) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (M > (int64_t)65535 * 128 || N > INT32_MAX / 2 || K > INT32_MAX / 2 || M * N > ((int64_t)1 << 40))
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: shape too large", who);
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(D)) & 15)
    return fail(ARCQ_ERR_SHAPE, "%s: A, B and D must be 16-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(SFA) | reinterpret_cast<uintptr_t>(SFB)) & 3)
    return fail(ARCQ_ERR_SHAPE, "%s: SFA and SFB must be 4-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(residual)) & 1)
    return fail(ARCQ_ERR_SHAPE, "%s: bias and residual must be 2-byte aligned", who);
  return gemm_mx(A, B, SFA, SFB, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, (hipStream_t)stream);
}

}  // extern "C"
