// extern "C" entry points of the paged KV cache (declared in include/arcq_kv.h): argument validation.  Every shape, NULL and
// alignment check runs before the first HIP call; the contents of the index tensors are the caller's contract (arcq_kv.h).
#include <hip/hip_runtime.h>

#include "../../include/arcq_kv.h"
#include "arcq_internal.hpp"

using namespace arcq;

namespace {

constexpr int64_t kMaxDim = INT32_MAX / 2;

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the geometry every entry point shares; returns ARCQ_OK to go on
int geometry(const char* who, int64_t B, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format) {
  if (format != ARCQ_KV_INT4 && format != ARCQ_KV_16BIT) return fail(ARCQ_ERR_SHAPE, "%s: format must be ARCQ_KV_INT4 or ARCQ_KV_16BIT, got %d", who, format);
  if (B < 0 || L <= 0 || N <= 0 || P <= 0 || B > kMaxDim || L > kMaxDim || N > 65535 || P > kMaxDim)
    return fail(ARCQ_ERR_SHAPE, "%s: need B >= 0, L >= 1, 1 <= N <= 65535, P >= 1 (B=%lld L=%lld N=%lld P=%lld)", who, (long long)B, (long long)L,
                (long long)N, (long long)P);
  if (layer_idx < 0 || layer_idx >= L) return fail(ARCQ_ERR_SHAPE, "%s: layer_idx=%lld is not a layer of L=%lld", who, (long long)layer_idx, (long long)L);
  return ARCQ_OK;
}

int dtype_ok(const char* who, int dtype) {
  if (dtype != ARCQ_KV_F16 && dtype != ARCQ_KV_BF16) return fail(ARCQ_ERR_SHAPE, "%s: dtype must be ARCQ_KV_F16 or ARCQ_KV_BF16, got %d", who, dtype);
  return ARCQ_OK;
}

int write_call(const char* who, KvWriteArgs& a, bool init, void* stream) {
  int rc = geometry(who, a.B, a.L, a.layer, a.N, a.P, a.format);
  if (rc != ARCQ_OK) return rc;
  if (a.quantize && (rc = dtype_ok(who, a.dtype)) != ARCQ_OK) return rc;
  if (a.ntok < 0 || a.ntok > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: ntok=%lld is out of range", who, (long long)a.ntok);
  if (a.quantize && a.format != ARCQ_KV_INT4) return fail(ARCQ_ERR_UNSUPPORTED, "%s: the quantiser writes ARCQ_KV_INT4 caches only", who);
  if (a.B == 0 || a.ntok == 0) return ARCQ_OK;
  if (!a.kv_data || !a.kv_param || !a.kv_indptr || !a.kv_indices || !a.last_page_offset || !a.k || !a.v || (init && !a.seqlen_indptr) ||
      (!a.quantize && (!a.k_param || !a.v_param)))
    return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(a.kv_data, 16) || misaligned(a.k, 16) || misaligned(a.v, 16)) return fail(ARCQ_ERR_SHAPE, "%s: kv_data, k and v must be 16-byte aligned", who);
  if (misaligned(a.kv_param, 4) || misaligned(a.kv_indptr, 4) || misaligned(a.kv_indices, 4) || misaligned(a.last_page_offset, 4) ||
      misaligned(a.seqlen_indptr, 4) || misaligned(a.k_param, 4) || misaligned(a.v_param, 4))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_param, k_param, v_param and the index tensors must be 4-byte aligned", who);
  return kv_write(a, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int arcq_kv_init(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset, const void* k,
                 const void* v, const void* k_param, const void* v_param, const int32_t* seqlen_indptr, int64_t ntok, int64_t B, int64_t L,
                 int64_t layer_idx, int64_t N, int64_t P, int format, void* stream) {
  KvWriteArgs a{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, ntok, B, L, layer_idx, N, P,
                format, 0, false};
  return write_call("arcq_kv_init", a, true, stream);
}

int arcq_kv_append(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset, const void* k,
                   const void* v, const void* k_param, const void* v_param, int64_t B, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format,
                   void* stream) {
  KvWriteArgs a{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, nullptr, B, B, L, layer_idx, N, P, format, 0,
                false};
  return write_call("arcq_kv_append", a, false, stream);
}

int arcq_kv_append_quantize(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset,
                            const void* k, const void* v, int64_t B, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format, int dtype,
                            void* stream) {
  KvWriteArgs a{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, nullptr, nullptr, nullptr, B, B, L, layer_idx, N, P, format, dtype,
                true};
  return write_call("arcq_kv_append_quantize", a, false, stream);
}

int arcq_kv_init_quantize(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset,
                          const void* k, const void* v, const int32_t* seqlen_indptr, int64_t ntok, int64_t B, int64_t L, int64_t layer_idx, int64_t N,
                          int64_t P, int format, int dtype, void* stream) {
  KvWriteArgs a{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, nullptr, nullptr, seqlen_indptr, ntok, B, L, layer_idx, N, P, format,
                dtype, true};
  return write_call("arcq_kv_init_quantize", a, true, stream);
}

int64_t arcq_kv_decode_workspace_bytes(int64_t B, int64_t Nq, int64_t N, int64_t nnz, int64_t P) {
  if (B <= 0 || Nq <= 0 || N <= 0 || Nq % N) return 0;
  const int64_t S = kv_decode_splits(B, Nq, N, nnz, P);
  return S <= 1 ? 0 : B * Nq * S * 130 * (int64_t)sizeof(float);
}

int arcq_kv_batch_decode(void* o, const void* q, const void* kv_data, const void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices,
                         const int32_t* last_page_offset, int64_t B, int64_t Nq, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int64_t nnz,
                         int format, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "arcq_kv_batch_decode";
  int rc = geometry(who, B, L, layer_idx, N, P, format);
  if (rc != ARCQ_OK) return rc;
  if ((rc = dtype_ok(who, dtype)) != ARCQ_OK) return rc;
  if (Nq <= 0 || Nq % N || Nq > 65535)
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (at most 65535)", who, (long long)Nq, (long long)N);
  if (nnz < 0 || nnz > kMaxDim || nnz * P > INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: nnz=%lld pages of P=%lld entries are out of range", who, (long long)nnz, (long long)P);
  if (B * Nq > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: B * Nq = %lld is out of range", who, (long long)(B * Nq));
  if (B == 0) return ARCQ_OK;
  if (!o || !q || !kv_data || !kv_indptr || !kv_indices || !last_page_offset || (format == ARCQ_KV_INT4 && !kv_param))
    return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(o, 16) || misaligned(q, 16) || misaligned(kv_data, 16)) return fail(ARCQ_ERR_SHAPE, "%s: o, q and kv_data must be 16-byte aligned", who);
  if (misaligned(kv_param, 4) || misaligned(kv_indptr, 4) || misaligned(kv_indices, 4) || misaligned(last_page_offset, 4) || misaligned(workspace, 4))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_param, the index tensors and the workspace must be 4-byte aligned", who);
  const int64_t need = arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return fail(ARCQ_ERR_WORKSPACE, "%s: workspace of %lld bytes, need %lld (arcq_kv_decode_workspace_bytes)", who, (long long)workspace_bytes, (long long)need);
  KvDecodeArgs a{o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, B, Nq, L, layer_idx, N, P, nnz, format, dtype, workspace};
  return kv_decode(a, (hipStream_t)stream);
}

int arcq_kv_batch_prefill(void* o, const void* q, const int32_t* qo_indptr, const void* kv_data, const void* kv_param, const int32_t* kv_indptr,
                          const int32_t* kv_indices, const int32_t* last_page_offset, int64_t ntok, int64_t B, int64_t Nq, int64_t L, int64_t layer_idx,
                          int64_t N, int64_t P, int64_t nnz, int format, int dtype, void* stream) {
  const char* who = "arcq_kv_batch_prefill";
  int rc = geometry(who, B, L, layer_idx, N, P, format);
  if (rc != ARCQ_OK) return rc;
  if ((rc = dtype_ok(who, dtype)) != ARCQ_OK) return rc;
  if (Nq <= 0 || Nq % N || Nq > 65535)
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (at most 65535)", who, (long long)Nq, (long long)N);
  if (nnz < 0 || nnz > kMaxDim || nnz * P > INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: nnz=%lld pages of P=%lld entries are out of range", who, (long long)nnz, (long long)P);
  if (ntok < 0 || ntok > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: ntok=%lld is out of range", who, (long long)ntok);
  if (format != ARCQ_KV_INT4) return fail(ARCQ_ERR_UNSUPPORTED, "%s: prefill attention reads ARCQ_KV_INT4 caches only", who);
  if (B == 0 || ntok == 0) return ARCQ_OK;
  if (!o || !q || !qo_indptr || !kv_data || !kv_param || !kv_indptr || !kv_indices || !last_page_offset) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(o, 16) || misaligned(q, 16) || misaligned(kv_data, 16)) return fail(ARCQ_ERR_SHAPE, "%s: o, q and kv_data must be 16-byte aligned", who);
  if (misaligned(kv_param, 4) || misaligned(qo_indptr, 4) || misaligned(kv_indptr, 4) || misaligned(kv_indices, 4) || misaligned(last_page_offset, 4))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_param and the index tensors must be 4-byte aligned", who);
  KvPrefillArgs a{o, q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, ntok, B, Nq, L, layer_idx, N, P, dtype};
  return kv_prefill(a, (hipStream_t)stream);
}

int64_t arcq_kv_decode_step_state_bytes(int64_t B, int64_t Nq, int64_t N) {
  if (B <= 0 || Nq <= 0 || N <= 0 || Nq % N) return 0;
  return B * N * kv_decode_chunks(Nq, N) * (int64_t)sizeof(int32_t);
}

int arcq_kv_decode_step(void* o, const void* q, const void* k, const void* v, int64_t q_stride, int64_t kv_stride, void* kv_data, void* kv_param,
                        const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset, int64_t B, int64_t Nq, int64_t L,
                        int64_t layer_idx, int64_t N, int64_t P, int64_t nnz, int format, int dtype, void* workspace, int64_t workspace_bytes,
                        void* state, int64_t state_bytes, void* stream) {
  const char* who = "arcq_kv_decode_step";
  int rc = geometry(who, B, L, layer_idx, N, P, format);
  if (rc != ARCQ_OK) return rc;
  if ((rc = dtype_ok(who, dtype)) != ARCQ_OK) return rc;
  if (Nq <= 0 || Nq % N || Nq > 65535)
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (at most 65535)", who, (long long)Nq, (long long)N);
  if (nnz < 0 || nnz > kMaxDim || nnz * P > INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: nnz=%lld pages of P=%lld entries are out of range", who, (long long)nnz, (long long)P);
  if (B * Nq > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: B * Nq = %lld is out of range", who, (long long)(B * Nq));
  if (format != ARCQ_KV_INT4) return fail(ARCQ_ERR_UNSUPPORTED, "%s: the decode step quantises into ARCQ_KV_INT4 caches only", who);
  if (q_stride < Nq * 128 || kv_stride < N * 128 || q_stride % 8 || kv_stride % 8 || q_stride > kMaxDim || kv_stride > kMaxDim)
    return fail(ARCQ_ERR_SHAPE, "%s: q_stride=%lld >= Nq * 128 = %lld and kv_stride=%lld >= N * 128 = %lld must be multiples of 8 elements", who,
                (long long)q_stride, (long long)(Nq * 128), (long long)kv_stride, (long long)(N * 128));
  if (B == 0) return ARCQ_OK;
  if (!o || !q || !k || !v || !kv_data || !kv_param || !kv_indptr || !kv_indices || !last_page_offset) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(o, 16) || misaligned(q, 16) || misaligned(k, 16) || misaligned(v, 16) || misaligned(kv_data, 16))
    return fail(ARCQ_ERR_SHAPE, "%s: o, q, k, v and kv_data must be 16-byte aligned", who);
  if (misaligned(kv_param, 4) || misaligned(kv_indptr, 4) || misaligned(kv_indices, 4) || misaligned(last_page_offset, 4) || misaligned(workspace, 4) ||
      misaligned(state, 4))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_param, the index tensors, the workspace and the state must be 4-byte aligned", who);
  const int64_t need = arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P);
  if (need > 0 && (!workspace || workspace_bytes < need))
    return fail(ARCQ_ERR_WORKSPACE, "%s: workspace of %lld bytes, need %lld (arcq_kv_decode_workspace_bytes)", who, (long long)workspace_bytes, (long long)need);
  const int64_t need_state = arcq_kv_decode_step_state_bytes(B, Nq, N);
  if (need > 0 && (!state || state_bytes < need_state))
    return fail(ARCQ_ERR_WORKSPACE, "%s: state of %lld bytes, need %lld (arcq_kv_decode_step_state_bytes)", who, (long long)state_bytes, (long long)need_state);
  KvDecodeArgs a{o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, B, Nq, L, layer_idx, N, P, nnz, format, dtype, workspace};
  KvStepArgs st{k, v, q_stride, kv_stride, state};
  return kv_decode_step(a, st, (hipStream_t)stream);
}

}  // extern "C"
