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

// a contiguous [ntok, heads, 128] result and a strided source of the same rows: the same tensor, or apart
bool overlaps(const void* out, const void* in, int64_t ntok, int64_t heads, int64_t in_stride) {
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(ntok * heads * 256);
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + (uintptr_t)(((ntok - 1) * in_stride + heads * 128) * 2);
  return o0 < i1 && i0 < o1;
}

int rope_write_call(const char* who, KvRopeArgs& a, bool init, int64_t rope_len, void* stream) {
  KvWriteArgs& w = a.w;
  int rc = geometry(who, w.B, w.L, w.layer, w.N, w.P, w.format);
  if (rc != ARCQ_OK) return rc;
  if ((rc = dtype_ok(who, w.dtype)) != ARCQ_OK) return rc;
  if (w.ntok < 0 || w.ntok > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: ntok=%lld is out of range", who, (long long)w.ntok);
  if (a.Nq <= 0 || a.Nq % w.N || a.Nq > 65535)
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (at most 65535)", who, (long long)a.Nq, (long long)w.N);
  if (w.format != ARCQ_KV_INT4) return fail(ARCQ_ERR_UNSUPPORTED, "%s: the quantiser writes ARCQ_KV_INT4 caches only", who);
  if (rope_len < 1 || rope_len > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: rope_len=%lld must be at least 1", who, (long long)rope_len);
  if (a.q_stride < a.Nq * 128 || a.kv_stride < w.N * 128 || a.q_stride % 8 || a.kv_stride % 8 || a.q_stride > kMaxDim || a.kv_stride > kMaxDim)
    return fail(ARCQ_ERR_SHAPE, "%s: q_stride=%lld >= Nq * 128 = %lld and kv_stride=%lld >= N * 128 = %lld must be multiples of 8 elements", who,
                (long long)a.q_stride, (long long)(a.Nq * 128), (long long)a.kv_stride, (long long)(w.N * 128));
  if (w.ntok * (a.Nq + 2 * w.N) > 16 * (int64_t)INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: ntok * (Nq + 2 N) rows are out of range", who);
  if (w.B == 0 || w.ntok == 0) return ARCQ_OK;
  if (!w.kv_data || !w.kv_param || !w.kv_indptr || !w.kv_indices || !w.last_page_offset || !w.k || !w.v || (init && !w.seqlen_indptr) || !a.q_out ||
      !a.q || !a.cos || !a.sin)
    return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(w.kv_data, 16) || misaligned(w.k, 16) || misaligned(w.v, 16) || misaligned(a.q, 16) || misaligned(a.q_out, 16) ||
      misaligned(a.cos, 16) || misaligned(a.sin, 16))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_data, q_out, q, k, v, cos and sin must be 16-byte aligned", who);
  if (misaligned(w.kv_param, 4) || misaligned(w.kv_indptr, 4) || misaligned(w.kv_indices, 4) || misaligned(w.last_page_offset, 4) ||
      misaligned(w.seqlen_indptr, 4))
    return fail(ARCQ_ERR_SHAPE, "%s: kv_param and the index tensors must be 4-byte aligned", who);
  if (overlaps(a.q_out, a.q, w.ntok, a.Nq, a.q_stride) && !(a.q_out == a.q && (a.q_stride == a.Nq * 128 || w.ntok == 1)))
    return fail(ARCQ_ERR_SHAPE, "%s: q_out must be q itself (q contiguous) or must not overlap it", who);
  a.who = who;
  return kv_rope_write(a, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int arcq_rope_qk(void* q, void* k, int64_t q_stride, int64_t k_stride, const int32_t* positions, int64_t n_pos, const void* cos, const void* sin,
                 int64_t rope_len, int64_t ntok, int64_t Nq, int64_t N, int dtype, void* stream) {
  const char* who = "arcq_rope_qk";
  int rc = dtype_ok(who, dtype);
  if (rc != ARCQ_OK) return rc;
  if (ntok < 0 || ntok > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: ntok=%lld is out of range", who, (long long)ntok);
  if (Nq <= 0 || Nq > 65535 || N < 0 || N > 65535 || (N > 0 && Nq % N))
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (N = 0: no k; at most 65535 each)", who, (long long)Nq, (long long)N);
  if (rope_len < 1 || rope_len > kMaxDim) return fail(ARCQ_ERR_SHAPE, "%s: rope_len=%lld must be at least 1", who, (long long)rope_len);
  if (n_pos < 1 || n_pos > kMaxDim || ntok % n_pos)
    return fail(ARCQ_ERR_SHAPE, "%s: n_pos=%lld must be at least 1 and divide ntok=%lld", who, (long long)n_pos, (long long)ntok);
  if (q_stride < Nq * 128 || q_stride % 8 || q_stride > kMaxDim || (N > 0 && (k_stride < N * 128 || k_stride % 8 || k_stride > kMaxDim)))
    return fail(ARCQ_ERR_SHAPE, "%s: q_stride=%lld >= Nq * 128 = %lld and k_stride=%lld >= N * 128 = %lld must be multiples of 8 elements", who,
                (long long)q_stride, (long long)(Nq * 128), (long long)k_stride, (long long)(N * 128));
  if (ntok * (Nq + N) > 16 * (int64_t)INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: ntok * (Nq + N) rows are out of range", who);
  if (ntok == 0) return ARCQ_OK;
  if (!q || (N > 0 && !k) || !positions || !cos || !sin) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (misaligned(q, 16) || (N > 0 && misaligned(k, 16)) || misaligned(cos, 16) || misaligned(sin, 16))
    return fail(ARCQ_ERR_SHAPE, "%s: q, k, cos and sin must be 16-byte aligned", who);
  if (misaligned(positions, 4)) return fail(ARCQ_ERR_SHAPE, "%s: positions must be 4-byte aligned", who);
  RopeQkArgs a{q, N > 0 ? k : nullptr, positions, cos, sin, q_stride, k_stride, ntok, n_pos, Nq, N, dtype};
  return kv_rope_qk(a, (hipStream_t)stream);
}

int arcq_kv_rope_append_quantize(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset,
                                 void* q_out, const void* q, const void* k, const void* v, int64_t q_stride, int64_t kv_stride, const void* cos,
                                 const void* sin, int64_t rope_len, int64_t B, int64_t Nq, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format,
                                 int dtype, void* stream) {
  KvRopeArgs a{{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, nullptr, nullptr, nullptr, B, B, L, layer_idx, N, P, format, dtype, true},
               q_out, q, cos, sin, q_stride, kv_stride, Nq, nullptr};
  return rope_write_call("arcq_kv_rope_append_quantize", a, false, rope_len, stream);
}

int arcq_kv_rope_init_quantize(void* kv_data, void* kv_param, const int32_t* kv_indptr, const int32_t* kv_indices, const int32_t* last_page_offset,
                               void* q_out, const void* q, const void* k, const void* v, int64_t q_stride, int64_t kv_stride, const void* cos,
                               const void* sin, int64_t rope_len, const int32_t* seqlen_indptr, int64_t ntok, int64_t B, int64_t Nq, int64_t L,
                               int64_t layer_idx, int64_t N, int64_t P, int format, int dtype, void* stream) {
  KvRopeArgs a{{kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, nullptr, nullptr, seqlen_indptr, ntok, B, L, layer_idx, N, P, format, dtype,
                true},
               q_out, q, cos, sin, q_stride, kv_stride, Nq, nullptr};
  return rope_write_call("arcq_kv_rope_init_quantize", a, true, rope_len, stream);
}

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
