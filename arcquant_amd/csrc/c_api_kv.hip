// extern "C" entry points of the paged KV cache (declared in include/arcq_kv.h): argument validation.  Every shape, NULL and
// alignment check runs before the first HIP call; the contents of the index tensors are the caller's contract (arcq_kv.h).  Each
// relation and each message is written once, as a named check below; the ORDER of the checks inside an entry point decides which of two
// faults a call reports, is part of the contract, and is recorded case by case in tests/golden/cabi_kv_rejections.json.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "../../include/arcq_kv.h"
#include "arcq_internal.hpp"

using namespace arcq;

namespace {

constexpr int64_t kMaxDim = INT32_MAX / 2;
constexpr const char* kQuantiserWrites = "the quantiser writes";

// Every check returns ARCQ_OK (0) to go on, so an entry point chains them with ||: the first that fails is the one reported.
// The geometry every entry point but arcq_rope_qk shares:
int geometry(const char* who, int64_t B, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format) {
  if (format != ARCQ_KV_INT4 && format != ARCQ_KV_16BIT) return fail(ARCQ_ERR_SHAPE, "%s: format must be ARCQ_KV_INT4 or ARCQ_KV_16BIT, got %d", who, format);
  if (B < 0 || L <= 0 || N <= 0 || P <= 0 || B > kMaxDim || L > kMaxDim || N > 65535 || P > kMaxDim)
    return fail(ARCQ_ERR_SHAPE, "%s: need B >= 0, L >= 1, 1 <= N <= 65535, P >= 1 (B=%lld L=%lld N=%lld P=%lld)", who, (long long)B, (long long)L,
                (long long)N, (long long)P);
  if (layer_idx < 0 || layer_idx >= L) return fail(ARCQ_ERR_SHAPE, "%s: layer_idx=%lld is not a layer of L=%lld", who, (long long)layer_idx, (long long)L);
  return ARCQ_OK;
}

// ---- the ranges and relations, each with its message
int dtype_ok(const char* who, int dtype) {
  return dtype != ARCQ_KV_F16 && dtype != ARCQ_KV_BF16 ? fail(ARCQ_ERR_SHAPE, "%s: dtype must be ARCQ_KV_F16 or ARCQ_KV_BF16, got %d", who, dtype) : ARCQ_OK;
}
int int4_only(const char* who, int format, const char* what) {          // what the entry point does with the cache: "the quantiser writes", ...
  return format != ARCQ_KV_INT4 ? fail(ARCQ_ERR_UNSUPPORTED, "%s: %s ARCQ_KV_INT4 caches only", who, what) : ARCQ_OK;
}
int heads_ok(const char* who, int64_t Nq, int64_t N) {                    // the query heads of a cache of N kv heads (geometry has checked N)
  if (Nq > 0 && Nq % N == 0 && Nq <= 65535) return ARCQ_OK;
  return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (at most 65535)", who, (long long)Nq, (long long)N);
}
int pages_ok(const char* who, int64_t nnz, int64_t P) {
  if (nnz >= 0 && nnz <= kMaxDim && nnz * P <= INT32_MAX) return ARCQ_OK;
  return fail(ARCQ_ERR_SHAPE, "%s: nnz=%lld pages of P=%lld entries are out of range", who, (long long)nnz, (long long)P);
}
int ntok_ok(const char* who, int64_t ntok) {
  return ntok < 0 || ntok > kMaxDim ? fail(ARCQ_ERR_SHAPE, "%s: ntok=%lld is out of range", who, (long long)ntok) : ARCQ_OK;
}
int rope_len_ok(const char* who, int64_t rope_len) {
  return rope_len < 1 || rope_len > kMaxDim ? fail(ARCQ_ERR_SHAPE, "%s: rope_len=%lld must be at least 1", who, (long long)rope_len) : ARCQ_OK;
}
int strides_ok(const char* who, int64_t q_stride, int64_t Nq, int64_t kv_stride, int64_t N) {      // token strides, in elements
  if (q_stride >= Nq * 128 && kv_stride >= N * 128 && q_stride % 8 == 0 && kv_stride % 8 == 0 && q_stride <= kMaxDim && kv_stride <= kMaxDim) return ARCQ_OK;
  return fail(ARCQ_ERR_SHAPE, "%s: q_stride=%lld >= Nq * 128 = %lld and kv_stride=%lld >= N * 128 = %lld must be multiples of 8 elements", who,
              (long long)q_stride, (long long)(Nq * 128), (long long)kv_stride, (long long)(N * 128));
}
int batch_heads_ok(const char* who, int64_t B, int64_t Nq) {
  return B * Nq > kMaxDim ? fail(ARCQ_ERR_SHAPE, "%s: B * Nq = %lld is out of range", who, (long long)(B * Nq)) : ARCQ_OK;
}
int workspace_ok(const char* who, const void* workspace, int64_t workspace_bytes, int64_t need) {  // the slices' records: none without slices
  if (need <= 0 || (workspace && workspace_bytes >= need)) return ARCQ_OK;
  return fail(ARCQ_ERR_WORKSPACE, "%s: workspace of %lld bytes, need %lld (arcq_kv_decode_workspace_bytes)", who, (long long)workspace_bytes, (long long)need);
}

// ---- pointer lists.  A pointer that a call does not need goes in as when(false, p): neither NULL nor misaligned.  NULL is aligned, so
// an optional pointer goes into the alignment lists as it is.  `names`: the entry point's own words for the list.
using Ptrs = std::initializer_list<const void*>;
alignas(16) const char kNotNeeded[16] = {};
const void* when(bool needed, const void* p) { return needed ? p : kNotNeeded; }
int none_null(const char* who, Ptrs ps) {
  for (const void* p : ps)
    if (!p) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  return ARCQ_OK;
}
bool any_misaligned(Ptrs ps, uintptr_t a) {
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) & (a - 1)) return true;
  return false;
}
int aligned16(const char* who, Ptrs ps, const char* names) {
  return any_misaligned(ps, 16) ? fail(ARCQ_ERR_SHAPE, "%s: %s must be 16-byte aligned", who, names) : ARCQ_OK;
}
int aligned4(const char* who, Ptrs ps, const char* names) {
  return any_misaligned(ps, 4) ? fail(ARCQ_ERR_SHAPE, "%s: %s must be 4-byte aligned", who, names) : ARCQ_OK;
}

int write_call(const char* who, KvWriteArgs& a, bool init, void* stream) {
  int rc;
  if ((rc = geometry(who, a.B, a.L, a.layer, a.N, a.P, a.format)) || (a.quantize && (rc = dtype_ok(who, a.dtype))) || (rc = ntok_ok(who, a.ntok)) ||
      (a.quantize && (rc = int4_only(who, a.format, kQuantiserWrites))))
    return rc;
  // the quantising writers launch one workgroup per 16 (token, K | V, head) rows (kv_write): the count must fit the grid
  if (a.quantize && a.ntok * 2 * a.N > 16 * (int64_t)INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: ntok * 2 N rows are out of range", who);
  if (a.B == 0 || a.ntok == 0) return ARCQ_OK;
  if ((rc = none_null(who, {a.kv_data, a.kv_param, a.kv_indptr, a.kv_indices, a.last_page_offset, a.k, a.v, when(init, a.seqlen_indptr),
                            when(!a.quantize, a.k_param), when(!a.quantize, a.v_param)})) ||
      (rc = aligned16(who, {a.kv_data, a.k, a.v}, "kv_data, k and v")) ||
      (rc = aligned4(who, {a.kv_param, a.kv_indptr, a.kv_indices, a.last_page_offset, a.seqlen_indptr, a.k_param, a.v_param},
                     "kv_param, k_param, v_param and the index tensors")))
    return rc;
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
  int rc;
  if ((rc = geometry(who, w.B, w.L, w.layer, w.N, w.P, w.format)) || (rc = dtype_ok(who, w.dtype)) || (rc = ntok_ok(who, w.ntok)) ||
      (rc = heads_ok(who, a.Nq, w.N)) || (rc = int4_only(who, w.format, kQuantiserWrites)) || (rc = rope_len_ok(who, rope_len)) ||
      (rc = strides_ok(who, a.q_stride, a.Nq, a.kv_stride, w.N)))
    return rc;
  if (w.ntok * (a.Nq + 2 * w.N) > 16 * (int64_t)INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: ntok * (Nq + 2 N) rows are out of range", who);
  if (w.B == 0 || w.ntok == 0) return ARCQ_OK;
  if ((rc = none_null(who, {w.kv_data, w.kv_param, w.kv_indptr, w.kv_indices, w.last_page_offset, w.k, w.v, when(init, w.seqlen_indptr), a.q_out, a.q,
                            a.cos, a.sin})) ||
      (rc = aligned16(who, {w.kv_data, w.k, w.v, a.q, a.q_out, a.cos, a.sin}, "kv_data, q_out, q, k, v, cos and sin")) ||
      (rc = aligned4(who, {w.kv_param, w.kv_indptr, w.kv_indices, w.last_page_offset, w.seqlen_indptr}, "kv_param and the index tensors")))
    return rc;
  if (overlaps(a.q_out, a.q, w.ntok, a.Nq, a.q_stride) && !(a.q_out == a.q && (a.q_stride == a.Nq * 128 || w.ntok == 1)))
    return fail(ARCQ_ERR_SHAPE, "%s: q_out must be q itself (q contiguous) or must not overlap it", who);
  a.who = who;
  return kv_rope_write(a, (hipStream_t)stream);
}

}  // namespace

extern "C" {

// (its head relation lets N = 0 through -- no k -- and its stride rule looks at k's only then: both stay its own)
int arcq_rope_qk(void* q, void* k, int64_t q_stride, int64_t k_stride, const int32_t* positions, int64_t n_pos, const void* cos, const void* sin,
                 int64_t rope_len, int64_t ntok, int64_t Nq, int64_t N, int dtype, void* stream) {
  const char* who = "arcq_rope_qk";
  int rc;
  if ((rc = dtype_ok(who, dtype)) || (rc = ntok_ok(who, ntok))) return rc;
  if (Nq <= 0 || Nq > 65535 || N < 0 || N > 65535 || (N > 0 && Nq % N))
    return fail(ARCQ_ERR_SHAPE, "%s: Nq=%lld must be a positive multiple of N=%lld (N = 0: no k; at most 65535 each)", who, (long long)Nq, (long long)N);
  if ((rc = rope_len_ok(who, rope_len))) return rc;
  if (n_pos < 1 || n_pos > kMaxDim || ntok % n_pos)
    return fail(ARCQ_ERR_SHAPE, "%s: n_pos=%lld must be at least 1 and divide ntok=%lld", who, (long long)n_pos, (long long)ntok);
  if (q_stride < Nq * 128 || q_stride % 8 || q_stride > kMaxDim || (N > 0 && (k_stride < N * 128 || k_stride % 8 || k_stride > kMaxDim)))
    return fail(ARCQ_ERR_SHAPE, "%s: q_stride=%lld >= Nq * 128 = %lld and k_stride=%lld >= N * 128 = %lld must be multiples of 8 elements", who,
                (long long)q_stride, (long long)(Nq * 128), (long long)k_stride, (long long)(N * 128));
  if (ntok * (Nq + N) > 16 * (int64_t)INT32_MAX) return fail(ARCQ_ERR_SHAPE, "%s: ntok * (Nq + N) rows are out of range", who);
  if (ntok == 0) return ARCQ_OK;
  if ((rc = none_null(who, {q, when(N > 0, k), positions, cos, sin})) || (rc = aligned16(who, {q, when(N > 0, k), cos, sin}, "q, k, cos and sin")) ||
      (rc = aligned4(who, {positions}, "positions")))
    return rc;
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
  int rc;
  if ((rc = geometry(who, B, L, layer_idx, N, P, format)) || (rc = dtype_ok(who, dtype)) || (rc = heads_ok(who, Nq, N)) || (rc = pages_ok(who, nnz, P)) ||
      (rc = batch_heads_ok(who, B, Nq)))
    return rc;
  if (B == 0) return ARCQ_OK;
  if ((rc = none_null(who, {o, q, kv_data, kv_indptr, kv_indices, last_page_offset, when(format == ARCQ_KV_INT4, kv_param)})) ||
      (rc = aligned16(who, {o, q, kv_data}, "o, q and kv_data")) ||
      (rc = aligned4(who, {kv_param, kv_indptr, kv_indices, last_page_offset, workspace}, "kv_param, the index tensors and the workspace")) ||
      (rc = workspace_ok(who, workspace, workspace_bytes, arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P))))
    return rc;
  KvDecodeArgs a{o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, B, Nq, L, layer_idx, N, P, nnz, format, dtype, workspace};
  return kv_decode(a, (hipStream_t)stream);
}

int arcq_kv_batch_prefill(void* o, const void* q, const int32_t* qo_indptr, const void* kv_data, const void* kv_param, const int32_t* kv_indptr,
                          const int32_t* kv_indices, const int32_t* last_page_offset, int64_t ntok, int64_t B, int64_t Nq, int64_t L, int64_t layer_idx,
                          int64_t N, int64_t P, int64_t nnz, int format, int dtype, void* stream) {
  const char* who = "arcq_kv_batch_prefill";
  int rc;
  if ((rc = geometry(who, B, L, layer_idx, N, P, format)) || (rc = dtype_ok(who, dtype)) || (rc = heads_ok(who, Nq, N)) || (rc = pages_ok(who, nnz, P)) ||
      (rc = ntok_ok(who, ntok)) || (rc = int4_only(who, format, "prefill attention reads")))
    return rc;
  if (B == 0 || ntok == 0) return ARCQ_OK;
  if ((rc = none_null(who, {o, q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset})) ||
      (rc = aligned16(who, {o, q, kv_data}, "o, q and kv_data")) ||
      (rc = aligned4(who, {kv_param, qo_indptr, kv_indptr, kv_indices, last_page_offset}, "kv_param and the index tensors")))
    return rc;
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
  int rc;
  if ((rc = geometry(who, B, L, layer_idx, N, P, format)) || (rc = dtype_ok(who, dtype)) || (rc = heads_ok(who, Nq, N)) || (rc = pages_ok(who, nnz, P)) ||
      (rc = batch_heads_ok(who, B, Nq)) || (rc = int4_only(who, format, "the decode step quantises into")) ||
      (rc = strides_ok(who, q_stride, Nq, kv_stride, N)))
    return rc;
  if (B == 0) return ARCQ_OK;
  const int64_t need = arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P), need_state = arcq_kv_decode_step_state_bytes(B, Nq, N);
  if ((rc = none_null(who, {o, q, k, v, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset})) ||
      (rc = aligned16(who, {o, q, k, v, kv_data}, "o, q, k, v and kv_data")) ||
      (rc = aligned4(who, {kv_param, kv_indptr, kv_indices, last_page_offset, workspace, state},
                     "kv_param, the index tensors, the workspace and the state")) ||
      (rc = workspace_ok(who, workspace, workspace_bytes, need)))
    return rc;
  if (need > 0 && (!state || state_bytes < need_state))       // (the arrival counters: no slices, no state)
    return fail(ARCQ_ERR_WORKSPACE, "%s: state of %lld bytes, need %lld (arcq_kv_decode_step_state_bytes)", who, (long long)state_bytes, (long long)need_state);
  KvDecodeArgs a{o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, B, Nq, L, layer_idx, N, P, nnz, format, dtype, workspace};
  KvStepArgs st{k, v, q_stride, kv_stride, state};
  return kv_decode_step(a, st, (hipStream_t)stream);
}

}  // extern "C"
