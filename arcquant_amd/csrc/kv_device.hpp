// Device-side helpers shared by the paged KV cache kernels (kv_cache.hip, kv_prefill.hip, kv_rope.hip): the tables of include/arcq_kv.h,
// the row addressing of the reference's page layout, the two 16-bit element types, and what the quantising writers share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"

namespace arcq {

constexpr int kKvD = 128;
constexpr float kKvIdle = -3.0e38f;

struct KvTables {
  const int32_t* indptr;
  const int32_t* indices;
  const int32_t* last;
};

__device__ __forceinline__ int kv_seq_len(const KvTables& t, int b, int P) { return (t.indptr[b + 1] - t.indptr[b] - 1) * P + t.last[b]; }

// row index in [pages, L, 2, N, P] of position `pos` of sequence b: K of head n (V: + N * P)
__device__ __forceinline__ size_t kv_row(const KvTables& t, int b, int n, int pos, int L, int layer, int N, int P) {
  const int pg = pos / P, e = pos - pg * P;
  const size_t page = (size_t)t.indices[t.indptr[b] + pg];
  return (((page * L + layer) * 2) * N + n) * P + e;
}

// ---- the 16-bit element types
template <bool BF16>
__device__ __forceinline__ float kv_to_f32(uint32_t bits) {
  if constexpr (BF16) return bf16_bits_to_f32(bits & 0xffffu);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)bits);
}
template <bool BF16>
__device__ __forceinline__ uint32_t kv_from_f32(float f) {
  if constexpr (BF16) return f32_to_bf16_bits(f);
  else return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
}
template <bool BF16>
__device__ __forceinline__ float kv_round(float f) { return kv_to_f32<BF16>(kv_from_f32<BF16>(f)); }

// ---- the writers' parameters, token lookup and row quantiser (kv_cache.hip, kv_rope.hip)
struct KvWriteParams {
  uint8_t* data;
  uint32_t* param;
  KvTables t;
  const uint8_t* k;
  const uint8_t* v;
  const uint32_t* kp;             // fp16 (scale, zero) pairs [ntok, N] (copy kernel only)
  const uint32_t* vp;
  const int32_t* seqlen_indptr;   // NULL: append -- token b is the last position of sequence b
  int ntok, B, L, layer, N, P, row_bytes;
};

// token -> (sequence, position); false: the token belongs to no sequence
__device__ __forceinline__ bool kv_locate(const KvWriteParams& p, int tok, int& b, int& pos) {
  if (p.seqlen_indptr == nullptr) {
    b = tok;
    pos = kv_seq_len(p.t, b, p.P) - 1;
    return pos >= 0;
  }
  if (tok >= p.seqlen_indptr[p.B]) return false;
  int lo = 0, hi = p.B;           // the last b with seqlen_indptr[b] <= tok
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.seqlen_indptr[mid] <= tok) lo = mid; else hi = mid;
  }
  b = lo;
  pos = kv_seq_len(p.t, b, p.P) - (p.seqlen_indptr[b + 1] - p.seqlen_indptr[b]) + (tok - p.seqlen_indptr[b]);
  return pos >= 0;
}

// The quantiser of a row of 128 values held NE per lane by 128 / NE adjacent lanes (lane c: elements c * NE ..): this lane's codes, element
// j in nibble j % 8 of word j / 8, and the row's fp16 (scale, zero) pair.  torch eager on a tensor of the input dtype: every operation's
// result is rounded to that dtype (the Scalar 1e-5 too).
template <bool BF16, int NE>
__device__ __forceinline__ uint32_t kv_quantize_row(const float (&x)[NE], uint32_t (&codes)[NE / 8]) {
  float xmax = x[0], xmin = x[0];
#pragma unroll
  for (int j = 1; j < NE; ++j) {
    xmax = fmaxf(xmax, x[j]);
    xmin = fminf(xmin, x[j]);
  }
#pragma unroll
  for (int sh = kKvD / NE / 2; sh > 0; sh >>= 1) {
    xmax = fmaxf(xmax, __shfl_xor(xmax, sh, 64));
    xmin = fminf(xmin, __shfl_xor(xmin, sh, 64));
  }
  const float range = fmaxf(kv_round<BF16>(xmax - xmin), kv_round<BF16>(1e-5f));
  const float scale = kv_round<BF16>(range / 15.0f);
  const float zero = -xmin;
#pragma unroll
  for (int w = 0; w < NE / 8; ++w) {
    uint32_t cw = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = kv_round<BF16>(x[w * 8 + j] + zero);
      const float qv = kv_round<BF16>(a / scale);
      const float rc = fminf(fmaxf(__builtin_rintf(qv), 0.0f), 15.0f);      // (NaN -- inf / inf of an overflowing fp16 range -- becomes code 0)
      cw |= (uint32_t)rc << (4 * j);
    }
    codes[w] = cw;
  }
  return kv_from_f32<false>(scale) | (kv_from_f32<false>(zero) << 16);
}

}  // namespace arcq
