// Device-side helpers shared by the paged KV cache kernels (kv_cache.hip, kv_prefill.hip): the tables of include/arcq_kv.h, the row
// addressing of the reference's page layout and the two 16-bit element types.
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

}  // namespace arcq
