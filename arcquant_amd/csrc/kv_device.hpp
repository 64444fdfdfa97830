// Device-side helpers shared by the paged KV cache kernels (kv_cache.hip, kv_rope.hip, and through kv_prefill_device.hpp and
// kv_gqa_device.hpp the MFMA attention units kv_prefill.hip, kv_prefill16.hip, kv_decode_gqa.hip, kv_decode_gqa16.hip): the tables of
// include/arcq_kv.h, the row addressing of the reference's page layout, the two 16-bit element types with their MFMA operand forms, the
// constants and lane exchanges of the MFMA attention kernels' base-2 softmax, and what the quantising writers share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "gemm_common.hpp"

namespace arcq {

constexpr int kKvD = 128;
constexpr float kKvIdle = -3.0e38f;
constexpr int kKvRec = kKvD + 2;         // a merge record of the decode kernels: max, sum, 128 accumulators

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

// MFMA operands of either type travel as dwords: eight 16-bit elements are a u32x4
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// v_mfma_f32_32x32x16_{f16,bf16} (prefill) and v_mfma_f32_16x16x32_{f16,bf16} (GQA decode)
template <bool BF16>
__device__ __forceinline__ f32x16 kv_mfma32(u32x4 a, u32x4 b, f32x16 c) {
  if constexpr (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <bool BF16>
__device__ __forceinline__ f32x4 kv_mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// two fp32 weights rounded to the 16-bit type (nearest even), a in the low half
template <bool BF16>
__device__ __forceinline__ uint32_t kv_pack2(float a, float b) {
  if constexpr (BF16) {
    return pack_bf16x2_hw(a, b);
  } else {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  }
}
// eight of them: one operand fragment
template <bool BF16>
__device__ __forceinline__ u32x4 kv_pack8(const float* w) {
  return u32x4{kv_pack2<BF16>(w[0], w[1]), kv_pack2<BF16>(w[2], w[3]), kv_pack2<BF16>(w[4], w[5]), kv_pack2<BF16>(w[6], w[7])};
}

// the int4 codes in bits 0-3 and 16-19 of x as two packed 16-bit values (exact: fp16 through 1024 + c, bf16 as the top half of the fp32)
template <bool BF16>
__device__ __forceinline__ uint32_t kv_code_pair(uint32_t x) {
  x &= 0x000f000fu;
  if constexpr (BF16) {
    return (__float_as_uint((float)(x & 0xffu)) >> 16) | (__float_as_uint((float)(x >> 16)) & 0xffff0000u);
  } else {
    const f16x2 v = __builtin_bit_cast(f16x2, 0x64006400u | x);
    const f16x2 k = {(_Float16)1024.0f, (_Float16)1024.0f};
    return __builtin_bit_cast(uint32_t, v - k);
  }
}

// ---- the online softmax of the MFMA attention kernels.  It runs in base 2 (v_exp_f32): the launchers fold log2(e) into the score scale,
//      and a maximum that leaves its kernel as a natural-log score is multiplied by ln 2.
constexpr float kKvSmScaleLog2 = 0.12751743074602467f;   // 128^-1/2 * log2(e)
constexpr float kKvLn2 = 0.6931471805599453f;

// A query row's state is spread over the lanes whose numbers differ in the bits of SHARE (32: prefill's two lane halves; 16 | 32: the GQA
// kernels' four k-groups).  The sum and the maximum of x over those lanes, in every one of them:
template <int SHARE>
__device__ __forceinline__ float kv_row_sum(float x) {
  if constexpr (SHARE & 16) x += __shfl_xor(x, 16, 64);
  if constexpr (SHARE & 32) x += __shfl_xor(x, 32, 64);
  return x;
}
template <int SHARE>
__device__ __forceinline__ float kv_row_max(float x) {
  if constexpr (SHARE & 16) x = fmaxf(x, __shfl_xor(x, 16, 64));
  if constexpr (SHARE & 32) x = fmaxf(x, __shfl_xor(x, 32, 64));
  return x;
}

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
