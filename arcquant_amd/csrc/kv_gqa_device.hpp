// What the two GQA decode kernels share (kv_decode_gqa.hip over int4 pages, kv_decode_gqa16.hip over 16-bit pages): the work split's
// constants, the launch parameters, the 16x16x32 MFMA of either 16-bit type and the rounding of a pair of weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kGqWaves = 4;
constexpr int kGqBlk = 32;           // positions per block
constexpr int kGqHeads = 16;         // columns of the MFMA tile: the most query heads per kv head
constexpr int kGqRecStride = 132;    // floats of a (wave, head) record in LDS: 128 accumulators, max, sum, 2 of padding (16-byte rows)
constexpr int kGqMaxSlices = 64;

struct KvGqaParams {
  void* o;
  const void* q;
  const uint8_t* data;
  const uint32_t* param;
  KvTables t;
  float* ws;                // [B * Nq, S, kKvRec]
  int B, Nq, L, layer, N, P, S, g;
  float sm_scale;           // 128^-1/2 log2(e)
};

typedef __bf16 gq_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t gq_u32x4 __attribute__((ext_vector_type(4)));

template <bool BF16>
__device__ __forceinline__ f32x4 gq_mfma(gq_u32x4 a, gq_u32x4 b, f32x4 c) {
  if constexpr (BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(gq_bf16x8, a), __builtin_bit_cast(gq_bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// two fp32 weights rounded to the 16-bit type (nearest even), a in the low half
template <bool BF16>
__device__ __forceinline__ uint32_t gq_pack(float a, float b) {
  if constexpr (BF16) {
    return pack_bf16x2_hw(a, b);
  } else {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  }
}

}  // namespace arcq
