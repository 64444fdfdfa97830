// The quantising writers of the FP8 (OCP e4m3) paged KV cache of include/arcq_kv.h (arcq_kv_fp8_append_quantize, arcq_kv_fp8_init_quantize):
// fp16 / bf16 rows [tokens, N, 128] -> 128 code bytes and one fp16 (scale, 0) pair per row, straight into the page, one launch.
//
// The rule (kvfp8.quantize_fp8 restates it in torch), in fp32 with IEEE division:
//     scale = fp16(max(amax / 448, 2^-14));   code = e4m3(clamp(x / float(scale), -448, 448))
// fp16(.) and e4m3(.) round to nearest even (v_cvt_f16_f32, v_cvt_pk_fp8_f32: subnormal codes included); the clamp keeps a quotient that a
// scale rounded DOWN to fp16 left a hair above 448 a finite code.  Byte for byte the torch formula on a CPU tensor.  Inputs are finite.
//
//   kv_quantize8_kernel   rows = (token, K | V, head), eight rows per wave: the eight lanes of a row hold 16 consecutive values each (two
//                         16-byte loads: the lanes of a row read its 256 bytes), |x| max over the lane and then over the eight lanes on
//                         DPP (two quad permutes, one half-row mirror: no LDS, no ds_bpermute), 16 quotients, eight packed conversions and
//                         ONE 16-byte store of codes per lane -- a row's eight stores are its one cache line; lane 0 of the row stores
//                         the (scale, 0) word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kQ8RowsPerWave = 8, kQ8RowsPerBlock = 4 * kQ8RowsPerWave;

template <int CTRL>
__device__ __forceinline__ float q8_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

template <bool BF16>
__global__ __launch_bounds__(256) void kv_quantize8_kernel(KvWriteParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane >> 3, c = lane & 7;
  const int64_t rows = (int64_t)p.ntok * 2 * p.N;
  const int64_t R = ((int64_t)blockIdx.x * 4 + wave) * kQ8RowsPerWave + r;
  if (R >= rows) return;                                // (the eight lanes of a row leave together; the DPP exchanges stay inside a row)
  const int tok = (int)(R / (2 * p.N)), rem = (int)(R - (int64_t)tok * 2 * p.N);
  const int which = rem >= p.N, n = rem - which * p.N;
  int b, pos;
  if (!kv_locate(p, tok, b, pos)) return;
  const uint4* src = reinterpret_cast<const uint4*>((which ? p.v : p.k) + ((size_t)tok * p.N + n) * (kKvD * 2) + c * 32);
  const uint4 d0 = src[0], d1 = src[1];
  const uint32_t w[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
  float x[16];
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[2 * j] = kv_to_f32<BF16>(w[j] & 0xffffu);
    x[2 * j + 1] = kv_to_f32<BF16>(w[j] >> 16);
    amax = fmaxf(amax, fmaxf(__builtin_fabsf(x[2 * j]), __builtin_fabsf(x[2 * j + 1])));
  }
  amax = fmaxf(amax, q8_dpp<0xB1>(amax));               // quad_perm [1, 0, 3, 2]
  amax = fmaxf(amax, q8_dpp<0x4E>(amax));               // quad_perm [2, 3, 0, 1]
  amax = fmaxf(amax, q8_dpp<0x141>(amax));              // row_half_mirror: the other quad of the eight lanes
  const uint32_t sbits = kv_from_f32<false>(fmaxf(amax / 448.0f, 0x1p-14f));
  const float scale = kv_to_f32<false>(sbits);
  uint32_t cw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = fminf(fmaxf(x[4 * j + e] / scale, -448.0f), 448.0f);
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], pk, true);
    cw[j] = (uint32_t)pk;
  }
  const size_t row = kv_row(p.t, b, n, pos, p.L, p.layer, p.N, p.P) + (size_t)which * p.N * p.P;
  *reinterpret_cast<uint4*>(p.data + row * kKvD + c * 16) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
  if (c == 0) p.param[row] = sbits;                     // (scale, 0)
}

// ---- launcher (arguments validated by c_api_kv.hip; a.k_param, a.v_param and a.format are not read)
int kv_write8(const KvWriteArgs& a, hipStream_t stream) {
  const char* who = a.seqlen_indptr ? "arcq_kv_fp8_init_quantize" : "arcq_kv_fp8_append_quantize";
  KvWriteParams p{};
  p.data = (uint8_t*)a.kv_data; p.param = (uint32_t*)a.kv_param;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.k = (const uint8_t*)a.k; p.v = (const uint8_t*)a.v;
  p.seqlen_indptr = a.seqlen_indptr;
  p.ntok = (int)a.ntok; p.B = (int)a.B; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.row_bytes = kKvD;
  const int64_t rows = a.ntok * 2 * a.N;
  const dim3 grid((unsigned)((rows + kQ8RowsPerBlock - 1) / kQ8RowsPerBlock));
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<kv_quantize8_kernel<true>>(grid, dim3(256), 0, stream, who, p);
  return launch_kernel<kv_quantize8_kernel<false>>(grid, dim3(256), 0, stream, who, p);
}

}  // namespace arcq
