// Rotary position embedding on the KV path (include/arcq_kv.h: arcq_rope_qk, arcq_kv_rope_append_quantize, arcq_kv_rope_init_quantize).
//
// The rotation is the rotate-half one over the full head dimension, from the caller's tables cos, sin [rope_len, 128]:
//     out[i] = round(round(x[i] * cos[p, i]) + round(rot(x)[i] * sin[p, i])),   rot(x)[i] = -x[i + 64] (i < 64) | x[i - 64]
// with the products and the sum in fp32 and each of the three results rounded to the 16-bit type: what torch eager gives for
// x * cos + rotate_half(x) * sin on a tensor of that type.  No trigonometry here, and the halves of a table row are not assumed equal.
//
// A row of 128 values is held 8 per lane by 16 adjacent lanes, as in kv_quantize_kernel (lane c: elements 8 c ..).  The partner of
// element i is i +- 64, which lane c ^ 8 holds at the same place in its words: one exchange of the four packed words.
//
//   kv_rope_quantize_kernel  rows = (token, slot); slots [0, Nq) are q heads, [Nq, Nq + N) k heads, [Nq + N, Nq + 2 N) v heads.  Four rows
//                            per wave.  q: rotated, one 16-byte store into q_out.  k: rotated, then kv_quantize_row, codes and parameters
//                            into the page.  v: quantised and stored as kv_quantize_kernel does.  The position of a token is the one it is
//                            written at (kv_locate); a token without a position writes nothing, its q_out rows included.
//   rope_qk_kernel           the rotation alone, in place on strided q and k rows; token i takes positions[i % n_pos].  A row is whole in
//                            registers before its first store and no two rows overlap.
// Neither uses LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "kv_device.hpp"

namespace arcq {

struct KvRopeParams {
  KvWriteParams w;                // k, v: rows kv_stride elements apart (kp, vp, row_bytes unused)
  const uint16_t* q;              // [ntok, Nq, 128], tokens q_stride elements apart
  uint16_t* q_out;                // [ntok, Nq, 128], contiguous
  const uint16_t* cos;            // [rope_len, 128]
  const uint16_t* sin;
  int64_t q_stride, kv_stride;
  int Nq;
};

struct RopeQkParams {
  uint16_t* q;
  uint16_t* k;
  const int32_t* positions;
  const uint16_t* cos;
  const uint16_t* sin;
  int64_t q_stride, k_stride;
  int ntok, n_pos, Nq, N;
};

// the four words lane c ^ 8 holds (the 16 lanes of a row are all here: callers leave a row at a time)
__device__ __forceinline__ void kv_rope_partner(const uint32_t (&w)[4], uint32_t (&o)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (uint32_t)__shfl_xor((int)w[j], 8, 64);
}

// this lane's 8 elements of a row rotated to position `pos`: x = own words, o = the partner lane's; every product and the sum rounded
template <bool BF16>
__device__ __forceinline__ void kv_rope_row(const uint32_t (&w)[4], const uint32_t (&o)[4], const uint16_t* cos, const uint16_t* sin, int pos, int c,
                                            float (&y)[8]) {
  const uint4 cd = *reinterpret_cast<const uint4*>(cos + (size_t)pos * kKvD + c * 8);
  const uint4 sd = *reinterpret_cast<const uint4*>(sin + (size_t)pos * kKvD + c * 8);
  const uint32_t cw[4] = {cd.x, cd.y, cd.z, cd.w}, sw[4] = {sd.x, sd.y, sd.z, sd.w};
  const float sign = c < 8 ? -1.0f : 1.0f;              // elements below 64 take -x[i + 64], the others x[i - 64]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int sh = 16 * h;
      const float x = kv_to_f32<BF16>((w[j] >> sh) & 0xffffu), r = sign * kv_to_f32<BF16>((o[j] >> sh) & 0xffffu);
      const float cs = kv_to_f32<BF16>((cw[j] >> sh) & 0xffffu), sn = kv_to_f32<BF16>((sw[j] >> sh) & 0xffffu);
      y[2 * j + h] = kv_round<BF16>(kv_round<BF16>(x * cs) + kv_round<BF16>(r * sn));
    }
  }
}

template <bool BF16>
__device__ __forceinline__ uint4 kv_rope_pack(const float (&y)[8]) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = kv_from_f32<BF16>(y[2 * j]) | (kv_from_f32<BF16>(y[2 * j + 1]) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

template <bool BF16>
__global__ __launch_bounds__(256) void kv_rope_quantize_kernel(KvRopeParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane >> 4, c = lane & 15;
  const int N = p.w.N, slots = p.Nq + 2 * N;
  const int64_t rows = (int64_t)p.w.ntok * slots;
  const int64_t R = ((int64_t)blockIdx.x * 4 + wave) * 4 + r;
  if (R >= rows) return;                                // (the 16 lanes of a row leave together; the shuffles below stay inside a row)
  const int tok = (int)(R / slots), slot = (int)(R - (int64_t)tok * slots);
  int b, pos;
  if (!kv_locate(p.w, tok, b, pos)) return;
  const bool isq = slot < p.Nq, isv = slot >= p.Nq + N;
  const int n = isq ? slot : slot - p.Nq - (isv ? N : 0);
  const uint16_t* src = isq ? p.q + (size_t)tok * p.q_stride
                            : reinterpret_cast<const uint16_t*>(isv ? p.w.v : p.w.k) + (size_t)tok * p.kv_stride;
  const uint4 d = *reinterpret_cast<const uint4*>(src + (size_t)n * kKvD + c * 8);
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  uint32_t o[4];
  kv_rope_partner(w, o);
  float x[8];
  if (isv) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = kv_to_f32<BF16>(w[j] & 0xffffu);
      x[2 * j + 1] = kv_to_f32<BF16>(w[j] >> 16);
    }
  } else {
    kv_rope_row<BF16>(w, o, p.cos, p.sin, pos, c, x);
  }
  if (isq) {
    *reinterpret_cast<uint4*>(p.q_out + ((size_t)tok * p.Nq + n) * kKvD + c * 8) = kv_rope_pack<BF16>(x);
    return;
  }
  uint32_t codes[1];
  const uint32_t param = kv_quantize_row<BF16, 8>(x, codes);
  const size_t row = kv_row(p.w.t, b, n, pos, p.w.L, p.w.layer, N, p.w.P) + (size_t)isv * N * p.w.P;
  *reinterpret_cast<uint32_t*>(p.w.data + row * 64 + c * 4) = codes[0];
  if (c == 0) p.w.param[row] = param;
}

template <bool BF16>
__global__ __launch_bounds__(256) void rope_qk_kernel(RopeQkParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane >> 4, c = lane & 15;
  const int slots = p.Nq + p.N;
  const int64_t rows = (int64_t)p.ntok * slots;
  const int64_t R = ((int64_t)blockIdx.x * 4 + wave) * 4 + r;
  if (R >= rows) return;                                // (a row's 16 lanes leave together)
  const int tok = (int)(R / slots), slot = (int)(R - (int64_t)tok * slots);
  const bool isq = slot < p.Nq;
  uint16_t* row = (isq ? p.q + (size_t)tok * p.q_stride + (size_t)slot * kKvD : p.k + (size_t)tok * p.k_stride + (size_t)(slot - p.Nq) * kKvD) + c * 8;
  const int pos = p.positions[tok % p.n_pos];
  const uint4 d = *reinterpret_cast<const uint4*>(row);
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  uint32_t o[4];
  kv_rope_partner(w, o);                                // the whole row is in registers here: the store below is safe in place
  float y[8];
  kv_rope_row<BF16>(w, o, p.cos, p.sin, pos, c, y);
  *reinterpret_cast<uint4*>(row) = kv_rope_pack<BF16>(y);
}

// ---- launchers (arguments validated by c_api_kv.hip)
int kv_rope_write(const KvRopeArgs& a, hipStream_t stream) {
  KvRopeParams p{};
  p.w.data = (uint8_t*)a.w.kv_data; p.w.param = (uint32_t*)a.w.kv_param;
  p.w.t = {a.w.kv_indptr, a.w.kv_indices, a.w.last_page_offset};
  p.w.k = (const uint8_t*)a.w.k; p.w.v = (const uint8_t*)a.w.v; p.w.kp = nullptr; p.w.vp = nullptr;
  p.w.seqlen_indptr = a.w.seqlen_indptr;
  p.w.ntok = (int)a.w.ntok; p.w.B = (int)a.w.B; p.w.L = (int)a.w.L; p.w.layer = (int)a.w.layer; p.w.N = (int)a.w.N; p.w.P = (int)a.w.P;
  p.w.row_bytes = 64;
  p.q = (const uint16_t*)a.q; p.q_out = (uint16_t*)a.q_out; p.cos = (const uint16_t*)a.cos; p.sin = (const uint16_t*)a.sin;
  p.q_stride = a.q_stride; p.kv_stride = a.kv_stride; p.Nq = (int)a.Nq;
  const int64_t rows = a.w.ntok * (a.Nq + 2 * a.w.N);
  const dim3 grid((unsigned)((rows + 15) / 16));
  if (a.w.dtype == ARCQ_KV_BF16) return launch_kernel<kv_rope_quantize_kernel<true>>(grid, dim3(256), 0, stream, a.who, p);
  return launch_kernel<kv_rope_quantize_kernel<false>>(grid, dim3(256), 0, stream, a.who, p);
}

int kv_rope_qk(const RopeQkArgs& a, hipStream_t stream) {
  RopeQkParams p{};
  p.q = (uint16_t*)a.q; p.k = (uint16_t*)a.k; p.positions = a.positions; p.cos = (const uint16_t*)a.cos; p.sin = (const uint16_t*)a.sin;
  p.q_stride = a.q_stride; p.k_stride = a.k_stride;
  p.ntok = (int)a.ntok; p.n_pos = (int)a.n_pos; p.Nq = (int)a.Nq; p.N = (int)a.N;
  const int64_t rows = a.ntok * (a.Nq + a.N);
  const dim3 grid((unsigned)((rows + 15) / 16));
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<rope_qk_kernel<true>>(grid, dim3(256), 0, stream, "arcq_rope_qk", p);
  return launch_kernel<rope_qk_kernel<false>>(grid, dim3(256), 0, stream, "arcq_rope_qk", p);
}

}  // namespace arcq
