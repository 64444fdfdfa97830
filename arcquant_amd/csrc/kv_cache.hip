// The paged KV cache of include/arcq_kv.h: writers (copy and quantise-and-write) and the decode attention over int4 or 16-bit pages.
//
// Layout (the reference's, include/flashinfer/page.cuh:76-103): rows of the grid [pages, L, 2, N, P]; a row is 64 bytes of codes
// (element 2j in the low nibble of byte j) or 128 16-bit values, and has one (scale, zero) fp16 pair in kv_param at the same row
// index.  Position t of sequence b lives in page kv_indices[kv_indptr[b] + t / P], entry t % P.
//
//   kv_write_kernel      one workgroup per token: 16-byte copies of the K and V rows of every head + their parameter pairs
//   kv_quantize_kernel   four rows per wave (16 lanes x 8 values): amax / amin over the row, the torch-eager formula with every
//                        operation rounded to the input dtype, codes and parameters stored straight into the page
//   kv_decode_kernel     grid (B * N * chunks, S): a 256-thread workgroup per (sequence, kv head, chunk of <= 4 query heads of that kv
//                        head, slice of the sequence).  A wave streams a contiguous range of positions: each lane holds 16 codes (8
//                        bytes, 8 rows per 512-byte wave load) or 8 16-bit values (16 bytes, 4 rows per 1-KiB load) of a row, four
//                        K loads, four V loads and their parameters requested together, the next block's in flight while this one
//                        is reduced.  Scores use  sum_d q_d (c_d s - z) = s sum_d q_d c_d - z sum_d q_d  and the value sum
//                        sum_t p_t (c_td s_t - z_t) = sum_t (p_t s_t) c_td - sum_t p_t z_t:  one conversion and one FMA per code
//                        and query head.  Online softmax per wave, the waves merge through LDS; S > 1 leaves (max, sum, 128
//                        accumulators) records in the workspace for kv_decode_combine.  fp32 throughout.
//   kv_decode_kernel<.., STEP>  the decode step in one launch (arcq_kv_decode_step): the same grid, ranges and arithmetic over strided
//                        q / k / v rows of the projection output.  The wave whose range holds position T - 1 quantises k[b, n] and
//                        v[b, n] (kv_quantize_row, the quantiser's own formula) in front of its last block and uses the codes in place
//                        of the page's row; chunk 0's owner stores them.  With S > 1 every workgroup publishes its records (agent-scope
//                        release) and draws a ticket from cnt[b, n, chunk]; the one that draws S - 1 acquires, merges the S records as
//                        kv_decode_combine does, stores o and puts the counter back to 0.  Nobody waits for anybody.
//   Rows past a wave's range are clamped to the sequence's last valid position (STEP: the one before it, which is in the page) and
//   masked: no byte outside the valid positions of the pages the tables name is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kKvRec = kKvD + 2;         // a merge record: max, sum, 128 accumulators
constexpr int kKvWaves = 4;

// ---- writers (KvWriteParams, kv_locate and kv_quantize_row: kv_device.hpp)
__global__ __launch_bounds__(256) void kv_write_kernel(KvWriteParams p) {
  const int tok = blockIdx.x, tid = threadIdx.x;
  int b, pos;
  if (!kv_locate(p, tok, b, pos)) return;
  const int cpr = p.row_bytes >> 4;                     // 16-byte chunks per row
  const int chunks = p.N * cpr;
  const size_t vrows = (size_t)p.N * p.P;
  const size_t row0 = kv_row(p.t, b, 0, pos, p.L, p.layer, p.N, p.P);
  for (int i = tid; i < 2 * chunks; i += 256) {
    const int which = i >= chunks, j = i - which * chunks;
    const int n = j / cpr, c = j - n * cpr;
    const uint4 d = *reinterpret_cast<const uint4*>((which ? p.v : p.k) + ((size_t)tok * p.N + n) * p.row_bytes + c * 16);
    *reinterpret_cast<uint4*>(p.data + (row0 + which * vrows + (size_t)n * p.P) * p.row_bytes + c * 16) = d;
  }
  for (int i = tid; i < 2 * p.N; i += 256) {
    const int which = i >= p.N, n = i - which * p.N;
    p.param[row0 + which * vrows + (size_t)n * p.P] = (which ? p.vp : p.kp)[(size_t)tok * p.N + n];
  }
}

// rows = (token, K | V, head); four rows per wave, 16 lanes x 8 values each
template <bool BF16>
__global__ __launch_bounds__(256) void kv_quantize_kernel(KvWriteParams p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane >> 4, c = lane & 15;
  const int64_t rows = (int64_t)p.ntok * 2 * p.N;
  const int64_t R = ((int64_t)blockIdx.x * 4 + wave) * 4 + r;
  if (R >= rows) return;                                // (the 16 lanes of a row leave together; the shuffles below stay inside a row)
  const int tok = (int)(R / (2 * p.N)), rem = (int)(R - (int64_t)tok * 2 * p.N);
  const int which = rem >= p.N, n = rem - which * p.N;
  int b, pos;
  if (!kv_locate(p, tok, b, pos)) return;
  const uint4 d = *reinterpret_cast<const uint4*>((which ? p.v : p.k) + ((size_t)tok * p.N + n) * (kKvD * 2) + c * 16);
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
  float x[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = kv_to_f32<BF16>(w[j] & 0xffffu);
    x[2 * j + 1] = kv_to_f32<BF16>(w[j] >> 16);
  }
  uint32_t codes[1];
  const uint32_t param = kv_quantize_row<BF16, 8>(x, codes);
  const size_t row = kv_row(p.t, b, n, pos, p.L, p.layer, p.N, p.P) + (size_t)which * p.N * p.P;
  *reinterpret_cast<uint32_t*>(p.data + row * 64 + c * 4) = codes[0];
  if (c == 0) p.param[row] = param;
}

// ---- decode attention
struct KvDecodeParams {
  void* o;
  const void* q;
  const uint8_t* data;
  const uint32_t* param;
  KvTables t;
  float* ws;                // [B * Nq, S, kKvRec]
  int B, Nq, L, layer, N, P, S, g, chunks;
  float sm_scale;
};
// what the decode step takes on top (its own type, so the other instances keep their kernel arguments as they were): this token's k, v
// rows [B, N, 128] (tokens kv_stride elements apart; q: q_stride) and the arrival counters
struct KvStepParams : KvDecodeParams {
  const uint16_t* k;
  const uint16_t* v;
  int32_t* cnt;             // [B * N * chunks], zero between launches
  int64_t q_stride, kv_stride;
};
template <bool STEP>
struct KvParamsOf { using type = KvDecodeParams; };
template <>
struct KvParamsOf<true> { using type = KvStepParams; };

template <int EPL>
struct KvRaw {
  uint32_t w[EPL == 16 ? 2 : 4];                       // 16 codes = 2 words, 8 16-bit values = 4 words
};

// The S slice records of one (sequence, query head) -> output element d: max over s, the sums in s order, one rounding.
template <bool BF16>
__device__ __forceinline__ uint16_t kv_merge_slices(const float* w, int S, int d) {
  float M = kKvIdle;
  for (int s = 0; s < S; ++s) M = fmaxf(M, w[s * kKvRec]);
  float Ls = 0.f, a = 0.f;
  for (int s = 0; s < S; ++s) {
    const float f = __expf(w[s * kKvRec] - M);
    Ls += w[s * kKvRec + 1] * f;
    a += w[s * kKvRec + 2 + d] * f;
  }
  return (uint16_t)kv_from_f32<BF16>(Ls > 0.f ? a / Ls : 0.f);
}

// STEP (int4 only) is the whole decode step in one launch: q, k, v are strided rows of the projection output, position T - 1 is taken from
// k / v -- quantised by the wave whose range holds it, which uses the codes in place of the page's row and, in chunk 0, stores them -- and
// the last workgroup of a (sequence, kv head, chunk) to arrive merges the S records.  No position T - 1 of the page is read: rows past a
// wave's range clamp to T - 2, and a sequence of one position loads nothing.  No workgroup waits for another.
template <int FMT, bool BF16, int GC, bool STEP = false>
__global__ __launch_bounds__(kKvWaves * 64) void kv_decode_kernel(typename KvParamsOf<STEP>::type p) {
  static_assert(!STEP || FMT == ARCQ_KV_INT4, "the decode step quantises into an int4 cache");
  constexpr bool I4 = FMT == ARCQ_KV_INT4;
  constexpr int EPL = I4 ? 16 : 8;                     // elements per lane
  constexpr int LPR = kKvD / EPL;                      // lanes per row: 8 | 16
  constexpr int RPL = 64 / LPR;                        // rows per wave load: 8 | 4
  constexpr int NL = 4;                                // loads of K (and of V) in flight per block
  constexpr int BP = NL * RPL;                         // positions per block: 32 | 16
  constexpr int ROWB = I4 ? 64 : 256, LANEB = ROWB / LPR, NW = LANEB / 4;
  __shared__ float rec[kKvWaves][GC][kKvRec];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane / LPR, c = lane % LPR;
  const int ch = blockIdx.x % p.chunks, bn = blockIdx.x / p.chunks;
  const int b = bn / p.N, n = bn - b * p.N;
  const int s = blockIdx.y;
  const int T = kv_seq_len(p.t, b, p.P);
  const int nblk = (T + BP - 1) / BP, units = p.S * kKvWaves;
  const int per = (nblk + units - 1) / units;
  const int t0 = min(T, (s * kKvWaves + wave) * per * BP), t1 = min(T, t0 + per * BP);
  const size_t vrows = (size_t)p.N * p.P;

  // this chunk's query heads (a head past the group repeats the last one and is not stored)
  float qf[GC][EPL], qsum[GC];
#pragma unroll
  for (int gi = 0; gi < GC; ++gi) {
    const int h = n * p.g + min(ch * GC + gi, p.g - 1);
    size_t qoff = ((size_t)b * p.Nq + h) * kKvD;
    if constexpr (STEP) qoff = (size_t)b * p.q_stride + (size_t)h * kKvD;
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(p.q) + qoff + c * EPL;
    float acc = 0.f;
#pragma unroll
    for (int e8 = 0; e8 < EPL / 8; ++e8) {
      const uint4 d = *reinterpret_cast<const uint4*>(qrow + e8 * 8);
      const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qf[gi][e8 * 8 + 2 * j] = kv_to_f32<BF16>(w[j] & 0xffffu) * p.sm_scale;
        qf[gi][e8 * 8 + 2 * j + 1] = kv_to_f32<BF16>(w[j] >> 16) * p.sm_scale;
      }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc += qf[gi][e];
#pragma unroll
    for (int sh = LPR / 2; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
    qsum[gi] = acc;
  }

  using Raw = KvRaw<EPL>;
  auto load_block = [&](int tb, Raw (&kk)[NL], Raw (&vv)[NL], uint32_t (&pk)[NL], uint32_t (&pv)[NL]) __attribute__((always_inline)) {
    if constexpr (STEP) {
      if (T == 1) {                                     // the new position alone: nothing of the page is read
#pragma unroll
        for (int u = 0; u < NL; ++u) {
          kk[u].w[0] = 0; kk[u].w[1] = 0; vv[u].w[0] = 0; vv[u].w[1] = 0;
          pk[u] = 0; pv[u] = 0;
        }
        return;
      }
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int t = min(tb + u * RPL + r, STEP ? T - 2 : T - 1);   // past the range: the sequence's last stored row, masked below
      const size_t row = kv_row(p.t, b, n, t, p.L, p.layer, p.N, p.P);
      const uint8_t* ka = p.data + row * ROWB + c * LANEB;
      const uint8_t* va = ka + vrows * ROWB;
      if constexpr (I4) {
        const uint2 a = *reinterpret_cast<const uint2*>(ka), bb = *reinterpret_cast<const uint2*>(va);
        kk[u].w[0] = a.x; kk[u].w[1] = a.y;
        vv[u].w[0] = bb.x; vv[u].w[1] = bb.y;
        pk[u] = p.param[row];
        pv[u] = p.param[row + vrows];
      } else {
        const uint4 a = *reinterpret_cast<const uint4*>(ka), bb = *reinterpret_cast<const uint4*>(va);
        kk[u].w[0] = a.x; kk[u].w[1] = a.y; kk[u].w[2] = a.z; kk[u].w[3] = a.w;
        vv[u].w[0] = bb.x; vv[u].w[1] = bb.y; vv[u].w[2] = bb.z; vv[u].w[3] = bb.w;
        pk[u] = 0; pv[u] = 0;
      }
    }
  };
  auto decode = [&](const Raw& raw, float (&x)[EPL]) __attribute__((always_inline)) {
#pragma unroll
    for (int wi = 0; wi < NW; ++wi) {
      if constexpr (I4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) x[wi * 8 + i] = (float)((raw.w[wi] >> (4 * i)) & 15u);
      } else {
        x[wi * 2] = kv_to_f32<BF16>(raw.w[wi] & 0xffffu);
        x[wi * 2 + 1] = kv_to_f32<BF16>(raw.w[wi] >> 16);
      }
    }
  };

  float m[GC], l[GC], zacc[GC], acc[GC][EPL];
#pragma unroll
  for (int gi = 0; gi < GC; ++gi) {
    m[gi] = kKvIdle; l[gi] = 0.f; zacc[gi] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[gi][e] = 0.f;
  }
  auto consume = [&](int tb, const Raw (&kk)[NL], const Raw (&vv)[NL], const uint32_t (&pk)[NL], const uint32_t (&pv)[NL]) __attribute__((always_inline)) {
    float d[NL][GC], mb[GC];
#pragma unroll
    for (int gi = 0; gi < GC; ++gi) mb[gi] = kKvIdle;
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      float x[EPL];
      decode(kk[u], x);
      const bool valid = tb + u * RPL + r < t1;
      const float ks = I4 ? kv_to_f32<false>(pk[u] & 0xffffu) : 1.f, kz = I4 ? kv_to_f32<false>(pk[u] >> 16) : 0.f;
#pragma unroll
      for (int gi = 0; gi < GC; ++gi) {
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) dot = fmaf(qf[gi][e], x[e], dot);
#pragma unroll
        for (int sh = LPR / 2; sh > 0; sh >>= 1) dot += __shfl_xor(dot, sh, 64);
        const float sc = I4 ? ks * dot - kz * qsum[gi] : dot;
        d[u][gi] = valid ? sc : kKvIdle;
        mb[gi] = fmaxf(mb[gi], d[u][gi]);
      }
    }
#pragma unroll
    for (int gi = 0; gi < GC; ++gi) {
#pragma unroll
      for (int sh = LPR; sh < 64; sh <<= 1) mb[gi] = fmaxf(mb[gi], __shfl_xor(mb[gi], sh, 64));   // over the row groups: wave-uniform
      const float mn = fmaxf(m[gi], mb[gi]), a = __expf(m[gi] - mn);
      l[gi] *= a;
      zacc[gi] *= a;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[gi][e] *= a;
      m[gi] = mn;
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      float x[EPL];
      decode(vv[u], x);
      const bool valid = tb + u * RPL + r < t1;
      const float vs = I4 ? kv_to_f32<false>(pv[u] & 0xffffu) : 1.f, vz = I4 ? kv_to_f32<false>(pv[u] >> 16) : 0.f;
#pragma unroll
      for (int gi = 0; gi < GC; ++gi) {
        const float pt = valid ? __expf(d[u][gi] - m[gi]) : 0.f;
        l[gi] += pt;                                    // (this lane's row group; the groups are added at the end)
        const float ps = pt * vs;
        if constexpr (I4) zacc[gi] += pt * vz;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[gi][e] = fmaf(ps, x[e], acc[gi][e]);
      }
    }
  };

  // STEP: the wave whose range ends at T owns position T - 1.  In front of its last block it quantises k[b, n] and v[b, n] and puts the
  // codes and parameters where load_block's row T - 1 would be (that row holds T - 2's, or zeros); chunk 0's owner stores them.
  const bool own = STEP && t0 < t1 && t1 == T;
  auto new_row = [&](int tb, Raw (&kk)[NL], Raw (&vv)[NL], uint32_t (&pk)[NL], uint32_t (&pv)[NL]) __attribute__((always_inline)) {
    if constexpr (STEP) {
      if (own && tb + BP >= T) {
        const int rel = T - 1 - tb, us = rel / RPL;
        const bool mine = r == rel - us * RPL;
        const size_t row = kv_row(p.t, b, n, T - 1, p.L, p.layer, p.N, p.P);
        uint8_t* data = const_cast<uint8_t*>(p.data);
        uint32_t* param = const_cast<uint32_t*>(p.param);
        auto one = [&](const uint16_t* src, size_t dst, Raw (&cc)[NL], uint32_t (&pp)[NL]) __attribute__((always_inline)) {
          const uint16_t* xr = src + (size_t)b * p.kv_stride + (size_t)n * kKvD + c * EPL;
          float x[EPL];
#pragma unroll
          for (int e8 = 0; e8 < EPL / 8; ++e8) {
            const uint4 d = *reinterpret_cast<const uint4*>(xr + e8 * 8);
            const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              x[e8 * 8 + 2 * j] = kv_to_f32<BF16>(w[j] & 0xffffu);
              x[e8 * 8 + 2 * j + 1] = kv_to_f32<BF16>(w[j] >> 16);
            }
          }
          uint32_t cw[EPL / 8];
          const uint32_t pw = kv_quantize_row<BF16, EPL>(x, cw);
#pragma unroll
          for (int u = 0; u < NL; ++u) {
            const bool here = mine && u == us;
            cc[u].w[0] = here ? cw[0] : cc[u].w[0];
            cc[u].w[1] = here ? cw[1] : cc[u].w[1];
            pp[u] = here ? pw : pp[u];
          }
          if (ch == 0 && mine) {
            *reinterpret_cast<uint2*>(data + dst * ROWB + c * LANEB) = make_uint2(cw[0], cw[1]);
            if (c == 0) param[dst] = pw;
          }
        };
        one(p.k, row, kk, pk);
        one(p.v, row + vrows, vv, pv);
      }
    }
  };

  if (t0 < t1) {
    Raw k0[NL], v0[NL], k1[NL], v1[NL];
    uint32_t pk0[NL], pv0[NL], pk1[NL], pv1[NL];
    load_block(t0, k0, v0, pk0, pv0);
    for (int tb = t0; tb < t1; tb += 2 * BP) {         // two blocks per trip: the other buffer's loads stay in flight
      if (tb + BP < t1) load_block(tb + BP, k1, v1, pk1, pv1);
      new_row(tb, k0, v0, pk0, pv0);
      consume(tb, k0, v0, pk0, pv0);
      if (tb + BP < t1) {
        if (tb + 2 * BP < t1) load_block(tb + 2 * BP, k0, v0, pk0, pv0);
        new_row(tb + BP, k1, v1, pk1, pv1);
        consume(tb + BP, k1, v1, pk1, pv1);
      }
    }
  }
  // the row groups of a wave hold the same columns: add them; then the wave's record
#pragma unroll
  for (int gi = 0; gi < GC; ++gi) {
#pragma unroll
    for (int sh = LPR; sh < 64; sh <<= 1) {
      l[gi] += __shfl_xor(l[gi], sh, 64);
      zacc[gi] += __shfl_xor(zacc[gi], sh, 64);
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[gi][e] += __shfl_xor(acc[gi][e], sh, 64);
    }
    if (r == 0) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) rec[wave][gi][2 + c * EPL + e] = acc[gi][e] - zacc[gi];
      if (c == 0) {
        rec[wave][gi][0] = m[gi];
        rec[wave][gi][1] = l[gi];
      }
    }
  }
  __syncthreads();
  if (tid < kKvD) {                                     // merge of the waves (idle ones carry m = kKvIdle, l = 0)
#pragma unroll
    for (int gi = 0; gi < GC; ++gi) {
      if (ch * GC + gi >= p.g) break;
      const int h = n * p.g + ch * GC + gi;
      float M = kKvIdle;
#pragma unroll
      for (int w = 0; w < kKvWaves; ++w) M = fmaxf(M, rec[w][gi][0]);
      float Ls = 0.f, a = 0.f;
#pragma unroll
      for (int w = 0; w < kKvWaves; ++w) {
        const float f = __expf(rec[w][gi][0] - M);
        Ls += rec[w][gi][1] * f;
        a += rec[w][gi][2 + tid] * f;
      }
      const size_t bh = (size_t)b * p.Nq + h;
      if (p.S == 1) {
        reinterpret_cast<uint16_t*>(p.o)[bh * kKvD + tid] = (uint16_t)kv_from_f32<BF16>(Ls > 0.f ? a / Ls : 0.f);
      } else {
        float* o = p.ws + (bh * p.S + s) * kKvRec;
        o[2 + tid] = a;
        if (tid == 0) {
          o[0] = M;
          o[1] = Ls;
        }
      }
    }
  }
  if constexpr (STEP) {
    if (p.S == 1) return;
    // records out, then one ticket per workgroup; the workgroup that draws the last one merges.  rec is free again behind the barrier.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int ticket = __hip_atomic_fetch_add(p.cnt + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = ticket == p.S - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      rec[0][0][0] = last ? 1.f : 0.f;
    }
    __syncthreads();                                    // two duties: "last" reaches every wave, and no wave loads a record before the acquire is complete
    if (rec[0][0][0] == 0.f) return;
    const int d = tid & (kKvD - 1);
#pragma unroll
    for (int gi = tid >> 7; gi < GC; gi += 2) {         // two query heads at a time
      if (ch * GC + gi >= p.g) break;
      const size_t bh = (size_t)b * p.Nq + n * p.g + ch * GC + gi;
      reinterpret_cast<uint16_t*>(p.o)[bh * kKvD + d] = kv_merge_slices<BF16>(p.ws + bh * p.S * kKvRec, p.S, d);
    }
    if (tid == 0) __hip_atomic_store(p.cnt + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool BF16>
__global__ __launch_bounds__(kKvD) void kv_decode_combine(KvDecodeParams p) {
  const size_t bh = blockIdx.x;
  const int d = threadIdx.x;
  reinterpret_cast<uint16_t*>(p.o)[bh * kKvD + d] = kv_merge_slices<BF16>(p.ws + bh * p.S * kKvRec, p.S, d);
}

// ---- launchers (arguments validated by c_api_kv.hip)
int kv_write(const KvWriteArgs& a, hipStream_t stream) {
  KvWriteParams p;
  p.data = (uint8_t*)a.kv_data; p.param = (uint32_t*)a.kv_param;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.k = (const uint8_t*)a.k; p.v = (const uint8_t*)a.v; p.kp = (const uint32_t*)a.k_param; p.vp = (const uint32_t*)a.v_param;
  p.seqlen_indptr = a.seqlen_indptr;
  p.ntok = (int)a.ntok; p.B = (int)a.B; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.row_bytes = a.format == ARCQ_KV_INT4 ? 64 : 256;
  if (!a.quantize) return launch_kernel<kv_write_kernel>(dim3((unsigned)a.ntok), dim3(256), 0, stream, "arcq_kv_write", p);
  const int64_t rows = a.ntok * 2 * a.N;
  const dim3 grid((unsigned)((rows + 15) / 16));
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<kv_quantize_kernel<true>>(grid, dim3(256), 0, stream, "arcq_kv_quantize", p);
  return launch_kernel<kv_quantize_kernel<false>>(grid, dim3(256), 0, stream, "arcq_kv_quantize", p);
}

// query heads of a kv head that share a workgroup's pass over its rows
static int kv_group_chunk(int64_t g) { return g == 1 ? 1 : g == 2 ? 2 : 4; }

// slices per sequence: enough workgroups for ~4 per CU while a wave keeps at least one 32-position block of an average sequence
int kv_decode_splits(int64_t B, int64_t Nq, int64_t N, int64_t nnz, int64_t P) {
  if (B <= 0 || Nq <= 0 || N <= 0 || nnz <= 0 || P <= 0) return 1;
  const int64_t g = Nq / N, gc = kv_group_chunk(g), chunks = (g + gc - 1) / gc;
  const int64_t avg = nnz * P / B;
  int64_t S = (1024 + B * N * chunks - 1) / (B * N * chunks);
  const int64_t cap = avg / (32 * kKvWaves);
  if (S > cap) S = cap;
  if (S > 32) S = 32;                                   // (kvstep.DecodeStepState sizes its record scratch for this cap: _MAX_SLICES)
  return S < 1 ? 1 : (int)S;
}

int64_t kv_decode_chunks(int64_t Nq, int64_t N) {
  const int64_t g = Nq / N, gc = kv_group_chunk(g);
  return (g + gc - 1) / gc;
}

template <typename Params>
static Params kv_decode_params(const KvDecodeArgs& a) {
  Params p{};
  p.o = a.o; p.q = a.q; p.data = (const uint8_t*)a.kv_data; p.param = (const uint32_t*)a.kv_param;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.ws = (float*)a.workspace;
  p.B = (int)a.B; p.Nq = (int)a.Nq; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.g = (int)(a.Nq / a.N);
  p.chunks = (int)kv_decode_chunks(a.Nq, a.N);
  p.S = kv_decode_splits(a.B, a.Nq, a.N, a.nnz, a.P);
  p.sm_scale = 0.08838834764831845f;                    // 128^-0.5
  return p;
}

// the kv_decode_kernel instantiation of a cache format, a 16-bit type and a group chunk
template <int FMT, bool STEP, int GC>
static int launch_kv_decode_gc(const typename KvParamsOf<STEP>::type& p, bool bf, const KvDecodeArgs& a, hipStream_t stream, const char* who) {
  const dim3 grid((unsigned)(a.B * a.N * p.chunks), (unsigned)p.S), block(kKvWaves * 64);
  if (bf) return launch_kernel<kv_decode_kernel<FMT, true, GC, STEP>>(grid, block, 0, stream, who, p);
  return launch_kernel<kv_decode_kernel<FMT, false, GC, STEP>>(grid, block, 0, stream, who, p);
}
template <int FMT, bool STEP>
static int launch_kv_decode(const typename KvParamsOf<STEP>::type& p, const KvDecodeArgs& a, hipStream_t stream, const char* who) {
  const int gc = kv_group_chunk(p.g);
  const bool bf = a.dtype == ARCQ_KV_BF16;
  if (gc == 1) return launch_kv_decode_gc<FMT, STEP, 1>(p, bf, a, stream, who);
  if (gc == 2) return launch_kv_decode_gc<FMT, STEP, 2>(p, bf, a, stream, who);
  return launch_kv_decode_gc<FMT, STEP, 4>(p, bf, a, stream, who);
}

int kv_decode_step(const KvDecodeArgs& a, const KvStepArgs& st, hipStream_t stream) {
  KvStepParams p = kv_decode_params<KvStepParams>(a);
  p.k = (const uint16_t*)st.k; p.v = (const uint16_t*)st.v; p.cnt = (int32_t*)st.state;
  p.q_stride = st.q_stride; p.kv_stride = st.kv_stride;
  return launch_kv_decode<ARCQ_KV_INT4, true>(p, a, stream, "arcq_kv_decode_step");
}

int kv_decode(const KvDecodeArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_decode";
  const KvDecodeParams p = kv_decode_params<KvDecodeParams>(a);
  const int rc = a.format == ARCQ_KV_INT4 ? launch_kv_decode<ARCQ_KV_INT4, false>(p, a, stream, who) : launch_kv_decode<ARCQ_KV_16BIT, false>(p, a, stream, who);
  if (rc != ARCQ_OK || p.S <= 1) return rc;
  const dim3 grid((unsigned)(a.B * a.Nq));
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<kv_decode_combine<true>>(grid, dim3(kKvD), 0, stream, who, p);
  return launch_kernel<kv_decode_combine<false>>(grid, dim3(kKvD), 0, stream, who, p);
}

}  // namespace arcq
