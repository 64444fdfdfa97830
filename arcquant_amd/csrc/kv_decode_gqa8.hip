// Decode attention of one query token per sequence over the FP8 (OCP e4m3) pages of include/arcq_kv.h for GQA models
// (arcq_kv_batch_decode_gqa_fp8): kv_decode_gqa16.hip's grid, slices, wave ranges, LDS merge and records over rows of 128 BYTES -- one cache
// line -- whose codes are converted to q's 16-bit type in registers (v_cvt_scalef32_pk_{f16,bf16}_fp8, two codes an instruction, exact) on
// their way into the same 16-bit MFMA.  The row scales never touch an element: K's multiplies the fp32 score, V's the fp32 weight.
// DESIGN.md 11 "FP8 cache".
//
//   grid (B * N, S), 256 threads = 4 waves, at most 168 VGPRs (three workgroups per CU: a block in flight is half the 16-bit kernel's
//   bytes, so more waves than its two workgroups keep the bytes under way; 166 VGPRs, no scratch).  A workgroup per (sequence, kv head,
//   slice); 32-position blocks; a wave streams a contiguous range of them with the next block's 8 KB in flight while this one is reduced.
//   S comes from kv_decode_gqa_splits: the rule counts workgroups and blocks, and both are the other GQA kernels'.
//
//   A lane is (i, c) = (lane % 16, lane / 16).  Column i of every B operand and of every result is query head i (heads g .. 15 are zero
//   columns, never loaded, never stored); c is the k-group, the lane supplies k indices 8 c .. 8 c + 7 of v_mfma_f32_16x16x32_{f16,bf16}.
//
//   Per block of 32 positions tb .. tb + 31 (two score tiles of 16):
//     tables    lane l % 32 looks up the row of position tb + l % 32 (clamped to T - 1, masked) and loads that row's two parameter words;
//               row indices and the (K scale, V scale) pair reach the lanes that need them by ds_bpermute.
//     scores    S^T = K Q^T per tile u.  Lane (i, c) loads the 16 bytes d = 64 h + 16 c .. + 15 (h = 0, 1) of the K row of position
//               tb + 16 u + i: two load instructions cover the row's line, the four lanes of a row read 64 contiguous bytes in each (four
//               lanes times the widest load are 64 bytes: a line cannot be one instruction in this lane map).  A 16-byte load is TWO
//               k-steps: dwords 2 e, 2 e + 1 convert to the eight 16-bit values d = 64 h + 16 c + 8 e .. + 7 of k-step 2 h + e, and the Q
//               fragment (registers, loaded once) takes the same d.  Result register r of lane (i, c) is head i at position
//               tb + 16 u + 4 c + r: "slot" j = 4 u + r.  score = (128^-1/2 log2(e) scale_k[t]) * s in fp32, one multiply per element.
//     softmax   base 2, online.  The weight that goes to the matrix cores is w_t scale_v[t], rounded once to 16 bits.  So that a small
//               scale_v cannot push it into fp16's subnormal range the running maximum is taken over score + e_t, e_t the exponent of
//               scale_v[t] (an integer: exact): x = exp2(score + e_t - m) <= 1, the rounded weight is x * (scale_v[t] 2^-e_t) in [0, 2) --
//               the largest one of a head is in [1, 2), as the 16-bit kernel's is 1 -- and the row sum takes x * 2^-e_t, the unscaled
//               weight to the same maximum.  Both factors are powers of two or exact products: nothing is rounded but x and the weight.
//     values    O^T += V^T W with the weights as the B fragment of one 32-deep k-step (k index 8 c + j is slot j).  The A operand wants
//               eight positions of ONE d: the lane loads the 8 bytes d = 8 i .. 8 i + 7 of each of its eight slot rows (the 16 lanes of a
//               k-group read one whole 128-byte row per instruction); v_perm_b32 puts bytes (m, m + 1) of slots 2 q and 2 q + 1 side by
//               side, and the conversion of the low or high half of that dword is register q of tile m = d - 8 i: the transposition is
//               the load's addressing, one byte select per two tiles and the conversion's half select -- no LDS.
//   Accumulator register r of tile m in lane (i, c) is O[d = 8 (4 c + r) + m][head i], as in the other two GQA kernels, and so are the
//   merge of the waves through LDS records, the direct store (S == 1) and kv_decode_kernel's records for kv_decode_combine (S > 1); the
//   record's maximum is a reference point only, so score + e_t serves as well as the score.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"
#include "kv_gqa_device.hpp"

namespace arcq {

constexpr int kG8RowBytes = kKvD;

// what a lane holds of a block: per score tile u its two 16-byte pieces of the K row of tb + 16 u + i, 8 bytes of the V row of each of
// its eight slots, and (lane % 32's position) the row's K and V parameter words -- 34 VGPRs
struct G8Block {
  u32x4 k[2][2];
  u32x2 v[8];
  uint32_t pk, pv;
};

// the two e4m3 codes in the low (HI: high) half of x as two packed 16-bit values: exact
template <bool BF16, bool HI>
__device__ __forceinline__ uint32_t kv_fp8_pair(uint32_t x) {
  if constexpr (BF16) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(x, 1.0f, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(x, 1.0f, HI));
}
// eight codes (two dwords) as one operand fragment
template <bool BF16>
__device__ __forceinline__ u32x4 kv_fp8_frag(uint32_t lo, uint32_t hi) {
  return u32x4{kv_fp8_pair<BF16, false>(lo), kv_fp8_pair<BF16, true>(lo), kv_fp8_pair<BF16, false>(hi), kv_fp8_pair<BF16, true>(hi)};
}

template <bool BF16>
__global__ __launch_bounds__(kGqWaves * 64, 3) void kv_decode_gqa8_kernel(KvGqaParams p) {
  __shared__ __attribute__((aligned(16))) float rec[kGqWaves][kGqHeads][kGqRecStride];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, c = lane >> 4;
  const int b = blockIdx.x / p.N, n = blockIdx.x - b * p.N;
  const int s = blockIdx.y;
  const int T = max(kv_seq_len(p.t, b, p.P), 0);
  const int nblk = (T + kGqBlk - 1) / kGqBlk, units = p.S * kGqWaves;
  const int per = (nblk + units - 1) / units;
  const int t0 = min(T, (s * kGqWaves + wave) * per * kGqBlk), t1 = min(T, t0 + per * kGqBlk);
  const size_t vrows = (size_t)p.N * p.P;

  // ---- this lane's query head: k-step ks = 2 h + e is elements 64 h + 16 c + 8 e .. + 7 (a head past the group is a zero column)
  u32x4 qf[4];
  {
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(p.q) + ((size_t)b * p.Nq + (size_t)n * p.g + i) * kKvD + c * 16;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = u32x4{0u, 0u, 0u, 0u};
      if (i < p.g) qf[ks] = *reinterpret_cast<const u32x4*>(qrow + (ks >> 1) * 64 + (ks & 1) * 8);
    }
  }

  // slot j of this lane is position tb + slot[j] of the block, looked up by lane slot[j]
  int slot[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) slot[j] = (j >> 2) * 16 + c * 4 + (j & 3);

  auto load_block = [&](int tb, G8Block& x) __attribute__((always_inline)) {
    const int pos = min(tb + (lane & 31), T - 1);       // past the range: the sequence's last valid row, masked below
    const size_t row = kv_row(p.t, b, n, pos, p.L, p.layer, p.N, p.P);
    x.pk = p.param[row];
    x.pv = p.param[row + vrows];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t r = gq_row_of(row, u * 16 + i);
      const uint8_t* krow = p.data + r * kG8RowBytes + c * 16;
#pragma unroll
      for (int h = 0; h < 2; ++h) x.k[u][h] = *reinterpret_cast<const u32x4*>(krow + h * 64);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t r = gq_row_of(row, slot[j]) + vrows;
      x.v[j] = *reinterpret_cast<const u32x2*>(p.data + r * kG8RowBytes + i * 8);
    }
  };

  f32x4 acc[8];
#pragma unroll
  for (int m8 = 0; m8 < 8; ++m8) acc[m8] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = kKvIdle, l = 0.f;                           // m: of head i, the same in the four k-groups; l: this lane's slots

  auto consume = [&](int tb, const G8Block& x) __attribute__((always_inline)) {
    // ---- scores of head i at the lane's eight slots: a 16-byte piece is two k-steps
    f32x4 sc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 2; ++e) sc[u] = kv_mfma16<BF16>(kv_fp8_frag<BF16>(x.k[u][h][2 * e], x.k[u][h][2 * e + 1]), qf[2 * h + e], sc[u]);
    }
    // ---- the slots' scales: (K scale, V scale) as one word from the lane that loaded them
    const uint32_t pair = __builtin_amdgcn_perm(x.pv, x.pk, 0x05040100u);
    uint32_t pr[8];
    float sv[8];
    float mb = kKvIdle;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pr[j] = (uint32_t)__shfl((int)pair, slot[j], 64);
      const float ks = kv_to_f32<false>(pr[j] & 0xffffu) * p.sm_scale;
      const int ev = __builtin_amdgcn_frexp_expf(kv_to_f32<false>(pr[j] >> 16)) - 1;   // scale_v = f 2^ev, 1 <= f < 2 (0: ev = -1, f = 0)
      sv[j] = tb + slot[j] < t1 ? sc[j >> 2][j & 3] * ks + (float)ev : kKvIdle;
      mb = fmaxf(mb, sv[j]);
    }
    kv_new_max<kGqShare>(mb, m, l, acc);
    // ---- weights: x to the maximum of score + ev; the row sum takes x 2^-ev (the unscaled weight), the B fragment (x 2^-ev) scale_v
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float vs = kv_to_f32<false>(pr[j] >> 16);
      const int ev = __builtin_amdgcn_frexp_expf(vs) - 1;
      const float wu = tb + slot[j] < t1 ? __builtin_ldexpf(__builtin_amdgcn_exp2f(sv[j] - m), -ev) : 0.f;
      l += wu;
      w[j] = wu * vs;
    }
    const u32x4 wf = kv_pack8<BF16>(w);
    // ---- values: bytes (2 mp, 2 mp + 1) of word wd of slots 2 q2 and 2 q2 + 1 side by side; tiles 4 wd + 2 mp and + 1 convert a half each
#pragma unroll
    for (int wd = 0; wd < 2; ++wd)
#pragma unroll
      for (int mp = 0; mp < 2; ++mp) {
        uint32_t t[4];
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) t[q2] = __builtin_amdgcn_perm(x.v[2 * q2 + 1][wd], x.v[2 * q2][wd], mp ? 0x07030602u : 0x05010400u);
        const int m8 = wd * 4 + mp * 2;
        const u32x4 a0 = {kv_fp8_pair<BF16, false>(t[0]), kv_fp8_pair<BF16, false>(t[1]), kv_fp8_pair<BF16, false>(t[2]), kv_fp8_pair<BF16, false>(t[3])};
        const u32x4 a1 = {kv_fp8_pair<BF16, true>(t[0]), kv_fp8_pair<BF16, true>(t[1]), kv_fp8_pair<BF16, true>(t[2]), kv_fp8_pair<BF16, true>(t[3])};
        acc[m8] = kv_mfma16<BF16>(a0, wf, acc[m8]);
        acc[m8 + 1] = kv_mfma16<BF16>(a1, wf, acc[m8 + 1]);
      }
  };

  if (t0 < t1) {
    G8Block x0, x1;
    load_block(t0, x0);
    for (int tb = t0; tb < t1; tb += 2 * kGqBlk) {      // two blocks per trip: the other buffer's loads stay in flight
      if (tb + kGqBlk < t1) load_block(tb + kGqBlk, x1);
      consume(tb, x0);
      if (tb + kGqBlk < t1) {
        if (tb + 2 * kGqBlk < t1) load_block(tb + 2 * kGqBlk, x0);
        consume(tb + kGqBlk, x1);
      }
    }
  }

  // ---- the wave's record per head: the k-groups' sums joined
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const f32x4 v = {acc[hf * 4][r], acc[hf * 4 + 1][r], acc[hf * 4 + 2][r], acc[hf * 4 + 3][r]};
      *reinterpret_cast<f32x4*>(&rec[wave][i][(c * 4 + r) * 8 + hf * 4]) = v;
    }
  if (c == 0) {
    rec[wave][i][kKvD] = m;
    rec[wave][i][kKvD + 1] = l;
  }
  __syncthreads();
  // ---- merge of the waves (idle ones carry m = kKvIdle, l = 0): thread (h, d), two heads at a time
  const int d = tid & (kKvD - 1);
  for (int h = tid >> 7; h < p.g; h += 2) {
    float M = kKvIdle;
#pragma unroll
    for (int w = 0; w < kGqWaves; ++w) M = fmaxf(M, rec[w][h][kKvD]);
    float Ls = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < kGqWaves; ++w) {
      const float f = __builtin_amdgcn_exp2f(rec[w][h][kKvD] - M);
      Ls += rec[w][h][kKvD + 1] * f;
      a += rec[w][h][d] * f;
    }
    const size_t bh = (size_t)b * p.Nq + (size_t)n * p.g + h;
    if (p.S == 1) {
      reinterpret_cast<uint16_t*>(p.o)[bh * kKvD + d] = (uint16_t)kv_from_f32<BF16>(Ls > 0.f ? a / Ls : 0.f);
    } else {                                            // kv_decode_kernel's record: its maximum is a natural-log reference point
      float* o = p.ws + (bh * p.S + s) * kKvRec;
      o[2 + d] = a;
      if (d == 0) {
        o[0] = M * kKvLn2;
        o[1] = Ls;
      }
    }
  }
}

// ---- launcher (arguments validated by c_api_kv.hip)
int kv_decode_gqa8(const KvDecodeArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_decode_gqa_fp8";
  KvGqaParams p{};
  kv_gqa_fill(p, a);
  p.param = (const uint32_t*)a.kv_param;
  const dim3 grid = kv_gqa_grid(p, a), block(kGqWaves * 64);
  const int rc = a.dtype == ARCQ_KV_BF16 ? launch_kernel<kv_decode_gqa8_kernel<true>>(grid, block, 0, stream, who, p)
                                         : launch_kernel<kv_decode_gqa8_kernel<false>>(grid, block, 0, stream, who, p);
  if (rc != ARCQ_OK || p.S <= 1) return rc;
  return kv_decode_combine_slices(a, p.S, stream, who);
}

}  // namespace arcq
