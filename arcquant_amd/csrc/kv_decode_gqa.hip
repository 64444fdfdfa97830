// Decode attention of one query token per sequence over the int4 pages of include/arcq_kv.h for GQA models (arcq_kv_batch_decode_gqa):
// the g <= 16 query heads of a kv head are the 16 columns of v_mfma_f32_16x16x32_{f16,bf16}, so every K and V row a workgroup reads is
// converted once, whatever g is, and there is no chunking over query heads.  DESIGN.md 11 "GQA decode on MFMA".
//
//   grid (B * N, S), 256 threads = 4 waves: a workgroup per (sequence, kv head, slice of the sequence).  The partition of the positions
//   is kv_decode_kernel's: 32-position blocks, a wave streams a contiguous range of them, the next block's loads are in flight while this
//   one is reduced.  S comes from kv_decode_gqa_splits (there are B * N workgroups per slice here, not B * N * chunks).
//
//   A lane is (i, c) = (lane % 16, lane / 16).  In every MFMA of the kernel column i of the B operand and of the result is query head i
//   (heads g .. 15 are zero columns and are never stored), and c is the k-group: the lane supplies k indices 8 c .. 8 c + 7.  The k index of
//   an MFMA may be permuted freely as long as both operands agree, and so may the row index of a result tile; both are used below.
//
//   Per block of 32 positions tb .. tb + 31 (two score tiles of 16):
//     tables    lanes l and l + 32 look up the row of position tb + l % 32 (clamped to T - 1: rows past the range are the sequence's last
//               valid row, masked) and load its (scale, zero) pair, K's in lanes 0-31 and V's in lanes 32-63: one page-table walk and one
//               parameter load per lane.  Row indices and pairs reach the lanes that need them by ds_bpermute (no LDS memory).
//     scores    S^T = C Q^T per tile u: lane (i, c) loads 16 bytes, codes 32 c .. 32 c + 31 of the K row of position tb + 16 u + i, and
//               feeds its four k-steps from them: step s is word s, whose nibbles 0..7 go out as the pairs (0, 4), (1, 5), (2, 6), (3, 7)
//               -- one shift and one mask per pair.  The Q fragment (registers, loaded once, 64 contiguous bytes per lane) is permuted the
//               same way.  No LDS.  Result register r of lane (i, c) is head i at position tb + 16 u + 4 c + r: eight positions per
//               lane, "slot" j = 4 u + r.   score = sm_scale log2(e) (s_t R - z_t sum_d q_d) in fp32; online softmax in base 2, the block
//               maximum of a head over the lane's eight slots and the four k-groups (two xor shuffles).
//     values    O^T += V^T W: the weights p_t s_t of lane (i, c), rounded once to the 16-bit type, ARE the B fragment of one 32-deep k-step
//               whose k index 8 c + j is slot j of k-group c: the weight tile does not move.  The A operand wants, in lane (i, c), eight
//               positions of ONE d.  V is stored [position][d], so the lane loads one dword -- codes 8 i .. 8 i + 7 -- of each of its
//               eight slot positions (the 16 lanes of a k-group read a whole 64-byte row) and MFMA m = 0..7 takes nibble m of the eight
//               dwords: its tile row i is d = 8 i + m.  The transposition is the load's addressing plus a nibble select; no LDS.
//               sum_t p_t z_t and the row sum are fp32 VALU sums over the unrounded weights.
//   Accumulator register r of tile m in lane (i, c) is O[d = 8 (4 c + r) + m][head i].  The waves merge through LDS (a record per wave and
//   head: 128 accumulators, max, sum); S == 1 stores o, S > 1 leaves kv_decode_kernel's records for kv_decode_combine.  No workgroup waits
//   for another, nothing is read on the host, there is no state.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"
#include "kv_gqa_device.hpp"

namespace arcq {

// the four pairs of one k-step from a word that holds them in nibbles (m, m + 4), m = 0..3
template <bool BF16>
__device__ __forceinline__ u32x4 gq_code_word(uint32_t w) {
  return u32x4{kv_code_pair<BF16>(w), kv_code_pair<BF16>(w >> 4), kv_code_pair<BF16>(w >> 8), kv_code_pair<BF16>(w >> 12)};
}

// what a lane holds of a block: 16 bytes of the K rows of tb + i and tb + 16 + i, one dword of the V rows of its eight slots, and the
// (scale, zero) pair of position tb + lane % 32 (K's in lanes 0-31, V's in lanes 32-63)
struct GqBlock {
  u32x4 k[2];
  uint32_t v[8];
  uint32_t prm;
};

template <bool BF16>
__global__ __launch_bounds__(kGqWaves * 64) void kv_decode_gqa_kernel(KvGqaParams p) {
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

  // ---- this lane's query head: elements 32 c .. 32 c + 31, each k-step's eight in the order 0, 4, 1, 5, 2, 6, 3, 7 (a head past the
  //      group is a zero column: nothing of q is read for it)
  const bool head = i < p.g;
  u32x4 qf[4];
  float qsum = 0.f;
  {
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(p.q) + ((size_t)b * p.Nq + (size_t)n * p.g + i) * kKvD + c * 32;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (head) w = *reinterpret_cast<const u32x4*>(qrow + ks * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) qsum += kv_to_f32<BF16>(w[j] & 0xffffu) + kv_to_f32<BF16>(w[j] >> 16);
      qf[ks] = u32x4{(w[0] & 0xffffu) | (w[2] << 16), (w[0] >> 16) | (w[2] & 0xffff0000u), (w[1] & 0xffffu) | (w[3] << 16),
                        (w[1] >> 16) | (w[3] & 0xffff0000u)};
    }
  }
  const float nqsum = -kv_row_sum<kGqShare>(qsum);

  // slot j of this lane is position tb + slot[j] of the block; the lanes that looked that position up are slot[j] (K) and 32 + slot[j] (V)
  int slot[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) slot[j] = (j >> 2) * 16 + c * 4 + (j & 3);

  auto load_block = [&](int tb, GqBlock& x) __attribute__((always_inline)) {
    const int pos = min(tb + (lane & 31), T - 1);       // past the range: the sequence's last valid row, masked below
    const size_t row = kv_row(p.t, b, n, pos, p.L, p.layer, p.N, p.P);
    x.prm = p.param[row + (lane >> 5 ? vrows : (size_t)0)];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t r = gq_row_of(row, u * 16 + i);
      x.k[u] = *reinterpret_cast<const u32x4*>(p.data + r * 64 + c * 16);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t r = gq_row_of(row, slot[j]) + vrows;
      x.v[j] = *reinterpret_cast<const uint32_t*>(p.data + r * 64 + i * 4);
    }
  };

  f32x4 acc[8];
#pragma unroll
  for (int m8 = 0; m8 < 8; ++m8) acc[m8] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = kKvIdle, l = 0.f, zacc = 0.f;               // m: of head i, the same in the four k-groups; l, zacc: this lane's slots

  auto consume = [&](int tb, const GqBlock& x) __attribute__((always_inline)) {
    // ---- scores of head i at the lane's eight slots
    f32x4 sc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) sc[u] = kv_mfma16<BF16>(gq_code_word<BF16>(x.k[u][ks]), qf[ks], sc[u]);
    }
    float sv[8], vs[8], vz[8];
    bool ok[8];
    float mb = kKvIdle;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t pk = __shfl(x.prm, slot[j], 64), pv = __shfl(x.prm, 32 + slot[j], 64);
      const float ksc = kv_to_f32<false>(pk & 0xffffu) * p.sm_scale, kzr = kv_to_f32<false>(pk >> 16) * p.sm_scale;
      vs[j] = kv_to_f32<false>(pv & 0xffffu);
      vz[j] = kv_to_f32<false>(pv >> 16);
      ok[j] = tb + slot[j] < t1;
      const float val = fmaf(kzr, nqsum, ksc * sc[j >> 2][j & 3]);
      sv[j] = ok[j] ? val : kKvIdle;
      mb = fmaxf(mb, sv[j]);
    }
    kv_new_max<kGqShare>(mb, m, l, acc, zacc);
    // ---- weights: p_t s_t rounded once, the B fragment as it stands
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pt = ok[j] ? __builtin_amdgcn_exp2f(sv[j] - m) : 0.f;
      l += pt;
      zacc = fmaf(pt, vz[j], zacc);
      w[j] = pt * vs[j];
    }
    const u32x4 wf = kv_pack8<BF16>(w);
    // ---- values: z0[q] / z1[q] hold nibbles 0-3 / 4-7 of slots 2 q (low half) and 2 q + 1 (high half)
    uint32_t z0[4], z1[4];
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
      z0[q2] = (x.v[2 * q2] & 0xffffu) | (x.v[2 * q2 + 1] << 16);
      z1[q2] = (x.v[2 * q2] >> 16) | (x.v[2 * q2 + 1] & 0xffff0000u);
    }
#pragma unroll
    for (int m8 = 0; m8 < 8; ++m8) {
      const int sh = 4 * (m8 & 3);
      u32x4 a;
#pragma unroll
      for (int q2 = 0; q2 < 4; ++q2) a[q2] = kv_code_pair<BF16>((m8 < 4 ? z0[q2] : z1[q2]) >> sh);
      acc[m8] = kv_mfma16<BF16>(a, wf, acc[m8]);
    }
  };

  if (t0 < t1) {
    GqBlock x0, x1;
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

  // ---- the wave's record per head: the k-groups' sums joined, the zero sum taken off
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  zacc += __shfl_xor(zacc, 16, 64);
  zacc += __shfl_xor(zacc, 32, 64);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const f32x4 v = {acc[hf * 4][r] - zacc, acc[hf * 4 + 1][r] - zacc, acc[hf * 4 + 2][r] - zacc, acc[hf * 4 + 3][r] - zacc};
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
    } else {                                            // kv_decode_kernel's record: its maximum is a natural-log score
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
// Slices per sequence: a slice is B * N workgroups here (no chunks over the query heads), so enough of them for ~4 workgroups per CU
// while a wave keeps at least one 32-position block of an average sequence
int kv_decode_gqa_splits(int64_t B, int64_t Nq, int64_t N, int64_t nnz, int64_t P) {
  if (B <= 0 || Nq <= 0 || N <= 0 || nnz <= 0 || P <= 0) return 1;
  const int64_t avg = nnz * P / B;
  int64_t S = (1024 + B * N - 1) / (B * N);
  const int64_t cap = avg / (kGqBlk * kGqWaves);
  if (S > cap) S = cap;
  if (S > kGqMaxSlices) S = kGqMaxSlices;
  return S < 1 ? 1 : (int)S;
}

int kv_decode_gqa(const KvDecodeArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_decode_gqa";
  KvGqaParams p{};
  kv_gqa_fill(p, a);
  p.param = (const uint32_t*)a.kv_param;
  const dim3 grid = kv_gqa_grid(p, a), block(kGqWaves * 64);
  const int rc = a.dtype == ARCQ_KV_BF16 ? launch_kernel<kv_decode_gqa_kernel<true>>(grid, block, 0, stream, who, p)
                                         : launch_kernel<kv_decode_gqa_kernel<false>>(grid, block, 0, stream, who, p);
  if (rc != ARCQ_OK || p.S <= 1) return rc;
  return kv_decode_combine_slices(a, p.S, stream, who);
}

}  // namespace arcq
