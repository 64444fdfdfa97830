// Decode attention of one query token per sequence over the 16-bit pages of include/arcq_kv.h for GQA models
// (arcq_kv_batch_decode_gqa_16bit): kv_decode_gqa.hip's work split and lane roles over rows of 256 bytes that are MFMA operands as they
// stand -- no codes to convert, no (scale, zero), no sum of q.  DESIGN.md 11 "GQA decode over a 16-bit cache".
//
//   grid (B * N, S), 256 threads = 4 waves, at most 256 VGPRs (two workgroups per CU).  A workgroup per (sequence, kv head, slice); 32-
//   position blocks; a wave streams a contiguous range of them with the next block's 16 KB in flight while this one is reduced.  S comes
//   from kv_decode_gqa_splits: the rule counts workgroups and blocks, and both are the int4 kernel's.
//
//   A lane is (i, c) = (lane % 16, lane / 16).  Column i of every B operand and of every result is query head i (heads g .. 15 are zero
//   columns, never loaded, never stored); c is the k-group, the lane supplies k indices 8 c .. 8 c + 7 of v_mfma_f32_16x16x32_{f16,bf16}.
//
//   Per block of 32 positions tb .. tb + 31 (two score tiles of 16):
//     tables    lane l % 32 looks up the row of position tb + l % 32 (clamped to T - 1: rows past the range are the sequence's last valid
//               row, masked); the row indices reach the lanes that load them by ds_bpermute.  One page-table walk per position.
//     scores    S^T = K Q^T per tile u, four k-steps.  k-step s of lane (i, c) is the 16 bytes d = 32 s + 8 c .. + 7 of the K row of
//               position tb + 16 u + i, as loaded: in every load instruction the four lanes of a row read 64 contiguous bytes, half a
//               128-byte line, so an instruction touches 16 lines (the lane's own 64 contiguous bytes, d = 32 c .., would touch both
//               lines of all 16 rows in each of the four instructions).  The Q fragment (registers, loaded once) takes the same d.  Result
//               register r of lane (i, c) is head i at position tb + 16 u + 4 c + r: "slot" j = 4 u + r.  score = 128^-1/2 log2(e) s in
//               fp32; online softmax in base 2, the block maximum of a head over the lane's eight slots and the four k-groups.
//     values    O^T += V^T W: the weights of lane (i, c), rounded once to the 16-bit type, ARE the B fragment of one 32-deep k-step whose
//               k index 8 c + j is slot j of k-group c.  The A operand wants eight positions of ONE d in a lane: the lane loads the 16
//               bytes d = 8 i .. 8 i + 7 of each of its eight slot rows (the 16 lanes of a k-group read one whole 256-byte row) and
//               MFMA m = 0..7 takes half-word m of the eight vectors, two to a v_perm_b32: its tile row i is d = 8 i + m.  The
//               transposition is the load's addressing plus a half-word select; no LDS.  The row sum is over the unrounded weights.
//   Accumulator register r of tile m in lane (i, c) is O[d = 8 (4 c + r) + m][head i], as in the int4 kernel, and so are the merge of
//   the waves through LDS records, the direct store (S == 1) and kv_decode_kernel's records for kv_decode_combine (S > 1).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"
#include "kv_gqa_device.hpp"

namespace arcq {

constexpr int kG16RowBytes = kKvD * 2;

// what a lane holds of a block: per score tile u and k-step s 16 bytes of the K row of tb + 16 u + i, and 16 bytes of the V row of each
// of its eight slots -- 64 VGPRs
struct G16Block {
  u32x4 k[2][4];
  u32x4 v[8];
};

template <bool BF16>
__global__ __launch_bounds__(kGqWaves * 64, 2) void kv_decode_gqa16_kernel(KvGqaParams p) {
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

  // ---- this lane's query head: k-step ks is elements 32 ks + 8 c .. + 7 (a head past the group is a zero column: nothing is read)
  u32x4 qf[4];
  {
    const uint16_t* qrow = reinterpret_cast<const uint16_t*>(p.q) + ((size_t)b * p.Nq + (size_t)n * p.g + i) * kKvD + c * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = u32x4{0u, 0u, 0u, 0u};
      if (i < p.g) qf[ks] = *reinterpret_cast<const u32x4*>(qrow + ks * 32);
    }
  }

  // slot j of this lane is position tb + slot[j] of the block, looked up by lane slot[j]
  int slot[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) slot[j] = (j >> 2) * 16 + c * 4 + (j & 3);

  auto load_block = [&](int tb, G16Block& x) __attribute__((always_inline)) {
    const int pos = min(tb + (lane & 31), T - 1);       // past the range: the sequence's last valid row, masked below
    const size_t row = kv_row(p.t, b, n, pos, p.L, p.layer, p.N, p.P);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t r = gq_row_of(row, u * 16 + i);
      const uint8_t* krow = p.data + r * kG16RowBytes + c * 16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) x.k[u][ks] = *reinterpret_cast<const u32x4*>(krow + ks * 64);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const size_t r = gq_row_of(row, slot[j]) + vrows;
      x.v[j] = *reinterpret_cast<const u32x4*>(p.data + r * kG16RowBytes + i * 16);
    }
  };

  f32x4 acc[8];
#pragma unroll
  for (int m8 = 0; m8 < 8; ++m8) acc[m8] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = kKvIdle, l = 0.f;                           // m: of head i, the same in the four k-groups; l: this lane's slots

  auto consume = [&](int tb, const G16Block& x) __attribute__((always_inline)) {
    // ---- scores of head i at the lane's eight slots
    f32x4 sc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      sc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) sc[u] = kv_mfma16<BF16>(x.k[u][ks], qf[ks], sc[u]);
    }
    float sv[8];
    bool ok[8];
    float mb = kKvIdle;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ok[j] = tb + slot[j] < t1;
      sv[j] = ok[j] ? sc[j >> 2][j & 3] * p.sm_scale : kKvIdle;
      mb = fmaxf(mb, sv[j]);
    }
    kv_new_max<kGqShare>(mb, m, l, acc);
    // ---- weights: rounded once, the B fragment as it stands
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w[j] = ok[j] ? __builtin_amdgcn_exp2f(sv[j] - m) : 0.f;
      l += w[j];
    }
    const u32x4 wf = kv_pack8<BF16>(w);
    // ---- values: tile m8's fragment is half-word m8 of the eight slot vectors, slots 2 q (low half) and 2 q + 1 (high half) to a register
#pragma unroll
    for (int m8 = 0; m8 < 8; ++m8) {
      u32x4 a;
#pragma unroll
      for (int q2 = 0; q2 < 4; ++q2) a[q2] = __builtin_amdgcn_perm(x.v[2 * q2 + 1][m8 >> 1], x.v[2 * q2][m8 >> 1], m8 & 1 ? 0x07060302u : 0x05040100u);
      acc[m8] = kv_mfma16<BF16>(a, wf, acc[m8]);
    }
  };

  if (t0 < t1) {
    G16Block x0, x1;
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

// ---- launcher (arguments validated by c_api_kv.hip; a.kv_param is not read)
int kv_decode_gqa16(const KvDecodeArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_decode_gqa_16bit";
  KvGqaParams p{};
  kv_gqa_fill(p, a);
  const dim3 grid = kv_gqa_grid(p, a), block(kGqWaves * 64);
  const int rc = a.dtype == ARCQ_KV_BF16 ? launch_kernel<kv_decode_gqa16_kernel<true>>(grid, block, 0, stream, who, p)
                                         : launch_kernel<kv_decode_gqa16_kernel<false>>(grid, block, 0, stream, who, p);
  if (rc != ARCQ_OK || p.S <= 1) return rc;
  return kv_decode_combine_slices(a, p.S, stream, who);
}

}  // namespace arcq
