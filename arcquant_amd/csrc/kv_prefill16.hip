// Causal prefill attention over the 16-bit pages of include/arcq_kv.h (arcq_kv_batch_prefill_16bit) on v_mfma_f32_32x32x16_{f16,bf16}.
//
//   The work split and the MFMA roles are kv_prefill.hip's and are described in kv_prefill_device.hpp, with the LDS strides as far as the
//   fragment reads go.  What is this kernel's own, per block of 32 kv positions:
//     staging   a block is 32 K rows and 32 V rows of 256 bytes: 1024 pieces of 16 bytes, four per thread, and ALL four waves stage.
//               Thread (rp, vc) takes the 16 bytes vc of rows 2 rp and 2 rp + 1, of K and of V: one pair of page lookups serves the four
//               loads, and four adjacent lanes read 64 contiguous bytes.  The pieces are loaded one block ahead into registers.  Rows
//               past T are never loaded (the position clamps to T - 1); the (page slot, entry) of a thread's rows is carried from block
//               to block, so the loop holds no division.
//               K goes to LDS as [position][d], one 16-byte write per piece.  V goes transposed as [d][position'] with position' =
//               position with bits 2 and 3 swapped (the k order in which the score tile presents its rows): the thread's two rows are
//               adjacent in that order too, so element e of both is one packed pair and one 32-bit write into row 8 vc + e.
//     scores    score = sm_scale * s in fp32 with sm_scale = 128^-1/2 log2(e): the softmax runs in base 2.
//   The stores are of O / l.
//
//   LDS strides and the staging writes.  K rows are 68 banks apart and 16 fragment reads of consecutive i cover the 64 banks once
//   (kv_prefill_device.hpp); the staging writes of four lanes fill 64 contiguous bytes and the lanes are ordered so that 16 consecutive
//   ones write rows 4 apart -- the same cover.  V^T rows are 20 banks apart.  A
//   wave's 32-bit V^T writes go to banks 32 vc + 20 e + tp: tp takes 16 consecutive values, 32 vc only two, so the lanes whose vc has bit 1 set
//   write their eight pairs in the order 4..7, 0..3 -- 20 * 4 = 16 (mod 64) moves them into the banks the others leave free.
//
// There is no split over the kv range: few query tokens over a long cache run on B * N workgroups (arcq_kv.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"
#include "kv_prefill_device.hpp"

namespace arcq {

constexpr int kP16RowBytes = kKvD * 2;

struct KvPrefill16Params {
  void* o;
  const void* q;
  const int32_t* qo_indptr;
  const uint8_t* data;
  KvTables t;
  int B, Nq, L, layer, N, P, g, hc, tpt, chunks;
  float sm_scale;
};

// what a thread holds of the next block: the 16 bytes vc of K rows 2 rp, 2 rp + 1 and of V rows 2 rp, 2 rp + 1
struct P16Stage {
  u32x4 ka, kb, va, vb;
};

template <bool BF16>
__global__ __launch_bounds__(256, 2) void kv_prefill16_kernel(KvPrefill16Params p) {
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[kPfBlk * kPfKStride];
  __shared__ __attribute__((aligned(16))) uint16_t v_lds[kKvD * kPfVStride];

  // ---- this workgroup's (sequence, tile) or nothing
  int x = blockIdx.x, b = 0, q0 = 0, nb = 0;
  for (; b < p.B; ++b) {
    q0 = p.qo_indptr[b];
    nb = p.qo_indptr[b + 1] - q0;
    const int nt = (nb + p.tpt - 1) / p.tpt;
    if (x < nt) break;
    x -= nt;
  }
  if (b >= p.B) return;
  const int T = kv_seq_len(p.t, b, p.P);
  if (T <= 0 || nb > T) return;                         // (outside the contract: nothing is read or written)
  const int n = blockIdx.y / p.chunks, ch = blockIdx.y - n * p.chunks;
  const int tok0 = x * p.tpt;                           // first token of the tile inside the sequence
  const int base = T - nb;                              // position of the sequence's first query token
  const int tile_last = base + min(nb, tok0 + p.tpt) - 1;              // the tile's causal limit
  const int nblk = tile_last / kPfBlk + 1;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5;

  // ---- this lane's query row
  const int slot = wave * 32 + i;
  const int tl = slot / p.hc, head = ch * p.hc + (slot - tl * p.hc);
  const int tok = tok0 + tl;
  const bool valid = tl < p.tpt && head < p.g && tok < nb;
  const int qpos = valid ? base + tok : -1;
  // the wave's own causal limit (-1: no token of the tile falls into its slots)
  const int wtl0 = (wave * 32) / p.hc, wtl1 = min((wave * 32 + 31) / p.hc, p.tpt - 1);
  const int wave_last = (wtl0 < p.tpt && tok0 + wtl0 < nb) ? base + min(tok0 + wtl1, nb - 1) : -1;
  const size_t orow = ((size_t)(q0 + tok) * p.Nq + (size_t)n * p.g + head) * kKvD;

  u32x4 qf[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = u32x4{0u, 0u, 0u, 0u};
    if (valid) qf[ks] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(p.q) + orow + ks * 16 + h * 8);
  }

  // ---- staging role: piece vc (16 bytes = 8 d) of rows 2 rp and 2 rp + 1.  Lanes 0..3 of a quad take adjacent pieces; the quads of a
  //      wave take the 16 row pairs, ordered so that 16 consecutive lanes hold rows 4 apart (K's LDS writes, see the top)
  const int vc = wave * 4 + (lane & 3);
  const int u = lane >> 2;
  const int rp = ((u & 3) << 1) | ((u >> 2) & 1) | (u & 8);
  const int r0 = 2 * rp;
  const int tp = (rp & 9) | ((rp & 2) << 1) | ((rp & 4) >> 1);          // the pair's place in position' order: bits 1 and 2 of rp swapped
  // (page slot, entry) of position tb + r0, carried from block to block; those of T - 1, where the loads clamp
  const int d32 = kPfBlk / p.P, r32 = kPfBlk - d32 * p.P;
  const int pgT = (T - 1) / p.P, eT = (T - 1) - pgT * p.P;
  int pg = r0 / p.P, en = r0 - pg * p.P;
  const int32_t* own = p.t.indices + p.t.indptr[b];                     // the sequence's pages
  const size_t page_rows = (size_t)p.L * 2 * p.N * p.P, v_rows = (size_t)p.N * p.P;
  const size_t head_row = ((size_t)p.layer * 2 * p.N + n) * p.P;
  auto fetch = [&](int tb, P16Stage& s) __attribute__((always_inline)) {
    int pa = pg, ea = en, pb = pg, eb = en + 1;
    if (eb == p.P) {
      eb = 0;
      ++pb;
    }
    if (tb + r0 >= T - 1) {
      pa = pgT;
      ea = eT;
    }
    if (tb + r0 + 1 >= T - 1) {
      pb = pgT;
      eb = eT;
    }
    const uint8_t* ra = p.data + ((size_t)own[pa] * page_rows + head_row + ea) * kP16RowBytes + vc * 16;
    const uint8_t* rb = p.data + ((size_t)own[pb] * page_rows + head_row + eb) * kP16RowBytes + vc * 16;
    s.ka = *reinterpret_cast<const u32x4*>(ra);
    s.kb = *reinterpret_cast<const u32x4*>(rb);
    s.va = *reinterpret_cast<const u32x4*>(ra + v_rows * kP16RowBytes);
    s.vb = *reinterpret_cast<const u32x4*>(rb + v_rows * kP16RowBytes);
    en += r32;                                                          // en, r32 < P: one correction
    pg += d32;
    if (en >= p.P) {
      en -= p.P;
      ++pg;
    }
  };
  const bool flip = (vc >> 1) & 1;
  uint16_t* const kdst = &k_lds[r0 * kPfKStride + vc * 8];
  uint16_t* const vdst = &v_lds[(vc * 8) * kPfVStride + 2 * tp];
  uint16_t* const vdst_lo = vdst + (flip ? 4 * kPfVStride : 0);        // where the first four writes go, and the last four
  uint16_t* const vdst_hi = vdst + (flip ? 0 : 4 * kPfVStride);
  auto stage = [&](const P16Stage& s) __attribute__((always_inline)) {
    *reinterpret_cast<u32x4*>(kdst) = s.ka;
    *reinterpret_cast<u32x4*>(kdst + kPfKStride) = s.kb;
    uint32_t pair[8];                                                   // element e of row 2 rp (low half) and of row 2 rp + 1
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pair[2 * j] = (s.va[j] & 0xffffu) | (s.vb[j] << 16);
      pair[2 * j + 1] = (s.va[j] >> 16) | (s.vb[j] & 0xffff0000u);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<uint32_t*>(vdst_lo + e * kPfVStride) = flip ? pair[e + 4] : pair[e];
      *reinterpret_cast<uint32_t*>(vdst_hi + e * kPfVStride) = flip ? pair[e] : pair[e + 4];
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m = kKvIdle, l = 0.f;

  P16Stage st;
  fetch(0, st);
  for (int blk = 0; blk < nblk; ++blk) {
    const int tb = blk * kPfBlk;
    stage(st);
    __syncthreads();
    if (blk + 1 < nblk) fetch(tb + kPfBlk, st);         // in flight behind this block's MFMAs
    if (tb <= wave_last) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(&k_lds[i * kPfKStride + ks * 16 + h * 8]);
        s = kv_mfma32<BF16>(a, qf[ks], s);
      }
      // register r of lane half h is position tb + 8 (r >> 2) + 4 h + (r & 3)
      bool ok[16];
      float mb = kKvIdle;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ok[r] = tb + 8 * (r >> 2) + 4 * h + (r & 3) <= qpos;
        s[r] = ok[r] ? s[r] * p.sm_scale : kKvIdle;
        mb = fmaxf(mb, s[r]);
      }
      mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
      const float mn = fmaxf(m, mb), alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      if (__any(alpha != 1.0f)) {                        // (wave-uniform: once the maxima have settled most blocks rescale nothing)
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[dt][r] *= alpha;
      }
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        w[r] = ok[r] ? __builtin_amdgcn_exp2f(s[r] - m) : 0.f;
        l += w[r];
      }
      u32x4 pf[2];
#pragma unroll
      for (int sk = 0; sk < 2; ++sk)
#pragma unroll
        for (int j = 0; j < 4; ++j) pf[sk][j] = kv_pack2<BF16>(w[sk * 8 + 2 * j], w[sk * 8 + 2 * j + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int sk = 0; sk < 2; ++sk) {
          const u32x4 a = *reinterpret_cast<const u32x4*>(&v_lds[(dt * 32 + i) * kPfVStride + sk * 16 + h * 8]);
          acc[dt] = kv_mfma32<BF16>(a, pf[sk], acc[dt]);
        }
    }
    __syncthreads();
  }

  // ---- O^T: lane (i, h) holds d = 32 dt + 8 (r >> 2) + 4 h + (r & 3) of query row i
  l += __shfl_xor(l, 32, 64);
  if (!valid) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  uint16_t* orow_p = reinterpret_cast<uint16_t*>(p.o) + orow;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = acc[dt][gq * 4 + e] * inv;
      const u32x2 pk = {kv_from_f32<BF16>(y[0]) | (kv_from_f32<BF16>(y[1]) << 16), kv_from_f32<BF16>(y[2]) | (kv_from_f32<BF16>(y[3]) << 16)};
      *reinterpret_cast<u32x2*>(orow_p + dt * 32 + gq * 8 + h * 4) = pk;
    }
}

// ---- launcher (arguments validated by c_api_kv.hip; a.kv_param is not read)
int kv_prefill16(const KvPrefillArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_prefill_16bit";
  KvPrefill16Params p{};
  kv_prefill_fill(p, a);
  const dim3 grid = kv_prefill_grid(p, a), block(256);
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<kv_prefill16_kernel<true>>(grid, block, 0, stream, who, p);
  return launch_kernel<kv_prefill16_kernel<false>>(grid, block, 0, stream, who, p);
}

}  // namespace arcq
