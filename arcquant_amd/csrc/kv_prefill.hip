// Causal prefill attention over the int4 pages of include/arcq_kv.h (arcq_kv_batch_prefill) on v_mfma_f32_32x32x16_{f16,bf16}.
//
//   grid (tiles, N * chunks), 256 threads = 4 waves.  A workgroup owns a tile of 128 query-row slots of one (sequence, kv head): slot r
//   is (token r / hc of the tile, head ch * hc + r % hc of the kv head's group), hc = min(g, 128) heads per chunk and tpt = 128 / hc tokens
//   per tile, so the g heads of a group share every K / V block.  Tiles are found on the device: workgroup x walks qo_indptr, sequence b
//   owning ceil(n_b / tpt) of them, and leaves when it runs out of sequences (the launch has ceil(ntok / tpt) + B: at most one partial
//   tile per sequence).  A wave owns 32 slots.
//
//   Per block of 32 kv positions (blocks wholly above the tile's last query position are never visited; a wave skips the MFMAs of
//   blocks above its own):
//     staging   waves 0-1 take K, waves 2-3 V: 16 bytes (K) or two rows' 8 bytes (V) of codes per thread and the rows' (scale, zero)
//               pairs, loaded one block ahead into registers.  The nibbles become 16-bit codes 0..15 (exact in fp16 and bf16) in LDS:
//               K as [position][d], V transposed as [d][position'] with position' = position with bits 2 and 3 swapped, which is the k
//               order in which the score tile below presents its rows.  Rows past T are never loaded (the load clamps to T - 1).
//     scores    S^T = C Q^T: K codes are the A operand, the wave's 32 query rows (registers, loaded once) the B operand, so lane
//               (i, h) holds query column i and positions 8 (r >> 2) + 4 h + (r & 3) in accumulator registers r = 0..15.  Exact
//               products, fp32 accumulation;  score = sm_scale (s_t R - z_t sum_d q_d)  in fp32 VALU, as in the decode kernel, with
//               sm_scale = 128^-1/2 log2(e) folded into (s_t, z_t) when they are staged: the softmax runs in base 2.
//     softmax   online, per lane + one exchange with lane i + 32; the causal mask is a select on the score and on the weight.
//     values    O^T += V^T P^T: registers 8 s .. 8 s + 7 of the weight tile p_t s_t, rounded once to the 16-bit type, are the B
//               fragment of k-step s with no lane movement; V^T comes from LDS.  sum_t p_t z_t and the row sum are fp32 VALU sums
//               (the row sum over the unrounded weights).
//   O^T leaves lane (i, h) holding four consecutive d per register group: 8-byte stores of (O - zsum) / l.
//
// There is no split over the kv range: few query tokens over a long cache run on B * N workgroups (arcq_kv.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/arcq_kv.h"
#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kPfRows = 128;       // query-row slots of a tile
constexpr int kPfBlk = 32;         // kv positions per block
constexpr int kPfKStride = 136;    // 16-bit elements of a K row in LDS: 272 bytes, consecutive rows four banks apart
constexpr int kPfVStride = 40;     // of a V^T row: 80 bytes

struct KvPrefillParams {
  void* o;
  const void* q;
  const int32_t* qo_indptr;
  const uint8_t* data;
  const uint32_t* param;
  KvTables t;
  int B, Nq, L, layer, N, P, g, hc, tpt, chunks;
  float sm_scale;
};

typedef __bf16 pf_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t pf_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pf_u32x2 __attribute__((ext_vector_type(2)));

template <bool BF16>
__device__ __forceinline__ f32x16 pf_mfma(pf_u32x4 a, pf_u32x4 b, f32x16 c) {
  if constexpr (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pf_bf16x8, a), __builtin_bit_cast(pf_bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// two codes 0..15 as packed 16-bit values, a in the low half (exact: fp16 through 1024 + c, bf16 as the top half of the fp32)
template <bool BF16>
__device__ __forceinline__ uint32_t pf_code_pair(uint32_t a, uint32_t b) {
  if constexpr (BF16) {
    return (__float_as_uint((float)a) >> 16) | (__float_as_uint((float)b) & 0xffff0000u);
  } else {
    const f16x2 v = __builtin_bit_cast(f16x2, 0x64006400u | a | (b << 16));
    const f16x2 k = {(_Float16)1024.0f, (_Float16)1024.0f};
    return __builtin_bit_cast(uint32_t, v - k);
  }
}

// two fp32 weights rounded to the 16-bit type (nearest even), a in the low half
template <bool BF16>
__device__ __forceinline__ uint32_t pf_pack(float a, float b) {
  if constexpr (BF16) {
    return pack_bf16x2_hw(a, b);
  } else {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
  }
}

// what a staging thread holds of the next block: K 16 bytes of one row, V 8 bytes of each of two adjacent rows; their parameter pairs
struct PfStage {
  pf_u32x4 raw;
  uint32_t p0, p1;
};

template <bool BF16>
__global__ __launch_bounds__(256, 2) void kv_prefill_kernel(KvPrefillParams p) {
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[kPfBlk * kPfKStride];
  __shared__ __attribute__((aligned(16))) uint16_t v_lds[kKvD * kPfVStride];
  __shared__ __attribute__((aligned(16))) float prm[4][kPfBlk];       // K scale, K zero, V scale, V zero of the block's positions

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

  pf_u32x4 qf[8];
  float qsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    qf[ks] = pf_u32x4{0u, 0u, 0u, 0u};
    if (valid) qf[ks] = *reinterpret_cast<const pf_u32x4*>(reinterpret_cast<const uint16_t*>(p.q) + orow + ks * 16 + h * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) qsum += kv_to_f32<BF16>(qf[ks][j] & 0xffffu) + kv_to_f32<BF16>(qf[ks][j] >> 16);
  }
  qsum += __shfl_xor(qsum, 32, 64);
  const float nqsum = -qsum;

  // ---- staging roles: threads 0..127 K (row idx & 31, 32 codes idx >> 5), 128..255 V (rows tv, tv + 1 whose LDS columns are 2 tp, 2 tp + 1;
  //      16 codes idx >> 4)
  const bool is_v = wave >= 2;
  const int idx = tid & 127;
  const int kt = idx & 31, kc = idx >> 5;
  const int tp = idx & 15, vc = idx >> 4;
  const int tv = ((2 * tp) & 19) | (((2 * tp) & 4) << 1) | (((2 * tp) & 8) >> 1);      // bits 2 and 3 swapped
  const size_t vrows = (size_t)p.N * p.P;
  auto fetch = [&](int tb, PfStage& s) __attribute__((always_inline)) {
    if (!is_v) {
      const size_t row = kv_row(p.t, b, n, min(tb + kt, T - 1), p.L, p.layer, p.N, p.P);
      s.raw = *reinterpret_cast<const pf_u32x4*>(p.data + row * 64 + kc * 16);
      s.p0 = kc == 0 ? p.param[row] : 0u;
      s.p1 = 0u;
    } else {
      const size_t r0 = kv_row(p.t, b, n, min(tb + tv, T - 1), p.L, p.layer, p.N, p.P) + vrows;
      const size_t r1 = kv_row(p.t, b, n, min(tb + tv + 1, T - 1), p.L, p.layer, p.N, p.P) + vrows;
      const pf_u32x2 a = *reinterpret_cast<const pf_u32x2*>(p.data + r0 * 64 + vc * 8);
      const pf_u32x2 c = *reinterpret_cast<const pf_u32x2*>(p.data + r1 * 64 + vc * 8);
      s.raw = pf_u32x4{a[0], a[1], c[0], c[1]};
      s.p0 = vc == 0 ? p.param[r0] : 0u;
      s.p1 = vc == 0 ? p.param[r1] : 0u;
    }
  };
  auto stage = [&](const PfStage& s) __attribute__((always_inline)) {
    if (!is_v) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        pf_u32x4 c;
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = pf_code_pair<BF16>((s.raw[w] >> (8 * j)) & 15u, (s.raw[w] >> (8 * j + 4)) & 15u);
        *reinterpret_cast<pf_u32x4*>(&k_lds[kt * kPfKStride + kc * 32 + w * 8]) = c;
      }
      if (kc == 0) {
        prm[0][kt] = kv_to_f32<false>(s.p0 & 0xffffu) * p.sm_scale;
        prm[1][kt] = kv_to_f32<false>(s.p0 >> 16) * p.sm_scale;
      }
    } else {
#pragma unroll
      for (int w = 0; w < 2; ++w) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t c = pf_code_pair<BF16>((s.raw[w] >> (4 * e)) & 15u, (s.raw[2 + w] >> (4 * e)) & 15u);
          *reinterpret_cast<uint32_t*>(&v_lds[(vc * 16 + w * 8 + e) * kPfVStride + 2 * tp]) = c;
        }
      }
      if (vc == 0) {
        prm[2][tv] = kv_to_f32<false>(s.p0 & 0xffffu);
        prm[3][tv] = kv_to_f32<false>(s.p0 >> 16);
        prm[2][tv + 1] = kv_to_f32<false>(s.p1 & 0xffffu);
        prm[3][tv + 1] = kv_to_f32<false>(s.p1 >> 16);
      }
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m = kKvIdle, l = 0.f, zacc = 0.f;

  PfStage st;
  fetch(0, st);
  for (int blk = 0; blk < nblk; ++blk) {
    const int tb = blk * kPfBlk;
    stage(st);
    __syncthreads();
    if (blk + 1 < nblk) fetch(tb + kPfBlk, st);          // in flight behind this block's MFMAs
    if (tb <= wave_last) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const pf_u32x4 a = *reinterpret_cast<const pf_u32x4*>(&k_lds[i * kPfKStride + ks * 16 + h * 8]);
        s = pf_mfma<BF16>(a, qf[ks], s);
      }
      // register r of lane half h is position tb + 8 (r >> 2) + 4 h + (r & 3)
      float vs[16], vz[16];
      bool ok[16];
      float mb = kKvIdle;
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 ksc = *reinterpret_cast<const f32x4*>(&prm[0][gq * 8 + h * 4]), kzr = *reinterpret_cast<const f32x4*>(&prm[1][gq * 8 + h * 4]);
        const f32x4 vsc = *reinterpret_cast<const f32x4*>(&prm[2][gq * 8 + h * 4]), vzr = *reinterpret_cast<const f32x4*>(&prm[3][gq * 8 + h * 4]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = gq * 4 + e;
          ok[r] = tb + gq * 8 + h * 4 + e <= qpos;
          const float sc = fmaf(kzr[e], nqsum, ksc[e] * s[r]);
          s[r] = ok[r] ? sc : kKvIdle;
          mb = fmaxf(mb, s[r]);
          vs[r] = vsc[e];
          vz[r] = vzr[e];
        }
      }
      mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
      const float mn = fmaxf(m, mb), alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      if (__any(alpha != 1.0f)) {                        // (wave-uniform: once the maxima have settled most blocks rescale nothing)
        l *= alpha;
        zacc *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[dt][r] *= alpha;
      }
      float w[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pt = ok[r] ? __builtin_amdgcn_exp2f(s[r] - m) : 0.f;
        l += pt;
        zacc = fmaf(pt, vz[r], zacc);
        w[r] = pt * vs[r];
      }
      pf_u32x4 pf[2];
#pragma unroll
      for (int sk = 0; sk < 2; ++sk)
#pragma unroll
        for (int j = 0; j < 4; ++j) pf[sk][j] = pf_pack<BF16>(w[sk * 8 + 2 * j], w[sk * 8 + 2 * j + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int sk = 0; sk < 2; ++sk) {
          const pf_u32x4 a = *reinterpret_cast<const pf_u32x4*>(&v_lds[(dt * 32 + i) * kPfVStride + sk * 16 + h * 8]);
          acc[dt] = pf_mfma<BF16>(a, pf[sk], acc[dt]);
        }
    }
    __syncthreads();
  }

  // ---- O^T: lane (i, h) holds d = 32 dt + 8 (r >> 2) + 4 h + (r & 3) of query row i
  l += __shfl_xor(l, 32, 64);
  zacc += __shfl_xor(zacc, 32, 64);
  if (!valid) return;
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  uint16_t* orow_p = reinterpret_cast<uint16_t*>(p.o) + orow;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      float y[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = (acc[dt][gq * 4 + e] - zacc) * inv;
      const pf_u32x2 pk = {kv_from_f32<BF16>(y[0]) | (kv_from_f32<BF16>(y[1]) << 16), kv_from_f32<BF16>(y[2]) | (kv_from_f32<BF16>(y[3]) << 16)};
      *reinterpret_cast<pf_u32x2*>(orow_p + dt * 32 + gq * 8 + h * 4) = pk;
    }
}

// ---- launcher (arguments validated by c_api_kv.hip)
int kv_prefill(const KvPrefillArgs& a, hipStream_t stream) {
  const char* who = "arcq_kv_batch_prefill";
  KvPrefillParams p{};
  p.o = a.o; p.q = a.q; p.qo_indptr = a.qo_indptr; p.data = (const uint8_t*)a.kv_data; p.param = (const uint32_t*)a.kv_param;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.B = (int)a.B; p.Nq = (int)a.Nq; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.g = (int)(a.Nq / a.N);
  p.hc = p.g < kPfRows ? p.g : kPfRows;
  p.tpt = kPfRows / p.hc;
  p.chunks = (p.g + p.hc - 1) / p.hc;
  p.sm_scale = 0.12751743074602467f;                    // 128^-0.5 * log2(e): the softmax runs in base 2 (v_exp_f32)
  const int64_t tiles = (a.ntok + p.tpt - 1) / p.tpt + a.B;
  const dim3 grid((unsigned)tiles, (unsigned)(a.N * p.chunks)), block(256);
  if (a.dtype == ARCQ_KV_BF16) return launch_kernel<kv_prefill_kernel<true>>(grid, block, 0, stream, who, p);
  return launch_kernel<kv_prefill_kernel<false>>(grid, block, 0, stream, who, p);
}

}  // namespace arcq
