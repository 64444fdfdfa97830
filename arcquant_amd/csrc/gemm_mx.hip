// MXFP4 GEMM for gfx950 on the block-scaled fp4 MFMA (v_mfma_scale_f32_{32x32x64,16x16x128}_f8f6f4, cbsz = blgp = 4).
//
//   D[m,n] = alpha * sum_{k < Kp} deq(A[m,k]) * deq(B[n,k])      A [M, Kp/2], B [N, Kp/2] e2m1, SFA / SFB [rows, Kp/32] E8M0
//
// Every product of two e2m1 codes and two power-of-two scales is exact, so the instruction takes the packed codes and the
// scale bytes as they are stored: no dequantisation instruction, the matrix pipe at the fp4 rate.
//
// Operand map of the fp4 form (pinned by tests/test_mx_gpu.py::test_lane_map_exact with exact integer data):
//   16x16x128: lane l supplies row l & 15, K elements [32 (l >> 4), +32) = 16 bytes, and the scale byte of that 32-block;
//   32x32x64:  lane l supplies row l & 31, K elements [32 (l >> 5), +32) and the scale byte of that block.
//   The scale operand is a VGPR; op_sel picks one of its bytes for the whole wave, so each lane shifts its byte down and
//   op_sel stays 0.  C/D as every gfx950 MFMA: 32x32 reg r of lane l = D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31],
//   16x16 reg r of lane l = D[4 (l >> 4) + r][l & 15]  (row = A's row, column = B's row).
//
// Two configurations:
//   mx_tile_kernel   M > kMxSmallM: 128 x 128 tiles, 4 waves of 64 x 64 (2 x 2 MFMA 32x32x64), K steps of 128 staged through
//                    LDS (XOR-swizzled 64-byte rows: the 16-byte fragment reads are bank-conflict free), double-buffered: the
//                    global loads of step s + 1 are in flight while step s computes.
//   mx_small_kernel  M <= kMxSmallM: one 16-column slice of B per workgroup (each weight byte is read by ONE workgroup
//                    when M <= 16), 8 waves splitting K, four K steps of loads in flight per wave, 16x16x128 MFMA, partial
//                    sums added in LDS in a fixed order.
//
// Both kernels take the epilogue as a template parameter.  kEpiSiluMul (arcq_gemm_mxfp4_silu_mul): B's rows interleave gate and up
// (g0, u0, g1, u1, ...), D = bf16 [M, N/2] receives silu(y_gate) * y_up with torch's roundings, y being the bf16 value the plain epilogue
// would store (never written).  A lane holds ONE output column, so gate and up of a pair sit in neighbouring lanes of a DPP quad (N % 16
// == 0: a quad of lanes is inside or outside n < N as a whole); see mx_silu_pair.
//
// kEpiSiluMulQuant (arcq_gemm_mxfp4_silu_mul_quantize): the same activations are not stored but quantised where they are, to the
// MXFP4-ARC operand of the next GEMM (QACT, SFACT = arcq_mx_quantize_x of ACT with the identity reorder_index).  A block's E8M0 scale
// needs the 32 values of the block and nothing else, and 32 adjacent activations are 64 adjacent y-columns: a 128-column tile holds two
// whole blocks per row (N % 128 == 0: no ragged column tile).  The activations of a tile go through the LDS the K loop has finished
// with, one thread then quantises one (row, block) with the quantisers' own mx_store_x_block -- residual blocks of the outlier tail
// and the row's padding blocks included.  M <= kMxSmallM: mx_slice_quant_kernel, mx_small_kernel's K split and sum order over a
// 64-column slice (one block per row) instead of a 16-column one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx_common.hpp"
#include "quantize_mx_device.hpp"

namespace arcq {

// One (row, block) of the quantised activation: the block's 32 bf16 activations at `src` (LDS, 16-byte aligned) -> codes and scale byte at
// block b of row m, the residual block when b is in the outlier tail, and, from the owner of the row's last block, the padding blocks.
__device__ __forceinline__ void mx_quantize_act_block(const MxArgs& p, const uint8_t* src, int m, int b) {
  const int KQ2 = p.N >> 1, K2 = KQ2 + p.KE, Kp2 = (K2 + 127) & ~127;
  const int B = KQ2 >> 5, P = (KQ2 - p.KE) >> 5, Bp = Kp2 >> 5;
  float v[32];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint4 u = *reinterpret_cast<const uint4*>(src + c * 16);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      v[8 * c + 2 * d] = bf16_bits_to_f32(w[d] & 0xffffu);
      v[8 * c + 2 * d + 1] = bf16_bits_to_f32(w[d] >> 16);
    }
  }
  uint8_t* qrow = p.QACT + (size_t)m * (size_t)(Kp2 >> 1);
  uint8_t* srow = p.SFACT + (size_t)m * (size_t)Bp;
  mx_store_x_block(qrow, srow, b, B + (b - P), b >= P, v);
  if (b == B - 1)
    for (int pb = K2 >> 5; pb < Bp; ++pb) {         // [K2, Kp2): code 0, scale 2^0 (K2 % 64 == 0: none or two blocks)
      *reinterpret_cast<uint4*>(qrow + (size_t)pb * 16) = make_uint4(0, 0, 0, 0);
      srow[pb] = 127;
    }
}

// ---------------------------------------------------------------------------------------------------------------- tiled
constexpr int kMxTile = 128;
constexpr int kMxOpBytes = kMxTile * 64;                     // one operand tile of one K step: 128 rows x 64 bytes
constexpr int kMxBufBytes = 2 * kMxOpBytes + 2 * kMxTile * 4;   // A, B, then one scale dword per row of A and of B
// kEpiSiluMulQuant: the tile's 128 x 64 bf16 activations in the staging buffers, rows of 128 bytes padded to 144 (unpadded, the 16
// lanes of a ds_read_b128 group -- 8 rows x 2 blocks -- would all start on banks 0 and 16; 36 r + 16 b mod 64 spreads them to 2-way at
// worst, on four reads per thread)
constexpr int kMxActRowBytes = 64 * 2 + 16;
static_assert(kMxTile * kMxActRowBytes <= 2 * kMxBufBytes, "the activation image reuses the staging buffers");

// LDS byte offset of 16-byte chunk c (0..3) of staged row r.  The chunk index is XORed with (r >> 2) & 3: the 16 lanes of each
// ds_read_b128 lane group read 16 different rows at one logical chunk; rows equal mod 4 would share banks in a plain 64-byte
// layout, the swizzle gives them four different chunks (conflict-free, and no padding: 4 workgroups fit a CU's LDS).
__device__ __forceinline__ int mx_lds_off(int r, int c) { return r * 64 + ((c ^ (r >> 2)) & 3) * 16; }

template <int kEpi>
__global__ __launch_bounds__(256) void mx_tile_kernel(MxArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kMxBufBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kMxTile, n0 = blockIdx.x * kMxTile;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;

  // staging: thread t moves 16-byte chunks t and t + 256 of each operand tile (row = chunk / 4) and one scale dword
  const int cr = tid >> 2, cc = tid & 3;
  const uint8_t* gA0 = p.A + (size_t)min(m0 + cr, p.M - 1) * rowb + cc * 16;
  const uint8_t* gA1 = p.A + (size_t)min(m0 + cr + 64, p.M - 1) * rowb + cc * 16;
  const uint8_t* gB0 = p.B + (size_t)min(n0 + cr, p.N - 1) * rowb + cc * 16;
  const uint8_t* gB1 = p.B + (size_t)min(n0 + cr + 64, p.N - 1) * rowb + cc * 16;
  const uint8_t* gS = tid < kMxTile ? p.SFA + (size_t)min(m0 + tid, p.M - 1) * rows
                                    : p.SFB + (size_t)min(n0 + tid - kMxTile, p.N - 1) * rows;
  const int l0 = mx_lds_off(cr, cc), l1 = mx_lds_off(cr + 64, cc);
  // the load of a step past the end re-reads the last step (stashed where nothing reads it): no branch around the loads
  uint4 ra0, ra1, rb0, rb1;
  uint32_t rs;
  auto load = [&](int s) __attribute__((always_inline)) {
    const size_t o = (size_t)min(s, steps - 1) * 64;
    ra0 = *reinterpret_cast<const uint4*>(gA0 + o);
    ra1 = *reinterpret_cast<const uint4*>(gA1 + o);
    rb0 = *reinterpret_cast<const uint4*>(gB0 + o);
    rb1 = *reinterpret_cast<const uint4*>(gB1 + o);
    rs = *reinterpret_cast<const uint32_t*>(gS + o / 16);
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
    uint8_t* L = lds + buf * kMxBufBytes;
    *reinterpret_cast<uint4*>(L + l0) = ra0;
    *reinterpret_cast<uint4*>(L + l1) = ra1;
    *reinterpret_cast<uint4*>(L + kMxOpBytes + l0) = rb0;
    *reinterpret_cast<uint4*>(L + kMxOpBytes + l1) = rb1;
    reinterpret_cast<uint32_t*>(L + 2 * kMxOpBytes)[tid] = rs;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int r32 = lane & 31, h = lane >> 5;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const uint8_t* L = lds + buf * kMxBufBytes;
    const uint32_t* LS = reinterpret_cast<const uint32_t*>(L + 2 * kMxOpBytes);
    uint32_t sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[i] = LS[wm * 64 + i * 32 + r32];
      sb[i] = LS[kMxTile + wn * 64 + i * 32 + r32];
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {            // two K-64 halves of the step: logical chunk 2 sub + h of each row
      const int sh = 8 * (2 * sub + h);
      i32x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = frag(*reinterpret_cast<const uint4*>(L + mx_lds_off(wm * 64 + i * 32 + r32, 2 * sub + h)));
        b[i] = frag(*reinterpret_cast<const uint4*>(L + kMxOpBytes + mx_lds_off(wn * 64 + i * 32 + r32, 2 * sub + h)));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], 4, 4, 0, (int)(sa[i] >> sh), 0,
                                                                      (int)(sb[j] >> sh));
    }
  };

  // the loads of step s + 1 are issued before step s computes and stored to the other LDS buffer after it.  The scheduling
  // barriers pin that order: left to itself the compiler hoists the LDS stores above the MFMAs (or sinks the loads below
  // them), and every step then waits out the full global latency.
  load(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    load(s + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(s & 1);
    __builtin_amdgcn_sched_barrier(0);
    stash((s + 1) & 1);
    __syncthreads();
  }

  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  if constexpr (kEpi == kEpiSiluMulQuant) {
    // every wave is past its last read of the staging buffers (the barrier that ends the K loop); N % 128 == 0: no column is outside
    const bool odd = lane & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nl = wn * 64 + j * 32 + r32;                 // y-column within the tile
        const float bias = p.bias ? bf16_bits_to_f32(p.bias[n0 + nl]) : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, acc[i][j][r], p.bias, bias), mx_y_bits(alpha, acc[i][j][r + 1], p.bias, bias), odd);
          const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h + (odd ? 1 : 0);
          if (!(lane & 2)) *reinterpret_cast<uint32_t*>(lds + ml * kMxActRowBytes + (nl >> 1) * 2) = pk;   // rows >= M hold clamped rows' values
        }
      }
    __syncthreads();
    const int ml = tid >> 1, bl = tid & 1;                     // thread -> (row, block): a lane pair stores 32 adjacent code bytes
    if (m0 + ml < p.M) mx_quantize_act_block(p, lds + ml * kMxActRowBytes + bl * 64, m0 + ml, (n0 >> 6) + bl);
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + r32;
      if (n >= p.N) continue;
      if constexpr (kEpi == kEpiSiluMul) {
        const bool odd = lane & 1;
        const float bias = p.bias ? bf16_bits_to_f32(p.bias[n]) : 0.0f;
        uint16_t* act = reinterpret_cast<uint16_t*>(p.D) + (n >> 1);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {                    // rows r and r + 1 of the register tile are adjacent rows of D
          const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, acc[i][j][r], p.bias, bias), mx_y_bits(alpha, acc[i][j][r + 1], p.bias, bias), odd);
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h + (odd ? 1 : 0);
          if (!(lane & 2) && m < p.M) *reinterpret_cast<uint32_t*>(act + (size_t)m * (size_t)(p.N >> 1)) = pk;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (m < p.M) mx_store(p, alpha, m, n, acc[i][j][r]);
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------- small M
constexpr int kMxSmallUnroll = 4;

template <int kEpi>
__global__ __launch_bounds__(64 * kMxSmallWaves) void mx_small_kernel(MxArgs p) {
  __shared__ float part[kMxSmallWaves][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  const int r16 = lane & 15, q = lane >> 4;
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowb + q * 16;
  const uint8_t* gB = p.B + (size_t)(n0 + r16) * rowb + q * 16;                     // N % 16 == 0: always in range
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const uint8_t* gSB = p.SFB + (size_t)(n0 + r16) * rows;
  const int sh = 8 * q;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave; s0 < steps; s0 += kMxSmallWaves * kMxSmallUnroll) {
    i32x4 a[kMxSmallUnroll], b[kMxSmallUnroll];
    uint32_t sa[kMxSmallUnroll], sb[kMxSmallUnroll];
#pragma unroll
    for (int u = 0; u < kMxSmallUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMA of a step past the end is skipped
      b[u] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gB + (size_t)s * 64));
      sb[u] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSB + (size_t)s * 4));
      a[u] = *reinterpret_cast<const i32x4*>(gA + (size_t)s * 64);
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + (size_t)s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMxSmallUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps)
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u]), frag(b[u]), acc, 4, 4, 0, (int)(sa[u] >> sh), 0,
                                                               (int)(sb[u] >> sh));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][lane][r] = acc[r];
  __syncthreads();
  if (wave != 0) return;
  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  const int n = n0 + r16;
  float t[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    t[r] = part[0][lane][r];
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) t[r] += part[w][lane][r];
  }
  if constexpr (kEpi == kEpiSiluMul) {
    const bool odd = lane & 1;
    const float bias = p.bias ? bf16_bits_to_f32(p.bias[n]) : 0.0f;
    uint16_t* act = reinterpret_cast<uint16_t*>(p.D) + (n >> 1);
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, t[r], p.bias, bias), mx_y_bits(alpha, t[r + 1], p.bias, bias), odd);
      const int m = m0 + 4 * q + r + (odd ? 1 : 0);
      if (!(lane & 2) && m < p.M) *reinterpret_cast<uint32_t*>(act + (size_t)m * (size_t)(p.N >> 1)) = pk;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 4 * q + r;
      if (m < p.M) mx_store(p, alpha, m, n, t[r]);
    }
  }
}

// kEpiSiluMulQuant for M <= kMxSmallM.  mx_small_kernel's 16 y-columns are 8 activations, a quarter of a block; this kernel gives a
// workgroup 64 y-columns = one block per row: one A fragment against four B fragments per K step.  Every (m, n) sum is mx_small_kernel's:
// wave w takes the steps s = w (mod 8) in ascending order, the eight partial sums are added w = 0 .. 7.  Waves 0 .. 3 each finish one
// 16-column fragment and put its activations into LDS (rows of 64 bytes padded to 80: 20 r mod 64 is a different multiple of 4 for each
// of the 16 rows); 16 threads then quantise one row's block each.
constexpr int kMxSliceCols = 64;
constexpr int kMxSliceFrags = kMxSliceCols / 16;
constexpr int kMxSliceUnroll = 2;
constexpr int kMxSliceActRowBytes = 32 * 2 + 16;

__global__ __launch_bounds__(64 * kMxSmallWaves) void mx_slice_quant_kernel(MxArgs p) {
  __shared__ __attribute__((aligned(16))) float part[kMxSmallWaves][kMxSliceFrags][64][4];
  __shared__ __attribute__((aligned(16))) uint8_t act[16 * kMxSliceActRowBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kMxSliceCols, m0 = blockIdx.y * 16;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  const int r16 = lane & 15, q = lane >> 4;
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowb + q * 16;
  const uint8_t* gB = p.B + (size_t)(n0 + r16) * rowb + q * 16;                     // N % 128 == 0: always in range
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const uint8_t* gSB = p.SFB + (size_t)(n0 + r16) * rows;
  const int sh = 8 * q;
  f32x4 acc[kMxSliceFrags];
#pragma unroll
  for (int j = 0; j < kMxSliceFrags; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave; s0 < steps; s0 += kMxSmallWaves * kMxSliceUnroll) {
    i32x4 a[kMxSliceUnroll], b[kMxSliceUnroll][kMxSliceFrags];
    uint32_t sa[kMxSliceUnroll], sb[kMxSliceUnroll][kMxSliceFrags];
#pragma unroll
    for (int u = 0; u < kMxSliceUnroll; ++u) {
      const int s = min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMAs of a step past the end are skipped
#pragma unroll
      for (int j = 0; j < kMxSliceFrags; ++j) {
        b[u][j] = ARCQ_WLOAD(reinterpret_cast<const i32x4*>(gB + (size_t)j * 16 * rowb + (size_t)s * 64));
        sb[u][j] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSB + (size_t)j * 16 * rows + (size_t)s * 4));
      }
      a[u] = *reinterpret_cast<const i32x4*>(gA + (size_t)s * 64);
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + (size_t)s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMxSliceUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps) {
#pragma unroll
        for (int j = 0; j < kMxSliceFrags; ++j)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag(a[u]), frag(b[u][j]), acc[j], 4, 4, 0, (int)(sa[u] >> sh), 0,
                                                                    (int)(sb[u][j] >> sh));
      }
  }
#pragma unroll
  for (int j = 0; j < kMxSliceFrags; ++j) *reinterpret_cast<f32x4*>(part[wave][j][lane]) = acc[j];
  __syncthreads();
  if (wave < kMxSliceFrags) {                                  // wave j: fragment j, y-columns [16 j, 16 j + 16) of the slice
    const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
    f32x4 t = *reinterpret_cast<const f32x4*>(part[0][wave][lane]);
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(part[w][wave][lane]);
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] += o[r];
    }
    const bool odd = lane & 1;
    const int nl = wave * 16 + r16;
    const float bias = p.bias ? bf16_bits_to_f32(p.bias[n0 + nl]) : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, t[r], p.bias, bias), mx_y_bits(alpha, t[r + 1], p.bias, bias), odd);
      const int ml = 4 * q + r + (odd ? 1 : 0);
      if (!(lane & 2)) *reinterpret_cast<uint32_t*>(act + ml * kMxSliceActRowBytes + (nl >> 1) * 2) = pk;
    }
  }
  __syncthreads();
  if (tid < 16 && m0 + tid < p.M) mx_quantize_act_block(p, act + tid * kMxSliceActRowBytes, m0 + tid, (int)blockIdx.x);
}

template <int kEpi>
static int mx_launch_gemm(const MxArgs& p, const char* who, hipStream_t stream) {
  if (p.M <= kMxSmallM) {
    const dim3 block(64 * kMxSmallWaves);
    const unsigned rows16 = (unsigned)((p.M + 15) / 16);
    if constexpr (kEpi == kEpiSiluMulQuant) return launch_kernel<mx_slice_quant_kernel>(dim3((unsigned)(p.N / kMxSliceCols), rows16), block, 0, stream, who, p);
    else return launch_kernel<mx_small_kernel<kEpi>>(dim3((unsigned)(p.N / 16), rows16), block, 0, stream, who, p);
  }
  return launch_kernel<mx_tile_kernel<kEpi>>(dim3((unsigned)((p.N + kMxTile - 1) / kMxTile), (unsigned)((p.M + kMxTile - 1) / kMxTile)), dim3(256), 0, stream, who, p);
}

int gemm_mx(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t Kp,
            float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return mx_launch_gemm<kEpiPlain>(p, "arcq_gemm_mxfp4", stream);
}

// ACT = bf16 [M, N/2]; the same contraction, kernel choice and accumulation order as gemm_mx
int gemm_mx_silu_mul(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* ACT, int64_t M, int64_t N, int64_t Kp,
                     float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = ACT;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = nullptr; p.out_dtype = ARCQ_OUT_BF16;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return mx_launch_gemm<kEpiSiluMul>(p, "arcq_gemm_mxfp4_silu_mul", stream);
}

// (QACT, SFACT) = mx_quantize_x(ACT of gemm_mx_silu_mul, identity, KQ2 = N/2, KE); ACT is never written.  N % 128 == 0.
int gemm_mx_silu_mul_quantize(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, uint8_t* QACT, uint8_t* SFACT, int64_t M,
                              int64_t N, int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = nullptr;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = nullptr; p.out_dtype = ARCQ_OUT_BF16;
  p.QACT = QACT; p.SFACT = SFACT; p.KE = (int)KE;
  return mx_launch_gemm<kEpiSiluMulQuant>(p, "arcq_gemm_mxfp4_silu_mul_quantize", stream);
}

}  // namespace arcq
