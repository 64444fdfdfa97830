// MXFP6 GEMM for gfx950 on the block-scaled MFMA with e3m2 activations (v_mfma_scale_f32_{32x32x64,16x16x128}_f8f6f4, cbsz = 3).
//
//   D[m,n] = alpha * sum_{k < Kp} deq(A[m,k]) * deq(B[n,k])      A [M, 3 Kp/4] e3m2, SFA / SFB [rows, Kp/32] E8M0
//   kBFmt = ARCQ_MX_B_E3M2:  B [N, 3 Kp/4] e3m2 (blgp = 3)        kBFmt = ARCQ_MX_B_E2M1:  B [N, Kp/2] e2m1 (blgp = 4), W4A6
//
// The two operands of the instruction carry their own format selector, so the mixed form is the same kernel with B's fetch and
// fragment swapped for gemm_mx.hip's; every product of two codes and two power-of-two scales is exact in either form.
//
// Operand map.  Lanes and scale bytes are the fp4 form's (gemm_mx.hip): 16x16x128 lane l = row l & 15, K elements [32 (l >> 4), +32);
// 32x32x64 lane l = row l & 31, K elements [32 (l >> 5), +32); the lane's scale byte shifted down to byte 0, op_sel 0.  An e3m2 operand
// is SIX registers: the lane's 32 codes as stored, element i in bits [6 i, 6 i + 6) of the 192-bit string (arcq.h "MXFP6-ARC") -- a
// fragment is a copy of the block's 24 bytes, no shuffle.  Pinned with exact data by tests/test_mx6_gpu.py::test_lane_and_bit_map_exact.
//
// What is new against gemm_mx.hip is the 6-bit data path: a block is 24 bytes and only 8-byte aligned, a row's K step 96 bytes.
//
// mx6_tile_kernel, M > kMxSmallM: 128 x 128 tiles, 4 waves of 64 x 64 (2 x 2 MFMA 32x32x64), K steps of 128 double-buffered through
//   LDS: the global loads of step s + 1 are in flight while step s computes (mx_tile_kernel's loop and barriers).
//   Global -> LDS: a row's step is 96 bytes = six 16-byte chunks (rows are multiples of 96 bytes: every chunk is 16-byte aligned), an
//   operand's step 768 chunks, three per thread: thread t takes chunks t, t + 256, t + 512, chunk c = row c / 6, piece c % 6 -- six
//   adjacent lanes fetch one row's 96 adjacent bytes.  An e2m1 B keeps mx_tile_kernel's two chunks per thread and its XOR swizzle.
//   LDS rows of e3m2 are padded from 96 to kMx6Pitch = 104 bytes.  The bank argument: a fragment is read as three 8-byte words
//   (ds_read_b64; 24 b is not a multiple of 16), and an 8-byte read is served 32 lanes at a time by the 64 four-byte banks.  Lanes 0..31
//   (and 32..63) of a wave read 32 consecutive rows at ONE in-row offset, so their words sit at 8 (13 r + const): 13 is odd, r -> 13 r
//   mod 32 is a permutation, the 32 words cover the 32 bank pairs once each -- conflict-free, as is any odd number of words per row; 13 is
//   the smallest above the 12 of the data.  (At the unpadded pitch, 12 r mod 32 takes 8 values: a 4-way conflict on every fragment read.)
//   The price is the stash: rows start at odd multiples of 8 bytes, so a chunk is stored as two 8-byte words, and 32 lanes' words wrap
//   the banks unevenly (2-way on some).  A step has 6 chunk stores per thread against 24 fragment words read: the reads are the ones
//   to keep free.  LDS: 2 x (13312 + 13312 + 1024) = 55296 bytes with an e3m2 B, 2 x (13312 + 8192 + 1024) = 45056 with an e2m1 B.
//
// mx6_small_kernel, M <= kMxSmallM: mx_small_kernel's split -- one 16-column slice of B per workgroup (each weight byte is read by ONE
//   workgroup when M <= 16), 8 waves over K, 16x16x128 MFMA, partial sums added in LDS in a fixed order -- with the fragments straight
//   from global memory into the MFMA registers.  A lane's 24 bytes at row + 96 s + 24 q are 8-byte aligned; global loads need dword
//   alignment only, so they are ONE global_load_dwordx4 (bytes 0..15) and ONE global_load_dwordx2 (bytes 16..23) into the six adjacent
//   registers of the operand (the pointer types below carry the 8-byte alignment, so the compiler neither splits nor assumes more).
//   The four lanes q = 0..3 of a row fetch its 96 adjacent bytes.  K steps in flight: an e3m2 pair is 12 operand registers and 2 scale
//   registers per step against MXFP4's 8 + 2; kMx6SmallUnroll = 4 steps are 56 registers beside 4 accumulators and the addresses, well
//   inside the 128 a 512-thread workgroup may use per lane -- so the depth stays mx_small_kernel's 4, one wave holding 4 x 1.5 KB of B.
//
// Two MFMAs per e3m2 pair.  Inside one 32-block the instruction aligns the 32 products to the largest and cuts what lies more than 14 bits
// below its exponent (measured through this GEMM, DESIGN.md 3.7: beside 28 * 28 a product of 2^-6 is lost, beside 14 * 14 one of 2^-8;
// blocks of one instruction do not affect each other, the scales are applied after).  e3m2 x e2m1 products are multiples of 2^-5 up to
// 168 < 2^8 and always fit; e3m2 x e3m2 products are multiples of 2^-8 up to 784 and do not.  So against an e3m2 B the A fragment is
// split in registers (mx6_split_fragment: a bit mask from bit 4 of each code, ~50 VALU operations per fragment) into the codes of
// magnitude >= 2 -- multiples of 1/2, products multiples of 2^-5 below 2^10 -- and the others -- below 2, products multiples of 2^-8
// below 2^6 -- and each half is multiplied by its own MFMA into the same accumulator: both fit the 14 bits with nothing cut.  B, the scale
// bytes and the stored format are untouched; an e2m1 B keeps one MFMA.
//
// Summation order per output, which tests/test_mx6_gpu.py counts.  Per (lane group, K block) an e2m1 B has ONE accumulation and an e3m2
// B TWO (large codes, then small).  Tile: the accumulator takes the 32x32x64 MFMAs of each 128-step in ascending K, Kp / 64 (e3m2 B:
// Kp / 32) accumulations, then alpha.  Small: wave w accumulates the 16x16x128 MFMAs of steps s = w (mod 8) in ascending order,
// ceil(steps / 8) (e3m2 B: twice that) of them, the eight partial sums are added w = 0 .. 7 (7 additions), then alpha.
// Epilogue: gemm_mx_common.hpp mx_store, arcq_gemm_mxfp4's roundings.  Row offsets are size_t throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mx6_common.hpp"
#include "gemm_mx_tile_common.hpp"

namespace arcq {

// (the e3m2 fragment, its split and the 8-byte-aligned pointer types: gemm_mx6_common.hpp, shared with gemm_mx6_rw.hip)
constexpr int kMx6Pitch = 104;                            // LDS row of a step: 13 eight-byte words
constexpr int kMx6OpBytes = kMxTile * kMx6Pitch;
static_assert((kMx6Pitch / 8) % 2 == 1 && kMx6Pitch % 8 == 0 && kMx6OpBytes % 16 == 0, "an odd number of 8-byte words per LDS row");

// ---------------------------------------------------------------------------------------------------------------- tiled
template <int kBFmt>
__global__ __launch_bounds__(256) void mx6_tile_kernel(MxArgs p) {
  constexpr bool kB6 = kBFmt == ARCQ_MX_B_E3M2;
  constexpr int kBCbsz = kB6 ? kMx6Fmt : 4;
  constexpr int kBBytes = kB6 ? kMx6OpBytes : kMxOpBytes;
  constexpr int kBufBytes = kMx6OpBytes + kBBytes + 2 * kMxTile * 4;     // A, B, then one scale dword per row of A and of B
  constexpr int kBChunks = kB6 ? 3 : 2;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kBufBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kMxTile, n0 = blockIdx.x * kMxTile;
  const size_t rowa = (size_t)(p.Kp >> 2) * 3, rowb = kB6 ? rowa : (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  constexpr int kBStep = kB6 ? kMx6StepBytes : 64;

  // staging: e3m2 chunk c = t + 256 k is piece c % 6 of row c / 6; e2m1 chunks t and t + 256 are piece t & 3 of rows t >> 2 and + 64
  const uint8_t* gA[3];
  const uint8_t* gB[kBChunks];
  int lA[3], lB[kBChunks];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = tid + 256 * k, r = c / 6, cc = c - 6 * r;
    gA[k] = p.A + (size_t)min(m0 + r, p.M - 1) * rowa + cc * 16;
    lA[k] = r * kMx6Pitch + cc * 16;
    if constexpr (kB6) {
      gB[k] = p.B + (size_t)min(n0 + r, p.N - 1) * rowb + cc * 16;
      lB[k] = lA[k];
    }
  }
  if constexpr (!kB6) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = (tid >> 2) + 64 * k, cc = tid & 3;
      gB[k] = p.B + (size_t)min(n0 + r, p.N - 1) * rowb + cc * 16;
      lB[k] = mx_lds_off(r, cc);
    }
  }
  const uint8_t* gS = tid < kMxTile ? p.SFA + (size_t)min(m0 + tid, p.M - 1) * rows : p.SFB + (size_t)min(n0 + tid - kMxTile, p.N - 1) * rows;
  // the load of a step past the end re-reads the last step (stashed where nothing reads it): no branch around the loads
  uint4 ra[3], rb[kBChunks];
  uint32_t rs;
  auto load = [&](int s) __attribute__((always_inline)) {
    const size_t o = (size_t)min(s, steps - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) ra[k] = *reinterpret_cast<const uint4*>(gA[k] + o * kMx6StepBytes);
#pragma unroll
    for (int k = 0; k < kBChunks; ++k) rb[k] = *reinterpret_cast<const uint4*>(gB[k] + o * kBStep);
    rs = *reinterpret_cast<const uint32_t*>(gS + o * 4);
  };
  auto put6 = [&](uint8_t* at, const uint4& v) __attribute__((always_inline)) {       // at: 8-byte aligned
    reinterpret_cast<uint2*>(at)[0] = make_uint2(v.x, v.y);
    reinterpret_cast<uint2*>(at)[1] = make_uint2(v.z, v.w);
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
    uint8_t* L = lds + buf * kBufBytes;
#pragma unroll
    for (int k = 0; k < 3; ++k) put6(L + lA[k], ra[k]);
#pragma unroll
    for (int k = 0; k < kBChunks; ++k) {
      if constexpr (kB6) put6(L + kMx6OpBytes + lB[k], rb[k]);
      else *reinterpret_cast<uint4*>(L + kMx6OpBytes + lB[k]) = rb[k];
    }
    reinterpret_cast<uint32_t*>(L + kMx6OpBytes + kBBytes)[tid] = rs;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int r32 = lane & 31, h = lane >> 5;
  auto get6 = [&](const uint8_t* at) __attribute__((always_inline)) {
    const uint2* w = reinterpret_cast<const uint2*>(at);
    return frag6(w[0], w[1], w[2]);
  };
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const uint8_t* L = lds + buf * kBufBytes;
    const uint32_t* LS = reinterpret_cast<const uint32_t*>(L + kMx6OpBytes + kBBytes);
    uint32_t sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[i] = LS[wm * 64 + i * 32 + r32];
      sb[i] = LS[kMxTile + wn * 64 + i * 32 + r32];
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {            // two K-64 halves of the step: block 2 sub + h of each row
      const int blk = 2 * sub + h, sh = 8 * blk;
      i32x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = get6(L + (wm * 64 + i * 32 + r32) * kMx6Pitch + blk * 24);
        if constexpr (kB6) b[i] = get6(L + kMx6OpBytes + (wn * 64 + i * 32 + r32) * kMx6Pitch + blk * 24);
        else b[i] = frag(*reinterpret_cast<const uint4*>(L + kMx6OpBytes + mx_lds_off(wn * 64 + i * 32 + r32, blk)));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr (kB6) {             // e3m2 x e3m2: A's large codes first, then its small ones (header, "Two MFMAs per e3m2 pair")
          i32x8 ah, al;
          split6(a[i], ah, al);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ah, b[j], acc[i][j], kMx6Fmt, kBCbsz, 0, (int)(sa[i] >> sh), 0, (int)(sb[j] >> sh));
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(al, b[j], acc[i][j], kMx6Fmt, kBCbsz, 0, (int)(sa[i] >> sh), 0, (int)(sb[j] >> sh));
          }
        } else {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], kMx6Fmt, kBCbsz, 0, (int)(sa[i] >> sh), 0,
                                                                        (int)(sb[j] >> sh));
        }
      }
    }
  };

  // mx_tile_kernel's loop: the loads of step s + 1 are issued before step s computes and stored to the other buffer after it; the
  // scheduling barriers pin that order
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
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + r32;
      if (n >= p.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < p.M) mx_store(p, alpha, m, n, acc[i][j][r]);
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------- small M
constexpr int kMx6SmallUnroll = 4;

template <int kBFmt>
__global__ __launch_bounds__(64 * kMxSmallWaves) void mx6_small_kernel(MxArgs p) {
  constexpr bool kB6 = kBFmt == ARCQ_MX_B_E3M2;
  constexpr int kBCbsz = kB6 ? kMx6Fmt : 4;
  constexpr int kBStep = kB6 ? kMx6StepBytes : 64, kBFrag = kB6 ? 24 : 16;
  __shared__ float part[kMxSmallWaves][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * 16;
  const size_t rowa = (size_t)(p.Kp >> 2) * 3, rowb = kB6 ? rowa : (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;
  const int r16 = lane & 15, q = lane >> 4;
  const uint8_t* gA = p.A + (size_t)min(m0 + r16, p.M - 1) * rowa + q * 24;
  const uint8_t* gB = p.B + (size_t)(n0 + r16) * rowb + q * kBFrag;                  // N % 16 == 0: always in range
  const uint8_t* gSA = p.SFA + (size_t)min(m0 + r16, p.M - 1) * rows;
  const uint8_t* gSB = p.SFB + (size_t)(n0 + r16) * rows;
  const int sh = 8 * q;
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int s0 = wave; s0 < steps; s0 += kMxSmallWaves * kMx6SmallUnroll) {
    i32x8 a[kMx6SmallUnroll], b[kMx6SmallUnroll];
    uint32_t sa[kMx6SmallUnroll], sb[kMx6SmallUnroll];
#pragma unroll
    for (int u = 0; u < kMx6SmallUnroll; ++u) {
      const size_t s = (size_t)min(s0 + u * kMxSmallWaves, steps - 1);      // clamped loads; the MFMA of a step past the end is skipped
      const uint8_t* pb = gB + s * kBStep;
      if constexpr (kB6) b[u] = frag6(ARCQ_WLOAD(reinterpret_cast<const i32x4_a8*>(pb)), ARCQ_WLOAD(reinterpret_cast<const i32x2_a8*>(pb + 16)));
      else b[u] = frag(ARCQ_WLOAD(reinterpret_cast<const i32x4*>(pb)));
      sb[u] = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(gSB + s * 4));
      const uint8_t* pa = gA + s * kMx6StepBytes;
      a[u] = frag6(*reinterpret_cast<const i32x4_a8*>(pa), *reinterpret_cast<const i32x2_a8*>(pa + 16));
      sa[u] = *reinterpret_cast<const uint32_t*>(gSA + s * 4);
    }
#pragma unroll
    for (int u = 0; u < kMx6SmallUnroll; ++u)
      if (s0 + u * kMxSmallWaves < steps) {
        if constexpr (kB6) {
          i32x8 ah, al;
          split6(a[u], ah, al);
          acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ah, b[u], acc, kMx6Fmt, kBCbsz, 0, (int)(sa[u] >> sh), 0, (int)(sb[u] >> sh));
          acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(al, b[u], acc, kMx6Fmt, kBCbsz, 0, (int)(sa[u] >> sh), 0, (int)(sb[u] >> sh));
        } else {
          acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[u], b[u], acc, kMx6Fmt, kBCbsz, 0, (int)(sa[u] >> sh), 0, (int)(sb[u] >> sh));
        }
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][lane][r] = acc[r];
  __syncthreads();
  if (wave != 0) return;
  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  const int n = n0 + r16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = part[0][lane][r];
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) t += part[w][lane][r];
    const int m = m0 + 4 * q + r;
    if (m < p.M) mx_store(p, alpha, m, n, t);
  }
}

template <int kBFmt>
static int mx6_launch_gemm(const MxArgs& p, hipStream_t stream) {
  const char* who = "arcq_gemm_mxfp6";
  if (p.M <= kMxSmallM)
    return launch_kernel<mx6_small_kernel<kBFmt>>(dim3((unsigned)(p.N / 16), (unsigned)((p.M + 15) / 16)), dim3(64 * kMxSmallWaves), 0, stream, who, p);
  return launch_kernel<mx6_tile_kernel<kBFmt>>(dim3((unsigned)((p.N + kMxTile - 1) / kMxTile), (unsigned)((p.M + kMxTile - 1) / kMxTile)), dim3(256), 0, stream,
                                               who, p);
}

int gemm_mx6(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t Kp, int b_format,
             float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream) {
  MxArgs p;
  p.A = A; p.B = B; p.SFA = SFA; p.SFB = SFB; p.D = D;
  p.M = (int)M; p.N = (int)N; p.Kp = (int)Kp;
  p.alpha_host = alpha_host; p.alpha_dev = alpha_dev;
  p.bias = (const uint16_t*)bias; p.residual = (const uint16_t*)residual; p.out_dtype = out_dtype;
  p.QACT = nullptr; p.SFACT = nullptr; p.KE = 0;
  return b_format == ARCQ_MX_B_E3M2 ? mx6_launch_gemm<ARCQ_MX_B_E3M2>(p, stream) : mx6_launch_gemm<ARCQ_MX_B_E2M1>(p, stream);
}

}  // namespace arcq
