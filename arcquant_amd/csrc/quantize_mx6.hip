// Reorder + MXFP6 quantise kernels for gfx950 (activation with ARC residual / weight with duplicate).
//
// Format (include/arcq.h "MXFP6-ARC"): MXFP4-ARC's augmented K and E8M0 scale bytes with e3m2 elements.  A 32-element
// block is 24 bytes at 24 b of its row: element i in bits [6 i, 6 i + 6) of the 192-bit little-endian string, the six-VGPR operand of the
// scaled MFMA as it stands.  A row is 3 Kp / 4 bytes, a multiple of 96: rows are 16-byte aligned, blocks only 8-byte aligned.
//
// Work decomposition: quantize_mx.hip's -- one workgroup per row (grid-strided), the row staged in LDS with the padded layout of
// quantize_device.hpp, decode-sized inputs split along the row over blockIdx.y (quant_grid).  The workgroup walks its block range in
// passes of 256 adjacent blocks; in a pass thread t owns block bb + t: gather 32 values, exponent from the bits, 32 codes shifted into
// six dwords (quantize_mx6_device.hpp), one scale byte.
//
// Packing and stores.  A thread's 24 bytes start at 24 (bb + t), so a store straight from the registers would put 8 bytes into every
// 24 with each instruction: three instructions that each touch every line of the span and fill none.  Instead the thread writes its six
// dwords as three 8-byte words into a 6 KB LDS image of the pass (word 3 t + j), and after a barrier the workgroup copies the image out
// with thread t storing the 8-byte words t, t + 256, t + 512 of the span: the 64 lanes of a wave write 512 adjacent bytes with one
// instruction -- four whole 128-byte lines when the span starts on a line, whole lines but the two at the ends otherwise -- and the
// pass's 6144 bytes leave as 48 full lines.  8-byte words, not 16: the span starts at 24 bb, and blockIdx.y's ranges may start at an odd
// block.  The residual (x) or duplicate (w) blocks of the outlier tail are adjacent too -- block B + (b - P) for b >= P -- and go out the
// same way: the duplicate is a second copy of the same image from word 3 (max(bb, P) - bb) on, the residual blocks are quantised into
// the image after the primary copy has left it.  Every barrier is reached by the whole workgroup: the pass loop and the tail test depend
// on bb alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "quantize_device.hpp"
#include "quantize_mx6_device.hpp"

namespace arcq {

constexpr int kMx6Threads = 256;

// words [0, n) of the LDS image -> dst (8-byte aligned), thread t the words t, t + 256, ...
__device__ __forceinline__ void mx6_copy_out(uint8_t* dst, const uint2* image, int n, int tid) {
  for (int c = tid; c < n; c += kMx6Threads) *reinterpret_cast<uint2*>(dst + (size_t)c * 8) = image[c];
}
__device__ __forceinline__ void mx6_put_block(uint2* image, int slot, const Mx6Block& q) {
#pragma unroll
  for (int j = 0; j < 3; ++j) image[3 * slot + j] = make_uint2(q.w[2 * j], q.w[2 * j + 1]);
}

template <bool kModeW>
__global__ __launch_bounds__(kMx6Threads) void mx6_quantize_rows_kernel(const uint16_t* __restrict__ X, const int16_t* __restrict__ idx,
                                                                        uint8_t* __restrict__ Q, uint8_t* __restrict__ SF, int rows, int KQ,
                                                                        int KE) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ __attribute__((aligned(16))) uint2 image[3 * kMx6Threads];
  uint16_t* row_lds = reinterpret_cast<uint16_t*>(smem);
  const int tid = threadIdx.x;
  const int K = KQ + KE;
  const int Kp = (K + 127) & ~127;
  const int B = KQ >> 5;                 // source blocks of the reordered row
  const int P = (KQ - KE) >> 5;          // first block of the outlier tail
  const int Bp = Kp >> 5;                // scale bytes per row
  const int chunks = KQ >> 3;
  // blockIdx.y owns a range of the row's blocks (every workgroup stages the whole row: the gather may touch any channel)
  const int b_per = (B + (int)gridDim.y - 1) / (int)gridDim.y;
  const int b_begin = (int)blockIdx.y * b_per;
  const int b_end = min(B, b_begin + b_per);
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    const uint16_t* xrow = X + (size_t)row * KQ;
    for (int c = tid; c < chunks; c += kMx6Threads) lds_put_chunk(row_lds, c, *reinterpret_cast<const uint4*>(xrow + (size_t)c * 8));
    __syncthreads();
    uint8_t* qrow = Q + (size_t)row * (size_t)(Bp * 24);
    uint8_t* srow = SF + (size_t)row * Bp;
    for (int bb = b_begin; bb < b_end; bb += kMx6Threads) {
      const int n = min(kMx6Threads, b_end - bb);          // blocks of this pass
      const int b = bb + tid;
      const bool has = tid < n, tail = has && b >= P;
      float v[32];
      Mx6Block q;
      if (has) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {        // two 16-index loads per half block
          const uint4 i0 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16);
          const uint4 i1 = *reinterpret_cast<const uint4*>(idx + (size_t)b * 32 + h * 16 + 8);
          const uint32_t iw[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t pw = lds_pad_pair(iw[j]);
            v[16 * h + 2 * j] = bf16_bits_to_f32(row_lds[pw & 0xffffu]);
            v[16 * h + 2 * j + 1] = bf16_bits_to_f32(row_lds[pw >> 16]);
          }
        }
        q = (!kModeW && tail) ? mx6_quantize_block<true>(v) : mx6_quantize_block<false>(v);
        mx6_put_block(image, tid, q);
        srow[b] = (uint8_t)q.s8;
      }
      __syncthreads();
      mx6_copy_out(qrow + (size_t)bb * 24, image, 3 * n, tid);
      const int t0 = max(bb, P), t1 = bb + n;              // the pass's blocks of the outlier tail: [t0, t1)
      if (t0 < t1) {
        uint8_t* dst = qrow + (size_t)(B + (t0 - P)) * 24;
        if (kModeW) {
          if (tail) srow[B + (b - P)] = (uint8_t)q.s8;
          mx6_copy_out(dst, image + 3 * (t0 - bb), 3 * (t1 - t0), tid);
        } else {
          __syncthreads();                                 // the primary copy has left the image
          if (tail) {
            const Mx6Block r = mx6_quantize_block<false>(v);
            mx6_put_block(image, b - t0, r);
            srow[B + (b - P)] = (uint8_t)r.s8;
          }
          __syncthreads();
          mx6_copy_out(dst, image, 3 * (t1 - t0), tid);
        }
      }
      __syncthreads();                                     // the image is rewritten by the next pass
    }
    // the padding blocks [K/32, Bp) (none or two): code 0, scale 2^0, by the workgroup of the row's first range
    if (blockIdx.y == 0 && tid < Bp - (K >> 5)) {
      const int pb = (K >> 5) + tid;
#pragma unroll
      for (int j = 0; j < 3; ++j) *reinterpret_cast<uint2*>(qrow + (size_t)pb * 24 + j * 8) = make_uint2(0, 0);
      srow[pb] = 127;
    }
    __syncthreads();   // row_lds is rewritten by the next row
  }
}

// (the grid is quant_grid over the row's 32-element blocks, the checks are arcq_mx_quantize_x's)
template <bool kModeW>
static int mx6_launch(const void* X, const int16_t* idx, uint8_t* Q, uint8_t* SF, int64_t rows, int64_t KQ, int64_t KE, hipStream_t stream,
                      const char* who) {
  QuantRule r{who};
  r.family = kQuantMx;
  if (const int rc = quant_checks(r, QuantArgs{X, nullptr, idx, Q, SF, rows, KQ, KE})) return rc < 0 ? rc : ARCQ_OK;
  return launch_kernel<mx6_quantize_rows_kernel<kModeW>>(quant_grid(rows, KQ / 32), dim3(kMx6Threads), (int)lds_row_bytes((size_t)KQ), stream, who,
                                                         (const uint16_t*)X, idx, Q, SF, (int)rows, (int)KQ, (int)KE);
}

int mx6_quantize_x(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, hipStream_t stream) {
  return mx6_launch<false>(X, idx, QX, SFX, M, KQ, KE, stream, "arcq_mx6_quantize_x");
}
int mx6_quantize_w(const void* W, const int16_t* idx, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE, hipStream_t stream) {
  return mx6_launch<true>(W, idx, QW, SFW, N, KQ, KE, stream, "arcq_mx6_quantize_w");
}

}  // namespace arcq
