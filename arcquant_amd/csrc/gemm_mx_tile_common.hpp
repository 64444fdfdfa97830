// What the MXFP4 GEMM kernels with an LDS stage or a quantising epilogue share, whichever layout the weight comes in (gemm_mx.hip: the
// reference layout; gemm_mx_tile_rw.hip and gemm_mx_slice_rw.hip: the repacked weight of arcq.h "MXFP4 repacked weight"): the tile's
// geometry and LDS image, and the quantiser of one (row, block) of the activation.  The kernels' statements themselves are shared as
// text: gemm_mx_tile_body.inc (the tiled kernel) and gemm_mx_slice_finish.inc (the end of the M <= kMxSmallM quantising kernels).
#pragma once
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

// ---------------------------------------------------------------------------------------------------------------- M <= kMxSmallM, quantising
// A workgroup of the quantising small-M kernels owns 64 y-columns = one 32-block of activations per row: four 16-column fragments.  The
// activations go through LDS in rows of 64 bytes padded to 80 (20 r mod 64 is a different multiple of 4 for each of the 16 rows).
constexpr int kMxSliceCols = 64;
constexpr int kMxSliceFrags = kMxSliceCols / 16;
constexpr int kMxSliceActRowBytes = 32 * 2 + 16;

// The K steps of one MRSF round (arcq.h "MXFP4 repacked weight"): 8 waves x the 4 bytes of a dword
constexpr int kMxRwRoundSteps = kMxSmallWaves * 4;

// gemm_mx_slice_rw.hip: the quantising kernel for 1 <= M <= kMxSmallM over p.B / p.SFB = MRW / MRSF (called by gemm_mx_tile_rw.hip)
int gemm_mx_slice_rw_quantize(const MxArgs& p, const char* who, hipStream_t stream);

}  // namespace arcq
