// Device pieces shared by the decode GEMMs over the REPACKED weight: gemm_rowblock.hip (image and direct kernels), gemm_rowmid.hip
// (rowmid and rowtok kernels) and gemm_stream.hip.  Plain functions and two small structs; every kernel keeps its own body -- the
// order of its requests, its sched_barriers, its by-name ring registers -- and calls these for text it used to repeat.
//
// What is here is what could move WITHOUT changing a kernel's assembly (profiles/rowblock_core_isa_identity.txt: all 26 kernels of
// the three units are the same text as before).  hipcc's register allocation follows the inlining structure closely: the same
// statements behind a function boundary gave other register numbers, or a few instructions more or fewer, for the work split of a
// wave, the K-tail clamps of the global-memory activations, the slice reduction, the epilogue prefetch and the three-deep ring loop
// (each tried in several forms: bool helper / return in the kernel, arrays by reference / scalars, structs / loose values).  Those
// stay written out in the kernels; gemm_stream.hip keeps a one-line `tile` lambda around tile_image for the same reason.
//
// Layout reminder (gemm_rowblock.hip has the full description): a weight TILE is 16 rows x 128 K in MFMA operand order, lane
// l = 16 q + r holds the 16 bytes of row r, K elements [32 q, 32 q + 32); a tile PAIR is 2 KB of codes and 256 bytes of scales (one
// dword per lane: the two ue4m3 bytes of its groups in either tile).
#pragma once
#include "gemm_common.hpp"
#include "rowblock_split.hpp"

namespace arcq {

typedef uint32_t rb_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rb_u32x2 __attribute__((ext_vector_type(2)));

// ---- weight stream ------------------------------------------------------------------------------------------------------------------
struct WeightPair {       // one tile pair of this lane: 2 x 16 bytes of codes, 4 scale bytes
  rb_u32x4 b0, b1;
  uint32_t s;
};

// pair i behind the lane's cursors wp (codes) and sp (scales)
__device__ __forceinline__ void weight_pair_load(WeightPair& r, const uint8_t* wp, const uint8_t* sp, int i) {
  // a weight byte is read once per launch by one CU: non-temporal loads (gemm_common.hpp)
  r.b0 = ARCQ_WLOAD(reinterpret_cast<const rb_u32x4*>(wp + (size_t)i * 2048));
  r.b1 = ARCQ_WLOAD(reinterpret_cast<const rb_u32x4*>(wp + (size_t)i * 2048 + 1024));
  r.s = ARCQ_WLOAD(reinterpret_cast<const uint32_t*>(sp + (size_t)i * 256));
}

// ---- one 16 x 128 tile against one token tile ---------------------------------------------------------------------------------------
struct TileFrags {        // a lane's four MFMA operand fragments of a 128-element tile
  Frag8 f0, f1, f2, f3;
};

// 16 packed bytes (32 codes) and the two ue4m3 bytes of their groups (bits 0 .. 15 of s16) -> fp16, exact (gemm_common.hpp).  Weights
// and packed activations have the same form.
__device__ __forceinline__ TileFrags tile_dequant(rb_u32x4 codes, uint32_t s16) {
  const f16x2 s0 = sf_pair_at(s16, 0), s1 = sf_pair_at(s16, 8);
  TileFrags t;
  t.f0 = dequant8(codes.x, s0); t.f1 = dequant8(codes.y, s0); t.f2 = dequant8(codes.z, s1); t.f3 = dequant8(codes.w, s1);
  return t;
}

// the lane's 64 bytes of an fp16 activation image
__device__ __forceinline__ TileFrags tile_from_image(const unsigned char* ap) {
  TileFrags t;
  t.f0.u = *reinterpret_cast<const uint4*>(ap);
  t.f1.u = *reinterpret_cast<const uint4*>(ap + 16);
  t.f2.u = *reinterpret_cast<const uint4*>(ap + 32);
  t.f3.u = *reinterpret_cast<const uint4*>(ap + 48);
  return t;
}

// weights are the MFMA A operand (rows = weight rows), activations the B operand (columns = tokens)
__device__ __forceinline__ f32x4 tile_mfma(const TileFrags& w, const TileFrags& a, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f0.v, a.f0.v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f1.v, a.f1.v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f2.v, a.f2.v, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f3.v, a.f3.v, acc, 0, 0, 0);
  return acc;
}

// weight tile (b, s16) against activation fragments from the LDS image
__device__ __forceinline__ f32x4 tile_image(rb_u32x4 b, uint32_t s16, const unsigned char* ap, f32x4 acc) {
  const TileFrags a = tile_from_image(ap);
  return tile_mfma(tile_dequant(b, s16), a, acc);
}

// ... against activation fragments from 16 packed bytes + 2 scale bytes
__device__ __forceinline__ f32x4 tile_packed(rb_u32x4 b, uint32_t s16, rb_u32x4 a, uint32_t as16, f32x4 acc) {
  const TileFrags x = tile_dequant(a, as16);
  return tile_mfma(tile_dequant(b, s16), x, acc);
}

// ---- activation image ---------------------------------------------------------------------------------------------------------------
// unit u = 32 elements (16 packed bytes qv, their two scale bytes in the atom's dword sf) -> 64 bytes of fp16; upr / real: units per
// token row, padded / real (the K padding is zeros)
__device__ __forceinline__ void image_put_unit(unsigned char* a_img, int a_stride, int u, int upr, int real, uint4 qv, uint32_t sf) {
  const int m = u / upr, c = u - m * upr;
  uint4 f0 = make_uint4(0, 0, 0, 0), f1 = f0, f2 = f0, f3 = f0;
  if (c < real) {
    sf >>= (c & 1) * 16;
    const f16x2 s0 = sf_pair_at(sf, 0), s1 = sf_pair_at(sf, 8);
    f0 = dequant8(qv.x, s0).u; f1 = dequant8(qv.y, s0).u; f2 = dequant8(qv.z, s1).u; f3 = dequant8(qv.w, s1).u;
  }
  uint4* dst = reinterpret_cast<uint4*>(a_img + (size_t)m * a_stride + c * 64);
  dst[0] = f0; dst[1] = f1; dst[2] = f2; dst[3] = f3;
}

}  // namespace arcq
