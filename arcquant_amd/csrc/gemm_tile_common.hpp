// Pieces shared by the tile GEMM kernels (gemm_tile.hip, gemm_tile_ws.hip): parameter block, LDS tile
// addressing, the register staging unit and its dequantising store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_internal.hpp"
#include "gemm_common.hpp"

namespace arcq {

struct TileParams {
  const uint8_t* A;
  const uint8_t* B;
  const uint8_t* SFA;
  const uint8_t* SFB;
  void* D;
  const float* alpha_dev;
  const uint16_t* bias;
  const uint16_t* residual;
  int M, N, K;
  float alpha_host;
  int out_dtype;
  int tiles_m, tiles_n;
  // split-K (shapes whose tiles alone leave CUs idle): workgroup blockIdx.x / (tiles_m*tiles_n) owns the scale-factor
  // atoms [split*atoms_per_split, +atoms_per_split) and writes raw fp32 sums to partial[split][M][N]
  int splits, atoms_per_split;
  float* partial;
  // epilogue ARCQ_EPI_SILU_MUL: weight rows interleave gate and up (g0,u0,g1,u1,...), D is the bf16 [M, N/2] tensor
  // silu(gate)*up and slots[blockIdx.x] receives this workgroup's max |D| (bit pattern) for the dynamic quantiser
  int epi;
  unsigned int* slots;
#ifdef ARCQ_STREAM_STAMPS      // DIAGNOSTIC build only (make diag): [workgroup][kTileStamps][2] = s_memtime / s_memrealtime at the phase boundaries of a tile
  unsigned long long* stamps;
#endif
};
constexpr int kTileStamps = 5;          // kernel entry, K loop starts, K loop ends, first / last output store issued (gemm_tile.hip)
// gemm_tile_ot.hip: launches gemm_tile_ot_kernel<256, 256, 2, 4, epi, b_layout> (the caller has checked that the launch is eligible)
int launch_tile_overlap_tail(const TileParams& p, int epi, int b_layout, dim3 grid, hipStream_t stream);
// gemm_tile_pl.hip: launches gemm_tile_pl_kernel<256, 256, 2, 4, kEpiPlain, b_layout> (a launch eligible for the overlapped tail, plain epilogue)
int launch_tile_pair_loads(const TileParams& p, int b_layout, dim3 grid, hipStream_t stream);

constexpr int kBK = 64;                 // K elements per step = one scale-factor atom column (4 groups)
constexpr int kRowBytes = kBK * 2;      // fp16 row of a tile in LDS

// Byte offset of 16-byte slot `ks` (0..7) of tile row `r`.  XOR with (r & 7):
//   * ds_read_b128 of an MFMA fragment (16 rows x one slot per 16-lane group) touches all 16 slots of the
//     256-byte bank row exactly once  -> conflict-free;
//   * ds_write_b128 of the staging pass (8-lane groups = 4 rows x 2 halves) touches all 8 slots of the
//     128-byte write bank period exactly once -> conflict-free.
// The term is invariant under r += 16, so fragment tile i is a constant byte offset from tile 0.
__device__ __forceinline__ int lds_slot(int r, int ks) { return r * kRowBytes + ((ks ^ (r & 7)) << 4); }
// Variant for 32-row MFMA fragments (v_mfma_f32_32x32x16_f16): a 16-lane ds_read_b128 group then spans rows
// {0-3,12-15,20-27} of ONE slot, which needs ((r >> 1) & 7) to stay conflict-free (invariant under r += 32).
__device__ __forceinline__ int lds_slot32(int r, int ks) { return r * kRowBytes + ((ks ^ ((r >> 1) & 7)) << 4); }

// One staging unit = 16 packed bytes (32 elements, two scale groups) of one tile row.
struct Staged {
  uint4 q;
  uint32_t sf;   // the two scale bytes in bits [15:0]
};

// Unconditional loads (row clamped into the matrix, dead rows neutralised through their scale bytes at
// dequantisation time): nothing here waits on a load, so the prefetch stays in flight across the MFMAs.
//
// Every staging address is [workgroup-uniform tile base] + [lane offset, fixed for the launch] + [byte offset of the K step, uniform].
// Only the last term moves, so the loads are BUFFER loads: the base sits in a descriptor (four SGPRs), the lane offset is a 32-bit VGPR
// computed once ahead of the loop and the step offset is the instruction's scalar offset -- no vector instruction forms an address
// inside the K loop.  (Spelled as uniform pointer + 32-bit lane offset through global loads, hipcc folds base and lane offset back into
// 64-bit lane pointers and adds the step to each with a 64-bit vector add in front of every load.)
// A descriptor covers the rows of ITS TILE that lie inside the operand, no more; every address the kernel forms (rows clamped, the K
// index clamped) is inside it, so nothing relies on what a buffer load returns out of range.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t buf_rsrc;

// `base` and `bytes` must be workgroup-uniform IN THE COMPILER'S EYES (kernel arguments, readfirstlane results and arithmetic on them):
// a descriptor it cannot prove uniform gets a readfirstlane loop around every load.
__device__ __forceinline__ buf_rsrc stage_rsrc(const uint8_t* base, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), 0, (int)bytes, 0x00020000);
}

struct StageSrc {        // one operand's codes and scale bytes: descriptors at the tile origin
  buf_rsrc q, sf;
};
struct StageStep {       // byte offsets of one K atom against the tile origin (SGPRs)
  uint32_t q, sf;
};
// reference layout: 32 code bytes per atom and row, 512 scale bytes per atom and block of 128 rows
__device__ __forceinline__ StageStep stage_step(int atom) { return {(uint32_t)atom * 32u, (uint32_t)atom * 512u}; }
// REPACKED weight (arcq.h, agemm.repack_w; T = K rounded up to 256, over 128): the 16 bytes of half h of row 16 rb + r in atom a sit at
// RW + rb T 1024 + a 512 + h 256 + r 16, their two scale bytes at RSF + rb (T/2) 256 + (a >> 2) 256 + (2 (a & 1) + h) 64 + r 4 +
// ((a >> 1) & 1) 2.  The lane offsets hold the atom-independent terms; the bytes are the reference's.
__device__ __forceinline__ StageStep stage_step_rw(int atom) {
  return {(uint32_t)atom * 512u, (uint32_t)((atom >> 2) * 256 + (atom & 1) * 128 + ((atom >> 1) & 1) * 2)};
}
__device__ __forceinline__ Staged stage_load(const StageSrc& src, uint32_t q_lane, uint32_t sf_lane, StageStep step) {
  Staged s;
  const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(src.q, (int)q_lane, (int)step.q, 0);
  s.q = make_uint4(q.x, q.y, q.z, q.w);
  s.sf = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(src.sf, (int)sf_lane, (int)step.sf, 0);
  return s;
}
// the two halves of stage_load on their own (gemm_tile_pl.hip orders the code loads of two atoms ahead of their scale loads)
__device__ __forceinline__ uint4 stage_load_q(const StageSrc& src, uint32_t q_lane, StageStep step) {
  const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(src.q, (int)q_lane, (int)step.q, 0);
  return make_uint4(q.x, q.y, q.z, q.w);
}
__device__ __forceinline__ uint32_t stage_load_sf(const StageSrc& src, uint32_t sf_lane, StageStep step) {
  return (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(src.sf, (int)sf_lane, (int)step.sf, 0);
}

// The two scale bytes of a unit -> ONE register: the fp16 pair (s0', s1') of sf_pair's values (byte << 7 in each half).  Shifting the
// 16 bits by 7 puts byte 0 in place, by 15 byte 1; the AND that takes the seven magnitude bits of each is also the live-row mask
// (kSfLive for a row inside the matrix, 0 outside: both scales then read 0) -- three vector instructions per unit.  A quarter of the
// unit multiplies by the low or the high half, broadcast through the packed multiply's op_sel.
constexpr uint32_t kSfLive = 0x3f803f80u;
__device__ __forceinline__ f16x2 sf_pair_both(uint32_t sf16, uint32_t live_mask) {
  const uint32_t w = ((sf16 << 7) | (sf16 << 15)) & live_mask;
  f16x2 r;
  __builtin_memcpy(&r, &w, 4);
  return r;
}
template <int kHalf>
__device__ __forceinline__ f16x2 sf_splat(f16x2 s) { return __builtin_shufflevector(s, s, kHalf, kHalf); }

// One quarter (8 elements, one 16-byte slot) of a staging unit: lets the K loop spread the dequantisation between its
// MFMA groups.
__device__ __forceinline__ void stage_piece(unsigned char* tile, int slot, const Staged& s, uint32_t live_mask, int j) {
  const uint32_t w = j == 0 ? s.q.x : j == 1 ? s.q.y : j == 2 ? s.q.z : s.q.w;
  const f16x2 sf = sf_pair_both(s.sf, live_mask);
  const Frag8 f = dequant8(w, j < 2 ? sf_splat<0>(sf) : sf_splat<1>(sf));
  *reinterpret_cast<uint4*>(tile + slot) = f.u;
}

#if defined(ARCQ_EXPERIMENT_A_RAW) || defined(ARCQ_EXPERIMENT_B_RAW)
// TIMING EXPERIMENT ONLY (tools/scripts/build_variant_lib.sh; results are WRONG): the A panel (activations) staged WITHOUT its
// dequantisation -- what a tile GEMM reading pre-dequantised fp16 activations (emitted by the quantiser) could gain at most
__device__ __forceinline__ void stage_piece_raw(unsigned char* tile, int slot, const Staged& s, uint32_t live_mask, int j) {
  const uint32_t w = (j == 0 ? s.q.x : j == 1 ? s.q.y : j == 2 ? s.q.z : s.q.w) & (live_mask ? 0x3bff3bffu : 0u);   // finite fp16 patterns
  *reinterpret_cast<uint4*>(tile + slot) = make_uint4(w, w, w, w);
}
#endif

__device__ __forceinline__ void stage_store(unsigned char* tile, const int (&slot)[4], const Staged& s, uint32_t live_mask) {
  const f16x2 sf = sf_pair_both(s.sf, live_mask);
  const f16x2 s0 = sf_splat<0>(sf), s1 = sf_splat<1>(sf);
  Frag8 f0 = dequant8(s.q.x, s0), f1 = dequant8(s.q.y, s0), f2 = dequant8(s.q.z, s1), f3 = dequant8(s.q.w, s1);
  *reinterpret_cast<uint4*>(tile + slot[0]) = f0.u;
  *reinterpret_cast<uint4*>(tile + slot[1]) = f1.u;
  *reinterpret_cast<uint4*>(tile + slot[2]) = f2.u;
  *reinterpret_cast<uint4*>(tile + slot[3]) = f3.u;
}


}  // namespace arcq
