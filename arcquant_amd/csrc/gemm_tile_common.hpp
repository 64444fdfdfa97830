// ARC-NVFP4 GEMM for prefill shapes (M > 16): LDS-tiled fp16-MFMA kernel for gfx950.
//
// Replaces the CUTLASS sm120 block-scaled GEMM instantiation of the reference
// (kernels/src/nvfp4.cu:10-33,48-74: 128x128x128 tiles, mma.sync block_scale) with a CDNA4 design:
//
//   HBM/L2 --(packed e2m1 + ue4m3 bytes, 16 B per lane)--> VGPR --dequantise once per block-->
//   fp16 tiles in LDS (XOR-swizzled 128-byte rows) --ds_read_b128--> v_mfma_f32_16x16x32_f16
//
// Each operand byte crosses HBM/L2 in its 4.5-bit form (3.6x less traffic than an fp16 GEMM) and is
// expanded exactly once per workgroup; the MFMA mainloop is then an ordinary fp16 contraction whose
// products are exact (gemm_common.hpp), fp32 accumulate, alpha / bias / bf16 rounding fused in the
// epilogue.  The bound is the dense fp16/bf16 MFMA rate (~2.5 PFLOP/s), see DESIGN.md.
//
// Tile: BM x BN x 64, kThreads = 256 (2x2 wave64, each 64x64 = 4x4 MFMA tiles) or 512 (2x4 waves on
// 128x256).  Double-buffered LDS, one barrier per K step: the global loads of step k+1 are issued
// before the MFMAs of step k and written to the other buffer after them.
//
// The files:
//   gemm_tile_common.hpp  (this one) parameter block, LDS tile addressing, the register staging unit and its dequantising store, the
//                         declarations of the host dispatch
//   gemm_tile_body.inc    the kernel's statements, included inside the braces of each kernel definition
//   gemm_tile_launch.hpp  gemm_tile_kernel (the kept kernel) and the templates that launch a configuration of it
//   gemm_tile.hip         the host dispatch (shape -> tile, split-K, knobs), defined ONCE, and the reference-layout instantiations
//   gemm_tile_rw.hip      the repacked-weight instantiations (a unit of its own: the two long compiles run in parallel)
//   gemm_tile_ot.hip      gemm_tile_ot_kernel, the overlapped-tail kernel of the 256 x 256 8-wave tile, and its launchers
//   gemm_tile_pl.hip      gemm_tile_pl_kernel, its paired-load sibling, and its launchers
//   gemm_tile_ql.hip      gemm_tile_ql_kernel, the quad-load sibling of that one (reference B layout), and its launchers
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
constexpr int kTileStamps = 5;          // kernel entry, K loop starts, K loop ends, first / last output store issued (gemm_tile_body.inc)
// gemm_tile_ot.hip: launches gemm_tile_ot_kernel<256, 256, 2, 4, epi, b_layout> (the caller has checked that the launch is eligible)
int launch_tile_overlap_tail(const TileParams& p, int epi, int b_layout, dim3 grid, hipStream_t stream);
// gemm_tile_pl.hip: launches gemm_tile_pl_kernel<256, 256, 2, 4, kEpiPlain, b_layout> (a launch eligible for the overlapped tail, plain epilogue)
int launch_tile_pair_loads(const TileParams& p, int b_layout, dim3 grid, hipStream_t stream);
// gemm_tile_ql.hip: launches gemm_tile_ql_kernel<256, 256, 2, 4, kEpiPlain, kBRef> (a launch the paired-load kernel would take, reference B layout)
int launch_tile_quad_loads(const TileParams& p, dim3 grid, hipStream_t stream);

// ---- the host dispatch, defined once in gemm_tile.hip (library-internal: not among the exported names) ----------------------------
#pragma GCC visibility push(hidden)
struct TileCfg { int id, bm, bn, waves; };
const TileCfg& tile_cfg(int id);        // the configuration ARCQ_TILE_CFG = id forces; an unknown id gives 256 x 256 with 8 waves
bool tile_stagger();                    // ARCQ_TILE_STAGGER=0|1 (tuning)
bool tile_pipe();                       // ARCQ_TILE_PIPE=0|1 (tuning)
void tile_split(int64_t M, int64_t N, int64_t K, int BM, int BN, int* splits, int* atoms_per_split);
// the configuration a launch uses, and whether it may split K (the silu-mul epilogue never does; 2 - 6 and 9 are the unsplit tuning arms)
int effective_cfg(int64_t M, int64_t N, int64_t K, bool* may_split);
#ifdef ARCQ_STREAM_STAMPS
extern unsigned long long* g_tile_stamps;     // arcq_debug_set_tile_stamps; NULL: no launch is stamped
#endif
#pragma GCC visibility pop

#ifdef ARCQ_STREAM_STAMPS
// DIAGNOSTIC build only: the in-kernel clock of the K loop = delta s_memtime / delta s_memrealtime x 100 MHz
// (MI355X_MICROARCH.md, "DVFS give-back" item 6) and the phases of a tile, stamped by wave 0 of every workgroup into a buffer
// nothing else reads (tools/tile_clock.py): kTileStamps (s_memtime, s_memrealtime) pairs per workgroup -- 0 kernel entry, 1 K loop
// starts, 2 K loop ends, 3 first output store issued, 4 last output store issued.  The product library has no stamps.
#define ARCQ_TILE_STAMP(k)                                                                                     \
  do {                                                                                                         \
    if (p.stamps && tid == 0) {                                                                                \
      unsigned long long t0_, t1_;                                                                             \
      asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_), "=s"(t1_)::"memory"); \
      p.stamps[(size_t)blockIdx.x * (2 * kTileStamps) + 2 * (k)] = t0_;                                        \
      p.stamps[(size_t)blockIdx.x * (2 * kTileStamps) + 2 * (k) + 1] = t1_;                                    \
    }                                                                                                          \
  } while (0)
#else
#define ARCQ_TILE_STAMP(k) do { } while (0)
#endif

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
