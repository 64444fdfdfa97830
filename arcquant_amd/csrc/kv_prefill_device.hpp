// What the two causal prefill kernels share (kv_prefill.hip over int4 pages, kv_prefill16.hip over 16-bit pages): the description of the
// work split and of the MFMA roles, the tile constants and the reasoning behind the LDS strides, and the
// launcher's arithmetic.  The MFMA wrappers, the rounding of the weights and the lane exchanges are kv_device.hpp's.  The tile walk, the
// query load, the two MFMA groups, the rescale step and the store loop are written out in both kernels: moved into functions here they
// changed the kernels' device code (profiles/kv_attn_shared_isa_identity.txt lists the forms that were tried).
//
//   Work split.  grid (tiles, N * chunks), 256 threads = 4 waves.  A workgroup owns a tile of 128 query-row slots of one (sequence, kv
//   head): slot r is (token r / hc of the tile, head ch * hc + r % hc of the kv head's group), hc = min(g, 128) heads per chunk and tpt =
//   128 / hc tokens per tile, so the g heads of a group share every K / V block.  Tiles are found on the device: workgroup x walks
//   qo_indptr, sequence b owning ceil(n_b / tpt) of them, and leaves when it runs out of sequences (the launch has ceil(ntok / tpt) + B: at
//   most one partial tile per sequence).  A wave owns 32 slots and keeps its query rows in registers.  Blocks of 32 kv positions wholly
//   above the tile's last query position are never visited; a wave skips the MFMAs of blocks above its own.
//
//   MFMA roles.  S^T = K Q^T: K (or its codes) from LDS is the A operand, the wave's 32 query rows (registers, loaded once) the B operand,
//   so lane (i, h) = (lane % 32, lane / 32) holds query column i and positions 8 (r >> 2) + 4 h + (r & 3) in accumulator registers r =
//   0..15.  Eight MFMAs.  The softmax is online, per lane + one exchange with lane i + 32; the causal mask is a select on the score and on
//   the weight; the accumulators are rescaled only in a block that moved some lane's maximum.  O^T += V^T P^T: registers 8 s .. 8 s + 7 of
//   the weight tile, rounded once to the 16-bit type, are the B fragment of k-step s with no lane movement; V^T comes from LDS as
//   [d][position'] with position' = position with bits 2 and 3 swapped, which is the k order in which the score tile presents its rows.
//   The row sum is an fp32 VALU sum over the unrounded weights.  O^T leaves lane (i, h) holding four consecutive d per register group:
//   8-byte stores (zeros when the row sum is 0).
//
//   LDS strides.  K rows are 136 elements (272 bytes = 68 banks of 4 bytes) apart: a 16-byte fragment read of lane (i, h) starts at
//   bank 4 i + const (mod 64), so 16 lanes of consecutive i cover the 64 banks once.  V^T rows are 40 elements (80 bytes = 20 banks)
//   apart: a fragment read starts at bank 20 i + const and i -> 5 i (mod 16) permutes the sixteen 4-bank groups.  (What the strides do
//   for a kernel's staging writes is said in that kernel.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kPfRows = 128;       // query-row slots of a tile
constexpr int kPfBlk = 32;         // kv positions per block
constexpr int kPfKStride = 136;    // 16-bit elements of a K row in LDS: 272 bytes, consecutive rows four banks apart
constexpr int kPfVStride = 40;     // of a V^T row: 80 bytes
constexpr int kPfShare = 32;       // lanes i and i + 32 hold one query row (kv_device.hpp's SHARE)

// ---- launcher: the fields KvPrefillParams and KvPrefill16Params have in common, and the grid that goes with them
template <class Params>
inline void kv_prefill_fill(Params& p, const KvPrefillArgs& a) {
  p.o = a.o; p.q = a.q; p.qo_indptr = a.qo_indptr; p.data = (const uint8_t*)a.kv_data;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.B = (int)a.B; p.Nq = (int)a.Nq; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.g = (int)(a.Nq / a.N);
  p.hc = p.g < kPfRows ? p.g : kPfRows;
  p.tpt = kPfRows / p.hc;
  p.chunks = (p.g + p.hc - 1) / p.hc;
  p.sm_scale = kKvSmScaleLog2;
}
template <class Params>
inline dim3 kv_prefill_grid(const Params& p, const KvPrefillArgs& a) {
  const int64_t tiles = (a.ntok + p.tpt - 1) / p.tpt + a.B;
  return dim3((unsigned)tiles, (unsigned)(a.N * p.chunks));
}

}  // namespace arcq
