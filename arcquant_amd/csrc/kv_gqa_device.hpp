// What the two GQA decode kernels share (kv_decode_gqa.hip over int4 pages, kv_decode_gqa16.hip over 16-bit pages): the work split's
// constants, the launch parameters and how the launchers fill them, the broadcast of a row index and the step that takes a block's maximum
// into the running softmax.  The MFMA wrappers, the rounding of the weights and the lane exchanges are kv_device.hpp's.  The work split,
// the two-buffer loop over a wave's blocks and the epilogue are written out in both kernels: moved into functions here they changed the
// kernels' device code (profiles/kv_attn_shared_isa_identity.txt lists the forms that were tried).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "kv_device.hpp"

namespace arcq {

constexpr int kGqWaves = 4;
constexpr int kGqBlk = 32;           // positions per block
constexpr int kGqHeads = 16;         // columns of the MFMA tile: the most query heads per kv head
constexpr int kGqRecStride = 132;    // floats of a (wave, head) record in LDS: 128 accumulators, max, sum, 2 of padding (16-byte rows)
constexpr int kGqMaxSlices = 64;
constexpr int kGqShare = 16 | 32;    // the four k-groups of a head are lanes i, i + 16, i + 32, i + 48 (kv_device.hpp's SHARE)

struct KvGqaParams {
  void* o;
  const void* q;
  const uint8_t* data;
  const uint32_t* param;
  KvTables t;
  float* ws;                // [B * Nq, S, kKvRec]
  int B, Nq, L, layer, N, P, S, g;
  float sm_scale;           // 128^-1/2 log2(e)
};

// the row index that lane src holds (ds_bpermute, no LDS memory)
__device__ __forceinline__ size_t gq_row_of(size_t row, int src) {
  const uint32_t rlo = (uint32_t)row, rhi = (uint32_t)((uint64_t)row >> 32);
  return (size_t)__shfl(rlo, src, 64) | ((size_t)__shfl(rhi, src, 64) << 32);
}

// A block's maximum mb (this lane's) joins the head's running maximum m; the row sum l, any further running sums and the accumulators are
// brought to the new maximum
template <int SHARE, class Acc, int NA, class... Sums>
__device__ __forceinline__ void kv_new_max(float mb, float& m, float& l, Acc (&acc)[NA], Sums&... sums) {
  mb = kv_row_max<SHARE>(mb);
  const float mn = fmaxf(m, mb), alpha = __builtin_amdgcn_exp2f(m - mn);
  m = mn;
  if (__any(alpha != 1.0f)) {                            // (wave-uniform: once the maxima have settled most blocks rescale nothing)
    l *= alpha;
    ((sums *= alpha), ...);
#pragma unroll
    for (int a = 0; a < NA; ++a) acc[a] *= alpha;
  }
}

// ---- launcher: everything of KvGqaParams but param (int4 only), and the grid
inline void kv_gqa_fill(KvGqaParams& p, const KvDecodeArgs& a) {
  p.o = a.o; p.q = a.q; p.data = (const uint8_t*)a.kv_data;
  p.t = {a.kv_indptr, a.kv_indices, a.last_page_offset};
  p.ws = (float*)a.workspace;
  p.B = (int)a.B; p.Nq = (int)a.Nq; p.L = (int)a.L; p.layer = (int)a.layer; p.N = (int)a.N; p.P = (int)a.P;
  p.g = (int)(a.Nq / a.N);
  p.S = kv_decode_gqa_splits(a.B, a.Nq, a.N, a.nnz, a.P);
  p.sm_scale = kKvSmScaleLog2;
}
inline dim3 kv_gqa_grid(const KvGqaParams& p, const KvDecodeArgs& a) { return dim3((unsigned)(a.B * a.N), (unsigned)p.S); }

}  // namespace arcq
