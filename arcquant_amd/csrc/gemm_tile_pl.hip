// The paired-load sibling of the LDS-tiled GEMM's overlapped-tail kernel (gemm_tile_body.inc, kPairLoads: the even K step requests a
// row's two following K atoms back to back and the odd K step requests nothing): plain epilogue, both B layouts, with its launchers and
// the debug setter that selects it -- in a translation unit of its own, so that the other units compile what they compiled before.
#include <type_traits>

#include "gemm_tile_common.hpp"

namespace arcq {

template <int BM, int BN, int WAVES_M, int WAVES_N, int kEpi, int kBLayout, int kEpiOps>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_tile_pl_kernel(TileParams p) {
  static_assert(kEpi == kEpiPlain && kEpiOps >= 0 && kEpiOps < 4, "bit 0 bias, bit 1 residual (SiLU * up keeps gemm_tile_ot_kernel)");
  constexpr bool kMfma32 = false, kStagger = false, kPipe = true, kOverlapTail = true, kPairLoads = true;
#define ARCQ_TILE_BODY_PAIR_LOADS     // this kernel alone declares the third register set and load_pair
#include "gemm_tile_body.inc"
#undef ARCQ_TILE_BODY_PAIR_LOADS
}

static int g_tile_pair_loads = 1;
int tile_pair_loads_mode() { return g_tile_pair_loads; }
// DEBUG / test control, read at every launch: 1 = a launch that is eligible for the overlapped tail (arcq_debug_set_tile_overlap_tail's
// rule) with the plain epilogue takes gemm_tile_pl_kernel, 0 = it takes gemm_tile_ot_kernel
extern "C" void arcq_debug_set_tile_pair_loads(int on) { g_tile_pair_loads = on != 0; }

template <int kBLayout, int kEpiOps>
static int launch_pl(const TileParams& p, dim3 grid, hipStream_t stream) {
  return launch_kernel<gemm_tile_pl_kernel<256, 256, 2, 4, kEpiPlain, kBLayout, kEpiOps>>(grid, dim3(512), 2 * (256 + 256) * kRowBytes, stream,
                                                                                        "arcq_gemm_nvfp4 (tile, paired loads)", p);
}
template <int kBLayout>
static int launch_pl_ops(const TileParams& p, dim3 grid, hipStream_t stream) {
  switch ((p.bias ? 1 : 0) | (p.residual ? 2 : 0)) {
    case 1: return launch_pl<kBLayout, 1>(p, grid, stream);
    case 2: return launch_pl<kBLayout, 2>(p, grid, stream);
    case 3: return launch_pl<kBLayout, 3>(p, grid, stream);
    default: return launch_pl<kBLayout, 0>(p, grid, stream);
  }
}
int launch_tile_pair_loads(const TileParams& p, int b_layout, dim3 grid, hipStream_t stream) {
  return b_layout == kBRepacked ? launch_pl_ops<kBRepacked>(p, grid, stream) : launch_pl_ops<kBRef>(p, grid, stream);
}

}  // namespace arcq
