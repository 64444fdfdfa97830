// The quad-load sibling of the LDS-tiled GEMM's paired-load kernel (gemm_tile_body.inc, kQuadLoads: a loop iteration is four K steps, A's
// four following K atoms of a row are requested back to back in step 0 and B's in step 2, steps 1 and 3 request scale bytes alone): plain epilogue,
// reference B layout, with its launchers and the debug setter that selects it -- in a translation unit of its own, so that the other
// units compile what they compiled before.  Launches over the repacked weight keep gemm_tile_pl_kernel.
#include <type_traits>

#include "gemm_tile_common.hpp"

namespace arcq {

template <int BM, int BN, int WAVES_M, int WAVES_N, int kEpi, int kBLayout, int kEpiOps>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_tile_ql_kernel(TileParams p) {
  static_assert(kEpi == kEpiPlain && kBLayout == kBRef && kEpiOps >= 0 && kEpiOps < 4, "bit 0 bias, bit 1 residual; the reference layout's rows");
  constexpr bool kMfma32 = false, kStagger = false, kPipe = true, kOverlapTail = true, kPairLoads = true, kQuadLoads = true;
#define ARCQ_TILE_BODY_PAIR_LOADS     // the prologue's load_pair and the steps that request nothing are the paired-load kernel's
#define ARCQ_TILE_BODY_QUAD_LOADS     // this kernel alone declares the quad sets, load_quad_q / load_quad_sf and the four-step loop
#include "gemm_tile_body.inc"
#undef ARCQ_TILE_BODY_QUAD_LOADS
#undef ARCQ_TILE_BODY_PAIR_LOADS
}

static int g_tile_quad_loads = 1;
int tile_quad_loads_mode() { return g_tile_quad_loads; }
// DEBUG / test control, read at every launch: 1 = a launch that takes the paired-load kernel (arcq_debug_set_tile_pair_loads's rule) over
// the reference B layout takes gemm_tile_ql_kernel instead, 0 = it keeps gemm_tile_pl_kernel.  Inert while the paired-load setter is 0.
extern "C" void arcq_debug_set_tile_quad_loads(int on) { g_tile_quad_loads = on != 0; }

template <int kEpiOps>
static int launch_ql(const TileParams& p, dim3 grid, hipStream_t stream) {
  return launch_kernel<gemm_tile_ql_kernel<256, 256, 2, 4, kEpiPlain, kBRef, kEpiOps>>(grid, dim3(512), 2 * (256 + 256) * kRowBytes, stream,
                                                                                     "arcq_gemm_nvfp4 (tile, quad loads)", p);
}
int launch_tile_quad_loads(const TileParams& p, dim3 grid, hipStream_t stream) {
  switch ((p.bias ? 1 : 0) | (p.residual ? 2 : 0)) {
    case 1: return launch_ql<1>(p, grid, stream);
    case 2: return launch_ql<2>(p, grid, stream);
    case 3: return launch_ql<3>(p, grid, stream);
    default: return launch_ql<0>(p, grid, stream);
  }
}

}  // namespace arcq
