// The kOverlapTail kernel of the LDS-tiled GEMM's 256 x 256 8-wave tile (gemm_tile_body.inc: the final step and the output stores under
// its MFMAs): plain and SiLU * up, both B layouts, with its launchers and the debug setter that selects it -- in a translation unit of
// its own, so that the units of gemm_tile_kernel compile what they compiled before.
#include <type_traits>

#include "gemm_tile_common.hpp"

namespace arcq {

template <int BM, int BN, int WAVES_M, int WAVES_N, int kEpi, int kBLayout, int kEpiOps>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_tile_ot_kernel(TileParams p) {
  static_assert(kEpiOps >= 0 && kEpiOps < (kEpi == kEpiSiluMul ? 2 : 4), "bit 0 bias, bit 1 residual (SiLU * up has no residual)");
  constexpr bool kMfma32 = false, kStagger = false, kPipe = true, kOverlapTail = true, kPairLoads = false;
#include "gemm_tile_body.inc"
}

static int g_tile_overlap_tail = 1;
int tile_overlap_tail_mode() { return g_tile_overlap_tail; }
// DEBUG / test control, read at every launch: 0 = never take this kernel, 1 = launches of the 256 x 256 8-wave tile whose tiles are all
// interior (launch_tile; not SiLU * up), 2 = whenever legal: SiLU * up too, and every shape with M % 256 == 0 and N % 256 == 0 takes that
// tile, whatever the routes and heuristics say
extern "C" void arcq_debug_set_tile_overlap_tail(int mode) { g_tile_overlap_tail = mode < 0 ? 0 : mode > 2 ? 2 : mode; }

template <int kEpi, int kBLayout, int kEpiOps>
static int launch_ot(const TileParams& p, dim3 grid, hipStream_t stream) {
  return launch_kernel<gemm_tile_ot_kernel<256, 256, 2, 4, kEpi, kBLayout, kEpiOps>>(grid, dim3(512), 2 * (256 + 256) * kRowBytes, stream,
                                                                                   "arcq_gemm_nvfp4 (tile, overlapped tail)", p);
}
template <int kEpi, int kBLayout>
static int launch_ot_ops(const TileParams& p, dim3 grid, hipStream_t stream) {
  const int ops = (p.bias ? 1 : 0) | (p.residual ? 2 : 0);
  if constexpr (kEpi == kEpiSiluMul) {
    return ops & 1 ? launch_ot<kEpi, kBLayout, 1>(p, grid, stream) : launch_ot<kEpi, kBLayout, 0>(p, grid, stream);
  } else {
    switch (ops) {
      case 1: return launch_ot<kEpi, kBLayout, 1>(p, grid, stream);
      case 2: return launch_ot<kEpi, kBLayout, 2>(p, grid, stream);
      case 3: return launch_ot<kEpi, kBLayout, 3>(p, grid, stream);
      default: return launch_ot<kEpi, kBLayout, 0>(p, grid, stream);
    }
  }
}
int launch_tile_overlap_tail(const TileParams& p, int epi, int b_layout, dim3 grid, hipStream_t stream) {
  if (epi == kEpiSiluMul) return b_layout == kBRepacked ? launch_ot_ops<kEpiSiluMul, kBRepacked>(p, grid, stream) : launch_ot_ops<kEpiSiluMul, kBRef>(p, grid, stream);
  return b_layout == kBRepacked ? launch_ot_ops<kEpiPlain, kBRepacked>(p, grid, stream) : launch_ot_ops<kEpiPlain, kBRef>(p, grid, stream);
}

}  // namespace arcq
