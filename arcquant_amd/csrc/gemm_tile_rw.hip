// The LDS-tiled GEMM over a REPACKED weight (B = RW, SFB = RSF of arcq.h): gemm_tile_kernel with kBLayout = kBRepacked, for every
// configuration the host dispatch of gemm_tile.hip can select, in a translation unit of its own so that the two halves compile in parallel.
#include "gemm_tile_launch.hpp"

namespace arcq {

int gemm_tile_repacked(const GemmArgs& a, hipStream_t stream) {
  return a.epilogue == kEpiSiluMul ? gemm_tile_epi<kEpiSiluMul, kBRepacked>(a, stream) : gemm_tile_epi<kEpiPlain, kBRepacked>(a, stream);
}

}  // namespace arcq
