// The kept kernel of the LDS-tiled GEMM and the templates that launch one configuration of it.  Included by gemm_tile.hip, which
// instantiates them for the reference B layout, and by gemm_tile_rw.hip, which instantiates them for the repacked one; everything
// here is a template, so neither unit compiles what the other uses.  What a launch decides by shape (tile, split-K, knobs) is the one
// host dispatch of gemm_tile.hip, declared in gemm_tile_common.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "arcq_internal.hpp"
#include "gemm_common.hpp"
#include "gemm_tile_common.hpp"

namespace arcq {

template <int BM, int BN, int WAVES_M, int WAVES_N, bool kMfma32, int kEpi, bool kStagger, bool kPipe, int kBLayout = kBRef>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void gemm_tile_kernel(TileParams p) {
  constexpr bool kOverlapTail = false, kPairLoads = false;
  [[maybe_unused]] constexpr int kEpiOps = 0;
#include "gemm_tile_body.inc"
}

template <int BM, int BN, int WAVES_M, int WAVES_N, bool kMfma32 = false, int kEpi = kEpiPlain, int kBLayout = kBRef>
static int launch_tile(const GemmArgs& a, hipStream_t stream, bool allow_split = false) {
  TileParams p;
  copy_gemm_fields(p, a);
  p.B = a.B; p.SFB = a.SFB;
  p.tiles_m = (a.M + BM - 1) / BM;
  p.tiles_n = (a.N + BN - 1) / BN;
  p.splits = 1; p.atoms_per_split = a.K / 64; p.partial = nullptr;
  p.epi = a.epilogue; p.slots = a.absmax_slots;
#ifdef ARCQ_STREAM_STAMPS
  p.stamps = g_tile_stamps;
#endif
  if (allow_split && a.epilogue == kEpiPlain) {
    tile_split(a.M, a.N, a.K, BM, BN, &p.splits, &p.atoms_per_split);
    if (p.splits > 1) {
      const int64_t need = (int64_t)p.splits * a.M * a.N * (int64_t)sizeof(float);
      if (!a.workspace || a.workspace_bytes < need)
        return fail(ARCQ_ERR_WORKSPACE, "arcq_gemm_nvfp4: split-K needs %lld B of workspace, got %lld", (long long)need,
                    (long long)a.workspace_bytes);
      p.partial = reinterpret_cast<float*>(a.workspace);
    }
  }
  // the staging loads address an operand's tile with 32-bit offsets: up to 256 rows of K / 2 code bytes, or 16 row blocks of the repacked
  // weight (K rounded up to 256)
  if (((int64_t)a.K + 255) / 256 * 256 * 128 > 0xffffffffll)
    return fail(ARCQ_ERR_SHAPE, "arcq_gemm_nvfp4 (tile): K = %lld: a tile's rows of an operand exceed 32-bit offsets", (long long)a.K);
  const int lds = 2 * (BM + BN) * kRowBytes;
  const dim3 grid((unsigned)(p.tiles_m * p.tiles_n * p.splits)), block(WAVES_M * WAVES_N * 64);
  const char* who = "arcq_gemm_nvfp4 (tile)";
  constexpr bool kCanStagger = WAVES_M * WAVES_N == 8 && BM == 256 && BN == 256;
  const bool pipe = tile_pipe(), stagger = !pipe && kCanStagger && tile_stagger();      // the variants of the instantiation
  int rc;
  // the kOverlapTail kernel (gemm_tile_ot.hip) takes the rotated 256 x 256 8-wave step's launches whose tiles are ALL interior: the
  // kernel's own `interior` test, made once for the launch.  SiLU * up launches take theirs only under the debug setter's 2: it has not
  // measured faster than the kept kernel
  bool overlap_tail = false;
  if constexpr (BM == 256 && BN == 256 && WAVES_M * WAVES_N == 8 && !kMfma32)
    overlap_tail = pipe && (kEpi == kEpiSiluMul ? tile_overlap_tail_mode() == 2 : tile_overlap_tail_mode() != 0) && a.M % BM == 0 && a.N % BN == 0 && p.splits <= 1 && a.out_dtype == ARCQ_OUT_BF16 &&
                   (int64_t)BM * a.N < (1ll << 31) && ((reinterpret_cast<uintptr_t>(a.bias) | reinterpret_cast<uintptr_t>(a.residual)) & 7) == 0;
  // ... and of those the plain-epilogue launches take its paired-load sibling (gemm_tile_pl.hip) unless the debug setter says 0
  // ... and of those the launches over the reference B layout its quad-load sibling (gemm_tile_ql.hip) unless ITS debug setter says 0
  if (overlap_tail && kEpi == kEpiPlain && kBLayout == kBRef && tile_pair_loads_mode() != 0 && tile_quad_loads_mode() != 0) rc = launch_tile_quad_loads(p, grid, stream);
  else if (overlap_tail && kEpi == kEpiPlain && tile_pair_loads_mode() != 0) rc = launch_tile_pair_loads(p, kBLayout, grid, stream);
  else if (overlap_tail) rc = launch_tile_overlap_tail(p, kEpi, kBLayout, grid, stream);
  else if (!pipe && !stagger) rc = launch_kernel<gemm_tile_kernel<BM, BN, WAVES_M, WAVES_N, kMfma32, kEpi, false, false, kBLayout>>(grid, block, lds, stream, who, p);
  else if (pipe) rc = launch_kernel<gemm_tile_kernel<BM, BN, WAVES_M, WAVES_N, kMfma32, kEpi, false, true, kBLayout>>(grid, block, lds, stream, who, p);
  else rc = launch_kernel<gemm_tile_kernel<BM, BN, WAVES_M, WAVES_N, kMfma32, kEpi, kCanStagger, false, kBLayout>>(grid, block, lds, stream, who, p);
  if (rc != ARCQ_OK) return rc;
  if (p.splits > 1) return gemm_splitk_finish(a, p.splits, stream);
  return ARCQ_OK;
}

// (the configurations by id: the table in front of kTileCfgs, gemm_tile.hip)
template <int kEpi, int kBLayout>
static int gemm_tile_epi(const GemmArgs& a, hipStream_t stream) {
  bool sp;
  switch (effective_cfg(a.M, a.N, a.K, &sp)) {
    case 1: case 9: return launch_tile<128, 128, 2, 2, false, kEpi, kBLayout>(a, stream, sp);
    case 2: return launch_tile<256, 256, 2, 2, false, kEpi, kBLayout>(a, stream);
    case 4: return launch_tile<128, 256, 2, 2, false, kEpi, kBLayout>(a, stream);
    case 5: return launch_tile<256, 256, 2, 4, true, kEpi, kBLayout>(a, stream);
    case 6: return launch_tile<128, 128, 2, 2, true, kEpi, kBLayout>(a, stream);
    case 7: return launch_tile<64, 256, 1, 4, false, kEpi, kBLayout>(a, stream, sp);
    case 8: return launch_tile<32, 256, 1, 4, false, kEpi, kBLayout>(a, stream, sp);
    case 10: return launch_tile<128, 256, 2, 4, false, kEpi, kBLayout>(a, stream, sp);
    case 11: return launch_tile<256, 128, 4, 2, false, kEpi, kBLayout>(a, stream, sp);
    case 12: return launch_tile<128, 128, 2, 4, false, kEpi, kBLayout>(a, stream, sp);
    case 13: return launch_tile<64, 256, 1, 8, false, kEpi, kBLayout>(a, stream, sp);
    case 14: return launch_tile<64, 128, 2, 4, false, kEpi, kBLayout>(a, stream, sp);
    case 15: return launch_tile<64, 64, 2, 2, false, kEpi, kBLayout>(a, stream, sp);
    case 16: return launch_tile<64, 128, 2, 2, false, kEpi, kBLayout>(a, stream, sp);
    case 17: return launch_tile<128, 64, 2, 2, false, kEpi, kBLayout>(a, stream, sp);
    default: return launch_tile<256, 256, 2, 4, false, kEpi, kBLayout>(a, stream);
  }
}

}  // namespace arcq
