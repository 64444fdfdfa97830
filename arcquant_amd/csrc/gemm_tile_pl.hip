// The paired-load sibling of the LDS-tiled GEMM's 256 x 256 8-wave kernel (gemm_tile.hip: gemm_tile_pl_kernel, the overlapped-tail
// kernel whose even K step requests a row's two following K atoms back to back and whose odd K step requests nothing): plain epilogue,
// both B layouts, with the debug setter that selects it -- in a translation unit of its own, so that the units of gemm_tile.hip and
// gemm_tile_ot.hip compile what they compiled before.
#define ARCQ_TILE_PL_UNIT
#include "gemm_tile.hip"
