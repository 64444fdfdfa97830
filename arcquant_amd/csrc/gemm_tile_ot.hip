// The kOverlapTail sibling of the LDS-tiled GEMM's 256 x 256 8-wave kernel (gemm_tile.hip: gemm_tile_ot_kernel, final step and output
// stores under its MFMAs): plain and SiLU * up, both B layouts, with the debug setter that selects it -- in a translation unit of its
// own, so that the two units of gemm_tile.hip compile what they compiled before.
#define ARCQ_TILE_OT_UNIT
#include "gemm_tile.hip"
