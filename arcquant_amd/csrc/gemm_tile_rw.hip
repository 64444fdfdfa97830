// The LDS-tiled GEMM over a REPACKED weight (B = RW, SFB = RSF of arcq.h): gemm_tile.hip's kernel template with kBLayout = kBRepacked,
// for every configuration gemm_tile.hip can select, in a translation unit of its own so that the two halves compile in parallel.
#define ARCQ_TILE_REPACKED_UNIT
#include "gemm_tile.hip"
