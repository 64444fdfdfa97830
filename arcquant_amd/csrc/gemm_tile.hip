// The LDS-tiled GEMM (design and file layout: gemm_tile_common.hpp): the host dispatch -- tile configurations, the tuning knobs, the
// shape -> tile rule, split-K and the sizes that follow from them -- defined here ONCE for every unit, and the instantiations of
// gemm_tile_kernel over B in the reference layout.
#include "gemm_tile_launch.hpp"

namespace arcq {

#ifdef ARCQ_STREAM_STAMPS
unsigned long long* g_tile_stamps = nullptr;
extern "C" void arcq_debug_set_tile_stamps(void* p) { g_tile_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

// ---- tile configurations --------------------------------------------------------------------------------------------------
// id = the value of ARCQ_TILE_CFG that forces it (debug / tuning only; 0 = heuristic).
//   1 = 128x128 (4 waves), 2 = 256x256 (4 waves), 3 = 256x256 (8 waves), 4 = 128x256 (4 waves), 5 / 6 = 32x32x16 MFMA variants of
//   3 / 1, 7 = 64x256 (4 waves), 8 = 32x256 (4 waves), 9 = 1 without split-K; 8-wave tiles for the shapes between decode and
//   prefill: 10 = 128x256, 11 = 256x128, 12 = 128x128, 13 = 64x256, 14 = 64x128; 4-wave: 15 = 64x64, 16 = 64x128, 17 = 128x64
static constexpr TileCfg kTileCfgs[] = {{1, 128, 128, 4}, {2, 256, 256, 4}, {3, 256, 256, 8}, {4, 128, 256, 4}, {5, 256, 256, 8}, {6, 128, 128, 4},
                                        {7, 64, 256, 4}, {8, 32, 256, 4}, {9, 128, 128, 4}, {10, 128, 256, 8}, {11, 256, 128, 8}, {12, 128, 128, 8},
                                        {13, 64, 256, 8}, {14, 64, 128, 8}, {15, 64, 64, 4}, {16, 64, 128, 4}, {17, 128, 64, 4}};
const TileCfg& tile_cfg(int id) {
  for (const TileCfg& c : kTileCfgs)
    if (c.id == id) return c;
  return kTileCfgs[2];
}

static int tile_cfg_override() {                // ARCQ_TILE_CFG (tuning)
  static const int v = env_int("ARCQ_TILE_CFG", 0);
  return v;
}
static int tile_split_override() {              // ARCQ_TILE_SPLIT = forced split-K factor (tuning; 0 = by shape)
  static const int v = env_int("ARCQ_TILE_SPLIT", 0);
  return v;
}
bool tile_stagger() {
  static const int v = env_int("ARCQ_TILE_STAGGER", 0);
  return v != 0;
}
bool tile_pipe() {
  static const int v = env_int("ARCQ_TILE_PIPE", 1);
  return v != 0;
}

// Split-K factor of a tile shape: split while the tiles alone leave CUs idle, keeping >= 8 atoms (512 K elements)
// per split so that the prologue/epilogue stay amortised; needs N % 4 == 0 (16-byte partial stores).
void tile_split(int64_t M, int64_t N, int64_t K, int BM, int BN, int* splits, int* atoms_per_split) {
  const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  const int atoms = (int)(K / 64);
  int s = 1;
  if ((N % 4) == 0) {
    if (tile_split_override() > 0) s = min(tile_split_override(), max(atoms / 2, 1));
    else
      while (tiles * s < 256 && atoms / (s * 2) >= 8 && s < 32) s *= 2;
  }
  const int per = (atoms + s - 1) / s;
  *splits = (atoms + per - 1) / per;      // drop empty splits
  *atoms_per_split = per;
}

// Shape -> tile: 256x256 with 8 waves (one workgroup per CU, two waves per SIMD) once it yields enough tiles to
// fill the 256 CUs (measured, tools/gemm_sweep.py: 4096^2 1066 vs 762 TFLOP/s, 8192^2 1347 vs 984); otherwise
// 128x128 (two workgroups per CU), or a 64- / 32-row tile over 256 weight rows for M <= 64 / 32, each with split-K.
static int tile_choice(int64_t M, int64_t N, int64_t K) {
  const int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256);
  if (t256 >= 192) return 3;
  if (M <= 32) return 8;
  if (M <= 64) return 7;
  // 128 x 256 with 8 waves where it measured faster than 128 x 128 (profiles/r03_midm_tile_sweep.jsonl: M = 2048, N = 4096 65.7 against
  // 75.7 us, M = 512 31.8 / 37.0, M = 1024 46.2 / 50.3; K = 18944, N = 3584: M = 1024 155 / 164, M = 2048 282 / 307): one exact round of the
  // chip, half a round, few tiles, or a long K -- elsewhere 128 x 128 (two workgroups per CU) fills the ragged rounds better
  const int64_t t10 = ((M + 127) / 128) * ((N + 255) / 256);
  if (t10 <= 64 || t10 == 128 || (t10 > 224 && t10 <= 256) || (K >= 8192 && t10 >= 96 && t10 <= 256)) return 10;
  return 1;
}

int effective_cfg(int64_t M, int64_t N, int64_t K, bool* may_split) {
  int id = tile_cfg_override();
  if (id == 0) id = tile_overlap_tail_forced(M, N) ? 3 : tile_choice(M, N, K);
  id = tile_cfg(id).id;
  *may_split = !(id >= 2 && id <= 6) && id != 9;
  return id;
}

// workgroups (= abs-max slots) of the silu-mul epilogue, which never splits K
int64_t gemm_tile_silu_slots(int64_t M, int64_t N, int64_t K) {
  bool sp;
  const TileCfg& c = tile_cfg(effective_cfg(M, N, K, &sp));
  return ((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn);
}

int64_t gemm_tile_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  int s = 1, per = 0;
  bool sp;
  const TileCfg& c = tile_cfg(effective_cfg(M, N, K, &sp));
  if (sp) tile_split(M, N, K, c.bm, c.bn, &s, &per);
  return s > 1 ? (int64_t)s * M * N * (int64_t)sizeof(float) : 0;
}

int gemm_tile(const GemmArgs& a, hipStream_t stream) {
  if (a.b_layout == kBRepacked) return gemm_tile_repacked(a, stream);       // gemm_tile_rw.hip
  // the epilogue is a template parameter: the plain kernels do not carry the exp code of silu-mul
  return a.epilogue == kEpiSiluMul ? gemm_tile_epi<kEpiSiluMul, kBRef>(a, stream) : gemm_tile_epi<kEpiPlain, kBRef>(a, stream);
}

}  // namespace arcq
