// The statements of the LDS-tiled GEMM kernel (design: gemm_tile_common.hpp), included inside the braces of a kernel definition.
//
// The kernel header in front of it supplies the template parameters BM, BN, WAVES_M, WAVES_N, kEpi, kBLayout, the parameter block
// `TileParams p`, and as template parameters or constants kMfma32, kStagger, kPipe, kOverlapTail, kPairLoads and kEpiOps (and kQuadLoads
// where ARCQ_TILE_BODY_QUAD_LOADS is defined: it is read behind that gate alone).
// ONE body text under several headers: the body as a __device__ __forceinline__ function called by the kernels made hipcc generate
// other code for every kernel, 0.3 - 0.9 % slower on the model's shapes (DESIGN.md 3.2); included as text, each kernel's code is what
// it was.
//
// kStagger (8-wave tiles): the two waves of a SIMD (w and w + 4) run half a step apart -- waves 0-3 multiply step k and
// then stage step k+1, waves 4-7 stage step k+2 FIRST (into the buffer step k was just read from, after the barrier)
// and then multiply step k+1 -- so that one wave's dequantise/ds_write phase overlaps the other's MFMA phase instead
// of both waves of a SIMD leaving the matrix pipe idle together.  ONE loop body with a barrier on either side of the
// staging block, each taken by one group (every wave still meets one barrier per step): no code is duplicated.
// kBLayout: kBRef = B / SFB in the reference layout, kBRepacked = the RW / RSF of arcq.h.  Only the addresses of B's staging loads
// differ: the staged bytes, the LDS image, the K order and every MFMA are the same, so the two produce identical sums.
// kOverlapTail (interior tiles of the rotated 256 x 256 8-wave step only): the last K step of the range is a FINAL step -- no loads, no
// staging, no barrier, pair-outer MFMA order -- and the interior epilogue of a pair of row tiles is issued under the MFMAs of the next
// pair, so that output leaves while the matrix pipe still works.  Every accumulator still takes its K half 0 MFMA before its K half 1
// one and the epilogue's operations are interior_epilogue's in its order: identical bits.  kEpiOps: the epilogue operands of such a
// launch, bit 0 bias, bit 1 residual -- chosen by the launcher (four straight-line copies of the final step behind uniform branches
// left hipcc's register allocation with spills).
// kPairLoads (with kOverlapTail): the staging loads of a row take 32 B of a 128-B line per K atom, a row per lane pair, so one
// wave-instruction touches 32 lines and the next atom of the same rows comes a whole K step later.  With kPairLoads the EVEN step of a
// pair of steps requests the code bytes of BOTH following atoms (kt + 2 and kt + 3), per unit back to back through the same descriptor
// and lane offset -- A's pair at the top of the step, B's ahead of block 2, the four scale loads ahead of block 4 -- and the ODD step
// requests nothing: still 8 loads per two steps, all ahead of the even step's barrier, every address formed the same way (clamped atom,
// inside the descriptor), but a row's two requests reach the vector L1 together (36 % fewer read requests to L2 per launch:
// profiles/tile_pair_loads_pmc.json).  A third register set (sa2 / sb2) holds atom kt + 2 across the even step; the odd step stages
// from it.  The staged bytes, the pieces and their blocks, the barrier, the LDS image, the K and MFMA order, the final step and the
// epilogue are the kOverlapTail kernel's: identical bits.  What only that kernel may DECLARE stands behind ARCQ_TILE_BODY_PAIR_LOADS,
// which its header defines in front of the include and undefines behind it.
// kQuadLoads (the paired-load kernel's text plus what stands behind ARCQ_TILE_BODY_QUAD_LOADS; reference B layout): a loop iteration is
// FOUR K steps and an operand's code bytes are requested a row-quad at a time -- atoms kt + 2 .. kt + 5 of a row (each clamped), per unit
// four 16-byte loads back to back through one descriptor and one lane offset: a whole 128-B line where the row starts one, two lines
// otherwise.  A's quad is requested at the top of step 0 of the iteration and B's ahead of block 2 of step 2, each followed two blocks
// later by the scale load of its FIRST atom; steps 1 and 3 request the other three scale pairs of the quad before them and no code
// bytes (16 loads per four steps, as before; with all four scale loads in the quad's own step hipcc spilled: three registers more at
// the step's end).  An iteration is entered with A's atom kt + 1 in sa and B's atoms kt + 1 .. kt + 3 in sb / yb (the prologue requests
// B's atoms 2 and 3 behind atoms 0 and 1): at most five sets of one operand and three of the other are live, 256 VGPRs, no scratch.
// The 1 - 3 steps left between the loop and the final step hold B's atoms already and request A's next atom one at a time, never an
// atom that no step stages.  Everything else is the paired-load kernel's: identical bits.
  constexpr int kThreads = WAVES_M * WAVES_N * 64;
  constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N;     // wave tile
  constexpr int kT = kMfma32 ? 32 : 16;                   // MFMA tile edge
  constexpr int TM = WM / kT, TN = WN / kT;               // MFMA tiles per wave
  using acc_t = typename std::conditional<kMfma32, f32x16, f32x4>::type;
  // 16-byte staging units per thread; a short tile edge (BM*2 or BN*2 < kThreads) leaves the upper threads without a unit
  constexpr int A_UNITS = (BM * 2 + kThreads - 1) / kThreads, B_UNITS = (BN * 2 + kThreads - 1) / kThreads;
  constexpr bool A_PARTIAL = (BM * 2) % kThreads != 0, B_PARTIAL = (BN * 2) % kThreads != 0;
  static_assert(!A_PARTIAL || A_UNITS == 1, "a partial A pass is a single pass");
  static_assert(!B_PARTIAL || B_UNITS == 1, "a partial B pass is a single pass");
  constexpr int A_TILE = BM * kRowBytes, B_TILE = BN * kRowBytes;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const lds_a0 = smem;                        // [buf][A | B]
  unsigned char* const lds_b0 = smem + A_TILE;
  unsigned char* const lds_a1 = smem + A_TILE + B_TILE;
  unsigned char* const lds_b1 = smem + 2 * A_TILE + B_TILE;

  // ---- XCD-aware tile order: blocks that land on one XCD (id % 8) get a contiguous range of tiles, and
  //      within it tiles walk M fastest in groups of 8 so concurrently resident blocks share B panels.
  const int ntiles = p.tiles_m * p.tiles_n;
  int bid = blockIdx.x, split = 0;
  if (p.splits > 1) {
    split = bid / ntiles;
    bid -= split * ntiles;
  }
  {
    const int q8 = ntiles >> 3, r8 = ntiles & 7, x = bid & 7, j = bid >> 3;
    bid = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + j;     // bijective for any ntiles
  }
  constexpr int kGroupM = 8;
  const int per_group = kGroupM * p.tiles_n;
  const int grp = bid / per_group;
  const int first_m = grp * kGroupM;
  const int gsz = min(p.tiles_m - first_m, kGroupM);
  const int tm = first_m + (bid % per_group) % gsz;
  const int tn = (bid % per_group) / gsz;
  // (workgroup-uniform; pinned to SGPRs: with the tile origin left to the compiler, hipcc moved the whole tile-order arithmetic to the
  // vector unit in one build of the interior epilogue and kept two more VGPRs through the K loop)
  const int m0 = __builtin_amdgcn_readfirstlane(tm * BM), n0 = __builtin_amdgcn_readfirstlane(tn * BN);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WAVES_N, wc = wave % WAVES_N;
  ARCQ_TILE_STAMP(0);
  const int half_k = p.K >> 1, atoms_k = p.K >> 6;
  const int a_begin = split * p.atoms_per_split, a_end = min(atoms_k, a_begin + p.atoms_per_split);   // never empty

  // ---- staging geometry (loop invariant): per operand two descriptors at the tile origin (workgroup-uniform: kernel arguments and
  //      m0 / n0) and per unit two 32-bit lane offsets against it (gemm_tile_common.hpp).  Rows are clamped into the matrix, so a lane
  //      offset is non-negative and spans at most BM - 1 / BN - 1 rows; the launcher refuses a K whose tile would not fit 32 bits.
  static_assert((128 % BM == 0 || BM % 128 == 0) && (128 % BN == 0 || BN % 128 == 0) && BM % 32 == 0 && BN % 32 == 0,
                "a tile lies inside one 128-row block of the scale layout or starts on one, and on a 32-row boundary: no row's scales precede the origin's");
  // reference layout: the tile's rows [t0, t0 + rows) of codes, and of scale bytes from the tile origin to the end of its last 128-row block
  auto ref_src = [&](const uint8_t* Q, const uint8_t* SF, int t0, int rows) {
    const uint32_t blocks = (uint32_t)(((t0 + rows - 1) >> 7) - (t0 >> 7) + 1), lead = (uint32_t)sf_atom_offset(t0 & 127, 0, atoms_k);
    return StageSrc{stage_rsrc(Q + (size_t)t0 * half_k, (uint32_t)rows * (uint32_t)half_k),
                    stage_rsrc(SF + sf_atom_offset(t0, 0, atoms_k), blocks * (uint32_t)atoms_k * 512u - lead)};
  };
  const StageSrc a_src = ref_src(p.A, p.SFA, m0, min(p.M - m0, BM));
  [[maybe_unused]] const int rw_tiles = ((p.K + 255) >> 8) * 2;      // kBRepacked: tiles of 128 K per block of 16 rows
  const StageSrc b_src = [&] {
    if constexpr (kBLayout == kBRepacked) {         // whole blocks of 16 rows (N is padded to 16 in RW / RSF)
      const uint32_t blocks = (uint32_t)((min(p.N - n0, BN) + 15) >> 4);
      return StageSrc{stage_rsrc(p.B + (size_t)(n0 >> 4) * rw_tiles * 1024, blocks * (uint32_t)rw_tiles * 1024u),
                      stage_rsrc(p.SFB + (size_t)(n0 >> 4) * rw_tiles * 128, blocks * (uint32_t)rw_tiles * 128u)};
    } else {
      return ref_src(p.B, p.SFB, n0, min(p.N - n0, BN));
    }
  }();
  uint32_t a_q[A_UNITS], a_sf[A_UNITS];
  uint32_t a_live[A_UNITS];
  int a_slot[A_UNITS][4];
#pragma unroll
  for (int u = 0; u < A_UNITS; ++u) {
    const int unit = tid + u * kThreads, r = A_PARTIAL ? min(unit >> 1, BM - 1) : unit >> 1, h = unit & 1;
    const int row = m0 + r, rc = row < p.M ? row : p.M - 1;
    a_q[u] = (uint32_t)(rc - m0) * (uint32_t)half_k + h * 16;
    a_sf[u] = (uint32_t)(sf_atom_offset(rc, 0, atoms_k) - sf_atom_offset(m0, 0, atoms_k)) + h * 2;
    a_live[u] = row < p.M ? kSfLive : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) a_slot[u][j] = kMfma32 ? lds_slot32(r, h * 4 + j) : lds_slot(r, h * 4 + j);
  }
  uint32_t b_q[B_UNITS], b_sf[B_UNITS];
  uint32_t b_live[B_UNITS];
  int b_slot[B_UNITS][4];
#pragma unroll
  for (int u = 0; u < B_UNITS; ++u) {
    const int unit = tid + u * kThreads, r = B_PARTIAL ? min(unit >> 1, BN - 1) : unit >> 1, h = unit & 1;
    const int row = n0 + r, rc = row < p.N ? row : p.N - 1;
    if constexpr (kBLayout == kBRepacked) {         // the atom-independent terms of stage_step_rw's layout
      const uint32_t rb = (uint32_t)((rc >> 4) - (n0 >> 4));
      b_q[u] = rb * (uint32_t)rw_tiles * 1024u + h * 256 + (rc & 15) * 16;
      b_sf[u] = rb * (uint32_t)rw_tiles * 128u + h * 64 + (rc & 15) * 4;
    } else {
      b_q[u] = (uint32_t)(rc - n0) * (uint32_t)half_k + h * 16;
      b_sf[u] = (uint32_t)(sf_atom_offset(rc, 0, atoms_k) - sf_atom_offset(n0, 0, atoms_k)) + h * 2;
    }
    b_live[u] = row < p.N ? kSfLive : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) b_slot[u][j] = kMfma32 ? lds_slot32(r, h * 4 + j) : lds_slot(r, h * 4 + j);
  }
  // fragment read offsets: one base per operand; tile i adds i*16 rows (the swizzle term is invariant under
  // +16 rows) and the second half of K flips bit 2 of the slot index, i.e. byte-offset bit 6
  const int fa_base = kMfma32 ? lds_slot32(wr * WM + (lane & 31), lane >> 5) : lds_slot(wr * WM + (lane & 15), lane >> 4);
  const int fb_base = kMfma32 ? lds_slot32(wc * WN + (lane & 31), lane >> 5) : lds_slot(wc * WN + (lane & 15), lane >> 4);
  acc_t acc[TM][TN];
  if constexpr (!kOverlapTail) {                // (kOverlapTail: zeroed behind the prologue's loads, while they are in flight)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < (kMfma32 ? 16 : 4); ++r) acc[i][j][r] = 0.f;
  }

  Staged sa[A_UNITS], sb[B_UNITS];     // registers holding step kt+1 while step kt is multiplied
  auto load_step = [&](int atom) {
    atom = __builtin_amdgcn_readfirstlane(atom);    // (uniform already unless kStagger shifts it by the wave's group: the step offsets are scalar operands)
    const StageStep sa_step = stage_step(atom), sb_step = kBLayout == kBRepacked ? stage_step_rw(atom) : sa_step;
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u) sa[u] = stage_load(a_src, a_q[u], a_sf[u], sa_step);
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u) sb[u] = stage_load(b_src, b_q[u], b_sf[u], sb_step);
  };
#ifdef ARCQ_TILE_BODY_PAIR_LOADS
  // kPairLoads: two atoms requested together.  Per unit the 16 code bytes of atom0 and directly behind them those of atom1 (the same line
  // of the row, or the next one), fenced so that hipcc keeps each pair adjacent and in that order.  kParts selects what one call issues:
  // bit 0 A's code pairs, bit 1 B's, bit 2 the scale loads of both operands -- the prologue issues all of it at once, the even step one
  // part per place (all eight loads of a wave in ONE burst at the top of the step measured SLOWER than the parent: DESIGN.md 3.2).
  // (Declared under this gate alone: an unused third register set and lambda moved instructions in the other kernels.)
  Staged sa2[A_UNITS], sb2[B_UNITS];   // atom kt + 2 across the even step (sa / sb receive atom kt + 3)
  auto load_pair = [&](int atom0, int atom1, Staged (&a0)[A_UNITS], Staged (&b0)[B_UNITS], Staged (&a1)[A_UNITS], Staged (&b1)[B_UNITS], auto parts) {
    constexpr int kParts = decltype(parts)::value;
    atom0 = __builtin_amdgcn_readfirstlane(atom0);
    atom1 = __builtin_amdgcn_readfirstlane(atom1);
    const StageStep a_s0 = stage_step(atom0), a_s1 = stage_step(atom1);
    const StageStep b_s0 = kBLayout == kBRepacked ? stage_step_rw(atom0) : a_s0, b_s1 = kBLayout == kBRepacked ? stage_step_rw(atom1) : a_s1;
    __builtin_amdgcn_sched_barrier(0);            // (the scalar offsets are formed ahead of the first pair, not inside one)
    if constexpr ((kParts & 1) != 0) {
#pragma unroll
      for (int u = 0; u < A_UNITS; ++u) {
        a0[u].q = stage_load_q(a_src, a_q[u], a_s0);
        __builtin_amdgcn_sched_barrier(0);
        a1[u].q = stage_load_q(a_src, a_q[u], a_s1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr ((kParts & 2) != 0) {
#pragma unroll
      for (int u = 0; u < B_UNITS; ++u) {
        b0[u].q = stage_load_q(b_src, b_q[u], b_s0);
        __builtin_amdgcn_sched_barrier(0);
        b1[u].q = stage_load_q(b_src, b_q[u], b_s1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr ((kParts & 4) != 0) {
#pragma unroll
      for (int u = 0; u < A_UNITS; ++u) {
        a0[u].sf = stage_load_sf(a_src, a_sf[u], a_s0);
        a1[u].sf = stage_load_sf(a_src, a_sf[u], a_s1);
      }
#pragma unroll
      for (int u = 0; u < B_UNITS; ++u) {
        b0[u].sf = stage_load_sf(b_src, b_sf[u], b_s0);
        b1[u].sf = stage_load_sf(b_src, b_sf[u], b_s1);
      }
    }
  };
  using kPairA = std::integral_constant<int, 1>;
  using kPairB = std::integral_constant<int, 2>;
  using kPairSf = std::integral_constant<int, 4>;
  using kPairAll = std::integral_constant<int, 7>;
#endif
#ifdef ARCQ_TILE_BODY_QUAD_LOADS
  // kQuadLoads: four atoms of a row requested together.  load_quad_q: per unit the 16 code bytes of atoms atom0 .. atom0 + 3 (each clamped
  // to the range's last atom, so every address lies inside the descriptor), four consecutive loads fenced like load_pair's two;
  // load_quad_sf: the scale bytes of atoms first .. last of that quad, one 2-byte load per atom and unit.  (Declared under this gate
  // alone, like the pair's.)
  static_assert(kBLayout == kBRef, "quads follow the reference layout's rows (repacked launches keep gemm_tile_pl_kernel)");
  Staged qa[4][A_UNITS], qb[4][B_UNITS];   // the quad last requested: A's atoms kt + 2 .. kt + 5 (step 0), B's kt + 4 .. kt + 7 (step 2)
  Staged yb[2][B_UNITS];                   // B's atoms kt + 2 and kt + 3 across the back-edge (sb holds kt + 1)
  bool quad_single = false;                // kStepOneA: whether the step requests A's atom kt + 2 at all (workgroup-uniform)
  auto quad_steps = [&](int atom0, StageStep (&s)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = stage_step(__builtin_amdgcn_readfirstlane(min(atom0 + i, a_end - 1)));
  };
  auto load_quad_q = [&](int atom0, const StageSrc& src, const auto& lane_q, auto& dst) {
    StageStep s[4];
    quad_steps(atom0, s);
    __builtin_amdgcn_sched_barrier(0);            // (the scalar offsets are formed ahead of the first load, not inside the run)
#pragma unroll
    for (int u = 0; u < (int)(sizeof(dst[0]) / sizeof(dst[0][0])); ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dst[i][u].q = stage_load_q(src, lane_q[u], s[i]);
        __builtin_amdgcn_sched_barrier(0);
      }
  };
  auto load_quad_sf = [&](int atom0, const StageSrc& src, const auto& lane_sf, auto& dst, int first, int last) {
    StageStep s[4];
    quad_steps(atom0, s);
#pragma unroll
    for (int u = 0; u < (int)(sizeof(dst[0]) / sizeof(dst[0][0])); ++u)
#pragma unroll
      for (int i = first; i <= last; ++i) dst[i][u].sf = stage_load_sf(src, lane_sf[u], s[i]);
  };
#endif
  auto store_step = [&](unsigned char* la, unsigned char* lb) {
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u)
      if (!A_PARTIAL || tid < BM * 2) stage_store(la, a_slot[u], sa[u], a_live[u]);
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u)
      if (!B_PARTIAL || tid < BN * 2) stage_store(lb, b_slot[u], sb[u], b_live[u]);
  };
  auto mma_step = [&](const unsigned char* la, const unsigned char* lb) {
    // weights (B of the GEMM) are the MFMA A operand, so a lane ends up with runs of 4 consecutive n
    if constexpr (kMfma32) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {          // 16 K elements per 32x32x16 MFMA: slot = 2*ks + (lane >> 5)
        Frag8 fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i].u = *reinterpret_cast<const uint4*>(la + (fa_base ^ (ks * 32)) + i * 32 * kRowBytes);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j].u = *reinterpret_cast<const uint4*>(lb + (fb_base ^ (ks * 32)) + j * 32 * kRowBytes);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[j].v, fa[i].v, acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {          // 32 K elements per 16x16x32 MFMA: slot = 4*ks + (lane >> 4)
        Frag8 fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i].u = *reinterpret_cast<const uint4*>(la + (fa_base ^ (ks * 64)) + i * 16 * kRowBytes);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j].u = *reinterpret_cast<const uint4*>(lb + (fb_base ^ (ks * 64)) + j * 16 * kRowBytes);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j].v, fa[i].v, acc[i][j], 0, 0, 0);
      }
    }
  };
  // One K step, branch-free: multiply the tile in (ca, cb) while the registers of the next step are
  // dequantised into (na, nb) and the loads of the step after that are issued.  The K index is clamped,
  // so the last steps re-stage the final atom into a buffer nobody reads.
  const bool late = kStagger && wave >= 4;       // wave-uniform: this wave stages one step further ahead, after the barrier
  auto k_step = [&](int kt, unsigned char* ca, unsigned char* cb, unsigned char* na, unsigned char* nb) {
    Staged ta[A_UNITS], tb[B_UNITS];
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u) ta[u] = sa[u];
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u) tb[u] = sb[u];
    load_step(min(kt + 2 + (late ? 1 : 0), a_end - 1));   // in flight during this whole step
    __builtin_amdgcn_sched_barrier(0);            // keep the loads at the top: hipcc otherwise sinks them to the barrier
    mma_step(ca, cb);
    if (kStagger && late) __syncthreads();        // every wave has multiplied step kt: its buffer may be overwritten
    unsigned char* const wa = late ? ca : na;
    unsigned char* const wb = late ? cb : nb;
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u)
      if (!A_PARTIAL || tid < BM * 2) stage_store(wa, a_slot[u], ta[u], a_live[u]);
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u)
      if (!B_PARTIAL || tid < BN * 2) stage_store(wb, b_slot[u], tb[u], b_live[u]);
    if (!kStagger || !late) __syncthreads();
  };

  // Hand-pipelined K step (16x16x32 MFMA): the compiler's own schedule waits for every pair of fragment reads right
  // after issuing it (LDS latency exposed every 8 MFMAs) and clusters the dequantisation.  Here a step is cut into
  // TM blocks of [2 fragment reads for the NEXT block | 2 x TN MFMAs of this block | 1/TM of the staging work], fenced
  // with sched_barrier so that hipcc keeps the order; waits become counted lgkmcnt(N) on reads issued a block earlier.
  // Where the 8-fragment step keeps its one barrier: kRot blocks of 8 MFMAs BEFORE the end of the step, so that what follows the release
  // is MFMAs on fragments already in registers.  (The step with the barrier last and the rotations 2 and 3 were the other arms of the A-B
  // and of the sweep recorded in DESIGN.md 3.2; they were compile-time arms of this file up to commit 07fad6c.)
  constexpr int kRot = 1;
  // (the 256 x 256 8-wave tile alone: no partial staging pass, one A and one B unit per thread; the other tiles keep the barrier last)
  constexpr bool kRotate = kPipe && !kMfma32 && TM == 8 && TN == 4 && WAVES_M * WAVES_N == 8 && !A_PARTIAL && !B_PARTIAL;
  auto rd_frag = [&](const unsigned char* tile, int base, int ks, int i) { Frag8 f; f.u = *reinterpret_cast<const uint4*>(tile + (base ^ (ks * 64)) + i * 16 * kRowBytes); return f; };
  [[maybe_unused]] Frag8 head_b[TN], head_a[2];   // kRotate: the fragments a step is entered with, carried across the loop's back-edge
  // what a step requests and which registers it stages from.  kStepOne: atom kt + 2 into sa / sb, staging what they held.  kPairLoads:
  // kStepPair (even) -- atoms kt + 2 into sa2 / sb2 and kt + 3 into sa / sb, staging what sa / sb held; kStepOdd -- no request, staging
  // sa2 / sb2; kStepNone (the step behind the loop, whose successor is the final step and stages nothing) -- no request, staging sa / sb
  using kStepOne = std::integral_constant<int, 0>;
  using kStepPair = std::integral_constant<int, 1>;
  using kStepOdd = std::integral_constant<int, 2>;
  using kStepNone = std::integral_constant<int, 3>;
#ifdef ARCQ_TILE_BODY_QUAD_LOADS
  // kQuadLoads: every step stages what sa / sb hold on entry (the caller names the sets).  kStepQuadA -- A's atoms kt + 2 .. kt + 5 into
  // qa, codes and the first scale pair; kStepQuadB -- the same for B into qb; kStepSfA / kStepSfB (the steps behind those) -- the other
  // three scale pairs of that quad; kStepOneA (behind the loop) -- A's atom kt + 2 alone into qa[0], if quad_single
  using kStepQuadA = std::integral_constant<int, 4>;
  using kStepQuadB = std::integral_constant<int, 5>;
  using kStepOneA = std::integral_constant<int, 6>;
  using kStepSfA = std::integral_constant<int, 7>;
  using kStepSfB = std::integral_constant<int, 8>;
#endif
  auto k_step_pipe = [&](int kt, unsigned char* ca, unsigned char* cb, unsigned char* na, unsigned char* nb, auto step_kind) {
    static_assert(kMfma32 || TM % 2 == 0, "pairs of A fragments");
    constexpr int kKind = decltype(step_kind)::value;
    static_assert(kKind == 0 || kPairLoads, "the paired-load sibling's steps");
    Staged ta[A_UNITS], tb[B_UNITS];
#pragma unroll
    for (int u = 0; u < A_UNITS; ++u) ta[u] = sa[u];
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u) tb[u] = sb[u];
    if constexpr (kKind == kStepOne::value) load_step(min(kt + 2, a_end - 1));            // in flight during this whole step
#ifdef ARCQ_TILE_BODY_PAIR_LOADS
    if constexpr (kKind == kStepOdd::value) {
#pragma unroll
      for (int u = 0; u < A_UNITS; ++u) ta[u] = sa2[u];
#pragma unroll
      for (int u = 0; u < B_UNITS; ++u) tb[u] = sb2[u];
    }
    if constexpr (kKind == kStepPair::value) load_pair(min(kt + 2, a_end - 1), min(kt + 3, a_end - 1), sa2, sb2, sa, sb, kPairA{});   // ... and the next: A's code pairs here
#endif
#ifdef ARCQ_TILE_BODY_QUAD_LOADS
    if constexpr (kKind == kStepQuadA::value) load_quad_q(kt + 2, a_src, a_q, qa);          // A's quad here, its first scale load ahead of block 2
    if constexpr (kKind == kStepSfA::value) load_quad_sf(kt + 1, a_src, a_sf, qa, 1, 3);
    if constexpr (kKind == kStepSfB::value) load_quad_sf(kt + 1, b_src, b_sf, qb, 1, 3);
    if constexpr (kKind == kStepOneA::value) {
      if (quad_single) {                          // (kt + 2 < a_end: a step stages it)
        const StageStep one = stage_step(__builtin_amdgcn_readfirstlane(kt + 2));
#pragma unroll
        for (int u = 0; u < A_UNITS; ++u) qa[0][u] = stage_load(a_src, a_q[u], a_sf[u], one);
      }
    }
#endif
    __builtin_amdgcn_sched_barrier(0);
    constexpr int kPieces = (A_UNITS + B_UNITS) * 4, kBlocks = kMfma32 ? 4 : TM;   // 32x32x16: one block per 16-wide K slice
    auto pieces = [&](int blk) {                  // this block's share of the staging of step kt + 1
#pragma unroll
      for (int c = blk; c < kPieces; c += kBlocks) {
        const int u = c >> 2, j = c & 3;
        if (u < A_UNITS) {
          if (!A_PARTIAL || tid < BM * 2) stage_piece(na, a_slot[u < A_UNITS ? u : 0][j], ta[u < A_UNITS ? u : 0], a_live[u < A_UNITS ? u : 0], j);
        } else {
          const int v = u - A_UNITS < B_UNITS ? u - A_UNITS : 0;
          if (!B_PARTIAL || tid < BN * 2) stage_piece(nb, b_slot[v][j], tb[v], b_live[v], j);
        }
      }
    };
    if constexpr (kMfma32) {
      // 32x32x16 MFMAs last 32 cycles: ~3 VALU instructions fit into each one's shadow.  Blocks = the four 16-wide K
      // slices; all TM + TN fragments of slice ks + 1 are requested before the TM x TN MFMAs of slice ks.
      Frag8 f32a[2][TM], f32b[2][TN];
      auto rd_set = [&](int buf, int ks) {
#pragma unroll
        for (int i = 0; i < TM; ++i) f32a[buf][i].u = *reinterpret_cast<const uint4*>(ca + (fa_base ^ (ks * 32)) + i * 32 * kRowBytes);
#pragma unroll
        for (int j = 0; j < TN; ++j) f32b[buf][j].u = *reinterpret_cast<const uint4*>(cb + (fb_base ^ (ks * 32)) + j * 32 * kRowBytes);
      };
      rd_set(0, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks + 1 < 4) rd_set((ks + 1) & 1, ks + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            if constexpr (kMfma32)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f32b[ks & 1][j].v, f32a[ks & 1][i].v, acc[i][j], 0, 0, 0);
        pieces(ks);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      return;
    }
    auto rd_a = [&](int ks, int i) { return rd_frag(ca, fa_base, ks, i); };
    auto rd_b = [&](int ks, int j) { return rd_frag(cb, fb_base, ks, j); };
    if constexpr (kRotate) {
      // ROTATED step: the barrier sits kRot blocks before the end.  The step is entered with B's fragments of K half 0 and the first A pair
      // in registers (head_b / head_a, read from this buffer behind the previous step's barrier).  Blocks 0 .. kLast multiply, stage ALL of
      // step kt + 1 into (na, nb) and issue every remaining fragment read of (ca, cb); then lgkmcnt(0) + barrier: this wave has finished its
      // reads of (ca, cb) and its writes of (na, nb).  Blocks kLast + 1 .. multiply fragments already held -- MFMAs are what follows the
      // release -- and between them read step kt + 1's first fragments from (na, nb).  Same MFMAs, same order, same accumulators.
      // Hazards by the barrier alone: (na, nb) is read only behind a barrier every writer reached with lgkmcnt(0); (ca, cb) is overwritten
      // (next step, blocks 0 ..) only behind a barrier every reader reached with its reads retired.
      constexpr int kQ = 2 * (TM / 2), kHalf = TM / 2, kLast = kQ - 1 - kRot, kNPre = kLast + 1;
      static_assert(kRot >= 1 && kLast >= kHalf, "the second K half's B fragments are read ahead of the barrier, a block before their use");
      // A pairs requested by the end of block b's read phase: one ahead, two per block over the last blocks so that pairs kLast + 2 .. are in
      auto read_by = [](int b) { const int extra = b - (kLast - kRot), h = b + 1 + (extra > 0 ? extra : 0); return h < kQ - 1 ? h : kQ - 1; };
      Frag8 fb1[TN], fq[kQ][2];
      fq[0][0] = head_a[0];
      fq[0][1] = head_a[1];
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int ks = q / kHalf, pr = q % kHalf;
        constexpr int kHeadReads = TN + 2;
        int n_pieces = 0, n_reads = 0;
#ifdef ARCQ_TILE_BODY_PAIR_LOADS
        if constexpr (kKind == kStepPair::value) {          // ... B's code pairs ahead of block 2, the scale loads of both ahead of block 4
          if (q == 2) load_pair(min(kt + 2, a_end - 1), min(kt + 3, a_end - 1), sa2, sb2, sa, sb, kPairB{});
          if (q == 4) load_pair(min(kt + 2, a_end - 1), min(kt + 3, a_end - 1), sa2, sb2, sa, sb, kPairSf{});
          if (q == 2 || q == 4) __builtin_amdgcn_sched_barrier(0);
        }
#endif
#ifdef ARCQ_TILE_BODY_QUAD_LOADS
        if constexpr (kKind == kStepQuadA::value) {         // ... the first scale load of A's quad ahead of block 2
          if (q == 2) {
            load_quad_sf(kt + 2, a_src, a_sf, qa, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        if constexpr (kKind == kStepQuadB::value) {         // B's quad ahead of block 2, its first scale load ahead of block 4
          if (q == 2) load_quad_q(kt + 2, b_src, b_q, qb);
          if (q == 4) load_quad_sf(kt + 2, b_src, b_sf, qb, 0, 0);
          if (q == 2 || q == 4) __builtin_amdgcn_sched_barrier(0);
        }
#endif
        if (q <= kLast) {
          // (1) reads for later blocks
#pragma unroll
          for (int r = (q ? read_by(q - 1) : 0) + 1; r <= read_by(q); ++r) {
            fq[r][0] = rd_a(r / kHalf, 2 * (r % kHalf));
            fq[r][1] = rd_a(r / kHalf, 2 * (r % kHalf) + 1);
          }
          if (q == kHalf - 1) {
#pragma unroll
            for (int j = 0; j < TN; ++j) fb1[j] = rd_b(1, j);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // (2) this block's MFMAs; weights are the MFMA A operand
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[2 * pr + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16((ks ? fb1[j] : head_b[j]).v, fq[q][ii].v, acc[2 * pr + ii][j], 0, 0, 0);
        if (q <= kLast) {
          // (3) its share of the staging of step kt + 1: all kPieces over the blocks ahead of the barrier
#pragma unroll
          for (int c = 0; c < kPieces; ++c)
            if (c * kNPre / kPieces == q) {
              const int u = c >> 2, j = c & 3;
              // (a unit's first piece pins its scale bytes to this block: left free, hipcc lifts the shifts that form the scale pair of
              // BOTH units to the top of the step, four vector instructions and the wait for the scale loads ahead of the first MFMA)
              if (u < A_UNITS) {
                if (j == 0) asm volatile("" : "+v"(ta[u].sf));
                stage_piece(na, a_slot[u][j], ta[u], a_live[u], j);
              } else {
                if (j == 0) asm volatile("" : "+v"(tb[u - A_UNITS].sf));
                stage_piece(nb, b_slot[u - A_UNITS][j], tb[u - A_UNITS], b_live[u - A_UNITS], j);
              }
              ++n_pieces;
            }
        } else {
          // (3') step kt + 1's first fragments, from the buffer the barrier has just published (the last step of a range reads bytes that
          // were staged from the clamped atom and are never multiplied): B's K half 0, then the first A pair
          const int i0 = q - kLast - 1;
#pragma unroll
          for (int n = i0 * kHeadReads / kRot; n < (i0 + 1) * kHeadReads / kRot; ++n) {
            if (n < TN) head_b[n] = rd_frag(nb, fb_base, 0, n);
            else head_a[n - TN] = rd_frag(na, fa_base, 0, n - TN);
            ++n_reads;
          }
        }
        // spacing: ahead of the barrier two vector instructions per staged piece in the shadow of every MFMA, behind it one fragment read
#pragma unroll
        for (int m8 = 0; m8 < 2 * TN; ++m8) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (q <= kLast) {
            if (n_pieces == 1) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);          // (the builtin takes literal counts)
            else if (n_pieces == 2) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            else if (n_pieces >= 3) __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
          } else if (m8 < n_reads) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (q == kLast) {
          __syncthreads();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      return;
    }
    // fragment queue: A fragments are requested kAhead pairs before their MFMAs, the B set of the second K half during the
    // last pairs of the first
    constexpr int kPairs = TM / 2, kSeq = 2 * kPairs, kAhead = 1;   // 2 measured the same (1188-1202 vs 1193-1200) with 8 more registers
    Frag8 fb[2][TN], fq[kSeq][2];
    auto rd_pair = [&](int q) {                   // q = ks * kPairs + pr (compile-time after unrolling)
      fq[q][0] = rd_a(q / kPairs, 2 * (q % kPairs));
      fq[q][1] = rd_a(q / kPairs, 2 * (q % kPairs) + 1);
    };
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[0][j] = rd_b(0, j);
#pragma unroll
    for (int q = 0; q < kAhead; ++q) rd_pair(q);
#pragma unroll
    for (int q = 0; q < kSeq; ++q) {
      const int ks = q / kPairs, pr = q % kPairs;
      // (1) reads for later blocks
      if (q + kAhead < kSeq) rd_pair(q + kAhead);
      if (ks == 0 && pr == kPairs - 1 - (kAhead - 1 < kPairs - 1 ? kAhead - 1 : kPairs - 1)) {
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[1][j] = rd_b(1, j);
      }
      __builtin_amdgcn_sched_barrier(0);
      // (2) this block's MFMAs; weights are the MFMA A operand
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          if constexpr (!kMfma32)
            acc[2 * pr + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[ks][j].v, fq[q][ii].v, acc[2 * pr + ii][j], 0, 0, 0);
      pieces(q);                                  // (3) its share of the staging of step kt + 1
      // spacing inside the block: two vector instructions in the shadow of every MFMA (measured on 4096^2, TFLOP/s:
      // compiler's own placement 1211-1219, 1 MFMA + 1 VALU 1195-1201, 1+2 1234-1236, 1+3 1217-1220, 2+4 1227, 4+5 1180)
      // The smaller tiles measure the same or slightly worse with it (M=1024: 612 vs 624), so only the 8-fragment tile.
#pragma unroll
      for (int m8 = 0; m8 < (TM == 8 ? 2 * TN : 0); ++m8) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  };

  // ---- prologue: tile 0 into buffer 0, registers <- step 1.  Both steps are requested together and only step 0 is awaited (a
  //      counted vmcnt: loads return in order): one memory round trip before the first MFMA, not two dependent ones.  The second
  //      register set exists only here.
#ifdef ARCQ_TILE_BODY_PAIR_LOADS                // (the same two steps, ordered as the even step orders its own)
  Staged sa0[A_UNITS], sb0[B_UNITS];
  load_pair(a_begin, min(a_begin + 1, a_end - 1), sa0, sb0, sa, sb, kPairAll{});
#ifdef ARCQ_TILE_BODY_QUAD_LOADS                // ... and behind them B's atoms 2 and 3, which the loop's first two steps do not request
  {
    const StageStep b_s2 = stage_step(__builtin_amdgcn_readfirstlane(min(a_begin + 2, a_end - 1)));
    const StageStep b_s3 = stage_step(__builtin_amdgcn_readfirstlane(min(a_begin + 3, a_end - 1)));
#pragma unroll
    for (int u = 0; u < B_UNITS; ++u) {
      yb[0][u] = stage_load(b_src, b_q[u], b_sf[u], b_s2);
      yb[1][u] = stage_load(b_src, b_q[u], b_sf[u], b_s3);
    }
  }
#endif
#else
  load_step(a_begin);
  Staged sa0[A_UNITS], sb0[B_UNITS];
#pragma unroll
  for (int u = 0; u < A_UNITS; ++u) sa0[u] = sa[u];
#pragma unroll
  for (int u = 0; u < B_UNITS; ++u) sb0[u] = sb[u];
  load_step(min(a_begin + 1, a_end - 1));
#endif
  __builtin_amdgcn_sched_barrier(0);            // keep the second set of loads above the first wait
  if constexpr (kOverlapTail) {                 // the accumulators are zeroed while the first loads are in flight, not between their arrival and the first MFMA
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = acc_t{};
        asm volatile("" : "+v"(acc[i][j]));     // (written here: left free, the zeros are materialised in front of the loop)
      }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int u = 0; u < A_UNITS; ++u)
    if (!A_PARTIAL || tid < BM * 2) stage_store(lds_a0, a_slot[u], sa0[u], a_live[u]);
#pragma unroll
  for (int u = 0; u < B_UNITS; ++u)
    if (!B_PARTIAL || tid < BN * 2) stage_store(lds_b0, b_slot[u], sb0[u], b_live[u]);
  if (kStagger && late) {                       // the late group enters the loop with step 1 staged and step 2 in registers
    store_step(lds_a1, lds_b1);
    load_step(min(a_begin + 2, a_end - 1));
  }
  __syncthreads();
  if constexpr (kRotate) {                      // the first step's head fragments
#pragma unroll
    for (int j = 0; j < TN; ++j) head_b[j] = rd_frag(lds_b0, fb_base, 0, j);
    head_a[0] = rd_frag(lds_a0, fa_base, 0, 0);
    head_a[1] = rd_frag(lds_a0, fa_base, 0, 1);
  }
  int kt = a_begin;
  // alpha_dev is workgroup-uniform: a scalar load ahead of the loop, held in one SGPR across it (no tile's epilogue starts with a
  // vector-memory round trip); the product with alpha_host is formed after the loop, so that no VGPR is live through it
  float alpha_dev = 1.0f;
  if (p.alpha_dev) alpha_dev = *reinterpret_cast<const __attribute__((address_space(4))) float*>(reinterpret_cast<uintptr_t>(p.alpha_dev));
  asm volatile("" : "+s"(alpha_dev));
  // the second-dispatched half of an 8-wave workgroup loses every issue arbitration against its SIMD partner at equal
  // priority; a static priority for it (never flipped) measured +0.8 % (1192-1203 -> 1209-1212 TFLOP/s)
  if (WAVES_M * WAVES_N == 8 && wave >= 4) __builtin_amdgcn_s_setprio(1);
  ARCQ_TILE_STAMP(1);
  [[maybe_unused]] int tail_buf = 0;            // kOverlapTail: byte offset of the LDS buffer that holds the range's last step
  if constexpr (kOverlapTail) {
    // the unchanged step pairs while at least three steps remain, one more unchanged step if two remain; the range's last step is
    // multiplied by the final step (inside the interior epilogue below) from whichever buffer it was staged into
    static_assert(kRotate, "the final step is entered with head fragments");
    using Even = std::conditional_t<kPairLoads, kStepPair, kStepOne>;
    using Odd = std::conditional_t<kPairLoads, kStepOdd, kStepOne>;
    using Last = std::conditional_t<kPairLoads, kStepNone, kStepOne>;
#ifdef ARCQ_TILE_BODY_QUAD_LOADS
    if constexpr (kQuadLoads) {
      auto stage_from = [&](const Staged (&a)[A_UNITS], const Staged (&b)[B_UNITS]) {     // names the sets the next step stages
#pragma unroll
        for (int u = 0; u < A_UNITS; ++u) sa[u] = a[u];
#pragma unroll
        for (int u = 0; u < B_UNITS; ++u) sb[u] = b[u];
      };
      // four steps per iteration while all four stage an atom of the range: entered with A's atom kt + 1 in sa and B's kt + 1 .. kt + 3 in
      // sb, yb[0], yb[1], left the same way
      for (; kt + 4 < a_end; kt += 4) {
        k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, kStepQuadA{});
        stage_from(qa[0], yb[0]);
        k_step_pipe(kt + 1, lds_a1, lds_b1, lds_a0, lds_b0, kStepSfA{});
        stage_from(qa[1], yb[1]);
        k_step_pipe(kt + 2, lds_a0, lds_b0, lds_a1, lds_b1, kStepQuadB{});
        stage_from(qa[2], qb[0]);
        k_step_pipe(kt + 3, lds_a1, lds_b1, lds_a0, lds_b0, kStepSfB{});
        stage_from(qa[3], qb[1]);
#pragma unroll
        for (int u = 0; u < B_UNITS; ++u) {
          yb[0][u] = qb[2][u];
          yb[1][u] = qb[3][u];
        }
      }
      // the 0 - 3 steps left ahead of the final step: B's atoms are held, A's next one is requested alone by the step before its own
      const int left = a_end - 1 - kt;
      if (left >= 1) {
        quad_single = left >= 2;
        k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, kStepOneA{});
        if (left >= 2) {
          stage_from(qa[0], yb[0]);
          quad_single = left >= 3;
          k_step_pipe(kt + 1, lds_a1, lds_b1, lds_a0, lds_b0, kStepOneA{});
          if (left >= 3) {
            stage_from(qa[0], yb[1]);
            k_step_pipe(kt + 2, lds_a0, lds_b0, lds_a1, lds_b1, kStepNone{});
          }
        }
        if (left & 1) tail_buf = A_TILE + B_TILE;
      }
    } else
#endif
    {
      for (; kt + 2 < a_end; kt += 2) {
        k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, Even{});
        k_step_pipe(kt + 1, lds_a1, lds_b1, lds_a0, lds_b0, Odd{});
      }
      if (kt + 1 < a_end) {
        k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, Last{});
        tail_buf = A_TILE + B_TILE;
      }
    }
  } else if constexpr (kPipe) {
    for (; kt + 1 < a_end; kt += 2) {
      k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, kStepOne{});
      k_step_pipe(kt + 1, lds_a1, lds_b1, lds_a0, lds_b0, kStepOne{});
    }
    if (kt < a_end) k_step_pipe(kt, lds_a0, lds_b0, lds_a1, lds_b1, kStepOne{});
  } else {
    for (; kt + 1 < a_end; kt += 2) {
      k_step(kt, lds_a0, lds_b0, lds_a1, lds_b1);
      k_step(kt + 1, lds_a1, lds_b1, lds_a0, lds_b0);
    }
    if (kt < a_end) k_step(kt, lds_a0, lds_b0, lds_a1, lds_b1);
  }
  if constexpr (!kOverlapTail) ARCQ_TILE_STAMP(2);      // (kOverlapTail: behind the final step's last MFMA)

  // ---- epilogue.  16x16 tiles: lane holds D[m = +(lane & 15)][n = +4*(lane >> 4) + r], r = 0..3.
  //      32x32 tiles: lane holds D[m = +(lane & 31)][n = +8*g + 4*(lane >> 5) + r], g = 0..3, r = 0..3.
  const float alpha = p.alpha_host * alpha_dev;
  const bool vec_ok = (p.N & 3) == 0;
  uint32_t act_max = 0;                       // kEpiSiluMul: max |act| of this thread, as bf16 magnitude bits
  // INTERIOR tiles (every row and column inside the matrix, bf16 output, N % 4 == 0, no split-K, 8-byte-aligned operands): one
  // workgroup-uniform test selects a straight-line epilogue -- no bounds, dtype or operand test per quad, bf16 rounding through
  // v_cvt_pk_bf16_f32, one 32-bit row offset per row tile against a uniform tile base (the TN column tiles are immediate offsets).
  // Bias / residual presence are compile-time parameters of it.  The SAME operations in the same order as store4: identical bits.
  [[maybe_unused]] auto interior_epilogue = [&](auto has_bias, auto has_res) __attribute__((always_inline)) {
    constexpr bool kBias = decltype(has_bias)::value, kRes = decltype(has_res)::value;
    constexpr bool kSilu = kEpi == kEpiSiluMul;                     // D is [M, N / 2]: one dword per quad
    constexpr uint32_t kElem = kSilu ? 1 : 2;                       // output bytes per GEMM column
    unsigned char* const tile_d = reinterpret_cast<unsigned char*>(p.D) + ((size_t)m0 * p.N + n0) * kElem;
    const unsigned char* const tile_r = kRes ? reinterpret_cast<const unsigned char*>(p.residual) + ((size_t)m0 * p.N + n0) * 2 : nullptr;
    // the lane's place in the tile, from a thread id the compiler cannot tie to the values it keeps through the K loop: nothing of
    // this path is computed before the loop or carried across it (the loop's register allocation stays the one it was tuned with)
    uint32_t t = tid;
    asm volatile("" : "+v"(t));
    const uint32_t lane_row = (t >> 6) / WAVES_N * WM + (t & 15), lane_col = (t >> 6) % WAVES_N * WN + 4 * ((t >> 4) & 3);
    uint32_t off = lane_row * (uint32_t)p.N + lane_col;             // in elements of the GEMM's [M, N]; < 2^31 (checked by the caller)
    const uint32_t row_step = 16u * (uint32_t)p.N;
    // 16-byte stores (two column tiles traded through v_permlane16_swap) instead of 8-byte ones: half the store instructions, 64
    // contiguous bytes per output row and instruction instead of 32 (the A-B against the 8-byte arm, a compile-time arm of this file up
    // to commit 07fad6c: DESIGN.md 3.2).  off_w: first column of the 8 a lane stores per pair of column tiles (SiLU * up stores one dword
    // per quad and keeps 8-byte addressing)
    constexpr bool kWide = !kSilu && TN % 2 == 0;
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));       // (rows are 8-byte aligned: N % 4 == 0)
    [[maybe_unused]] const uint32_t g4 = (t >> 4) & 3;
    [[maybe_unused]] uint32_t off_w = off - 4 * g4 + ((g4 & 1) ? 16 + 4 * (g4 - 1) : 4 * g4);
    [[maybe_unused]] uint2 held = make_uint2(0, 0);
    // (kOverlapTail with both operands: the bias quads stay packed and are unpacked per use -- 8 registers fewer beside the fragments)
    constexpr bool kPackedBias = kOverlapTail && kBias && kRes;
    float bias_f[TN][4];
    [[maybe_unused]] uint2 bias_v[TN];
    if constexpr (kBias) {
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const uint2 b = *reinterpret_cast<const uint2*>(p.bias + n0 + lane_col + j * 16);
        if constexpr (kPackedBias) {
          bias_v[j] = b;
        } else {
          bias_f[j][0] = bf16_bits_to_f32(b.x & 0xffffu); bias_f[j][1] = bf16_bits_to_f32(b.x >> 16);
          bias_f[j][2] = bf16_bits_to_f32(b.y & 0xffffu); bias_f[j][3] = bf16_bits_to_f32(b.y >> 16);
        }
      }
    }
    uint2 res_cur[TN], res_nxt[TN];
    auto res_load = [&](uint32_t o, uint2 (&r)[TN]) {
#pragma unroll
      for (int j = 0; j < TN; ++j) r[j] = *reinterpret_cast<const uint2*>(tile_r + (size_t)o * 2 + j * 32);
    };
    if constexpr (kRes) res_load(off, res_cur);
    // row tile i is finished and stored as: the residual quads of row tile i + 1 requested, its TN quads, the row offsets advanced
    auto row_quad = [&](int i, int j) __attribute__((always_inline)) {
      {
        if constexpr (kPackedBias) {
          uint2 b = bias_v[j];
          asm volatile("" : "+v"(b.x), "+v"(b.y));
          bias_f[j][0] = bf16_bits_to_f32(b.x & 0xffffu); bias_f[j][1] = bf16_bits_to_f32(b.x >> 16);
          bias_f[j][2] = bf16_bits_to_f32(b.y & 0xffffu); bias_f[j][3] = bf16_bits_to_f32(b.y >> 16);
        }
        float d[4] = {alpha * acc[i][j][0], alpha * acc[i][j][1], alpha * acc[i][j][2], alpha * acc[i][j][3]};
        if constexpr (kSilu) {
          if constexpr (kBias) {
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              round2_to_bf16(d[r], d[r + 1]);
              d[r] += bias_f[j][r];
              d[r + 1] += bias_f[j][r + 1];
            }
          }
          const uint32_t y01 = pack_bf16x2_hw(d[0], d[1]), y23 = pack_bf16x2_hw(d[2], d[3]);
          const uint32_t a0 = silu_mul_bf16(y01 & 0xffffu, y01 >> 16), a1 = silu_mul_bf16(y23 & 0xffffu, y23 >> 16);
          *reinterpret_cast<uint32_t*>(tile_d + (size_t)off + j * 16) = a0 | (a1 << 16);
          act_max = max(act_max, max(a0 & 0x7fffu, a1 & 0x7fffu));
        } else {
          if constexpr (kBias) {
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              round2_to_bf16(d[r], d[r + 1]);
              d[r] += bias_f[j][r];
              d[r + 1] += bias_f[j][r + 1];
            }
          }
          if constexpr (kRes) {
            const uint32_t rw[2] = {res_cur[j].x, res_cur[j].y};
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              round2_to_bf16(d[r], d[r + 1]);
              d[r] += bf16_bits_to_f32(rw[r >> 1] & 0xffffu);
              d[r + 1] += bf16_bits_to_f32(rw[r >> 1] >> 16);
            }
          }
          const uint2 pk = make_uint2(pack_bf16x2_hw(d[0], d[1]), pack_bf16x2_hw(d[2], d[3]));
          if constexpr (kWide) {
            // column tiles j - 1 (held) and j: v_permlane16_swap trades the odd 16-lane rows of the first with the even rows of the
            // second, after which a lane owns 8 CONSECUTIVE columns -- of tile j - 1 in the even rows, of tile j in the odd ones
            if (j & 1) {
              const auto lo = __builtin_amdgcn_permlane16_swap(held.x, pk.x, false, false);
              const auto hi = __builtin_amdgcn_permlane16_swap(held.y, pk.y, false, false);
              const u32x4_a8 v = {lo[0], hi[0], lo[1], hi[1]};
              *reinterpret_cast<u32x4_a8*>(tile_d + (size_t)off_w * 2 + (j >> 1) * 64) = v;
            } else {
              held = pk;
            }
          } else {
            *reinterpret_cast<uint2*>(tile_d + (size_t)off * 2 + j * 32) = pk;
          }
        }
        if (i == 0 && j == 0) ARCQ_TILE_STAMP(3);
      }
    };
    if constexpr (!kOverlapTail) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if constexpr (kRes) { if (i + 1 < TM) res_load(off + row_step, res_nxt); }
#pragma unroll
        for (int j = 0; j < TN; ++j) row_quad(i, j);
        if constexpr (kRes) {
#pragma unroll
          for (int j = 0; j < TN; ++j) res_cur[j] = res_nxt[j];
        }
        off += row_step;
        off_w += row_step;
      }
    } else {
      auto row_open = [&](int i) __attribute__((always_inline)) {
        if constexpr (kRes) { if (i + 1 < TM) res_load(off + row_step, res_nxt); }
      };
      auto row_close = [&]() __attribute__((always_inline)) {
        if constexpr (kRes) {
#pragma unroll
          for (int j = 0; j < TN; ++j) res_cur[j] = res_nxt[j];
        }
        off += row_step;
        off_w += row_step;
      };
      // FINAL step: multiplies the range's last K step from the buffer it was staged into (tail_buf) and stages nothing -- no load, no
      // LDS write, no barrier (nobody writes LDS any more) and no head reads.  Entered like any rotated step, with B's K half 0 and the
      // first A pair in registers.  Pair-outer: block b = K half (b & 1) of row tiles 2 (b >> 1), 2 (b >> 1) + 1, so a pair of row tiles is
      // final after its second block, and row tile b - 2 is finished and stored in the shadow of block b's MFMAs: one quad behind every
      // two MFMAs, fenced, so that no more than a quad's values are live beside the fragments.  Each accumulator still takes K half 0
      // before K half 1.  Fragment reads: B's K half 1 first, then A one block ahead (counted lgkmcnt waits).
      // SiLU * up keeps its epilogue behind the final step: under the MFMAs its exp / divide work measured SLOWER than the kept kernel
      // (DESIGN.md 3.2), so its sibling has the unstaged final step and the early zeroing alone.
      constexpr int kQ = TM;
      constexpr bool kUnder = !kSilu;
      constexpr int kValu = 3 + (kBias ? 5 : 0) + (kRes ? 7 : 0);     // half a quad's vector instructions: between its two MFMAs
      const unsigned char* const fla = lds_a0 + tail_buf;
      const unsigned char* const flb = lds_b0 + tail_buf;
      Frag8 fb1[TN], fq[kQ][2];
      fq[0][0] = head_a[0];
      fq[0][1] = head_a[1];
#pragma unroll
      for (int j = 0; j < TN; ++j) fb1[j] = rd_frag(flb, fb_base, 1, j);
#pragma unroll
      for (int b = 0; b < kQ; ++b) {
        if (b + 1 < kQ) {
          fq[b + 1][0] = rd_frag(fla, fa_base, (b + 1) & 1, 2 * ((b + 1) >> 1));
          fq[b + 1][1] = rd_frag(fla, fa_base, (b + 1) & 1, 2 * ((b + 1) >> 1) + 1);
        }
        if (kUnder && b >= 2) row_open(b - 2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < TN; ++s) {
#pragma unroll
          for (int m8 = 2 * s; m8 < 2 * s + 2; ++m8)          // (the block's MFMAs in the order of every step: row tile outer, column tile inner)
            if constexpr (!kMfma32)
              acc[2 * (b >> 1) + m8 / TN][m8 % TN] = __builtin_amdgcn_mfma_f32_16x16x32_f16(((b & 1) ? fb1[m8 % TN] : head_b[m8 % TN]).v, fq[b][m8 / TN].v,
                                                                                             acc[2 * (b >> 1) + m8 / TN][m8 % TN], 0, 0, 0);
          if (kUnder && b >= 2) {
            row_quad(b - 2, s);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, kValu, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (kUnder && b >= 2) row_close();
      }
      ARCQ_TILE_STAMP(2);
#pragma unroll
      for (int i = kUnder ? TM - 2 : 0; i < TM; ++i) {
        row_open(i);
#pragma unroll
        for (int j = 0; j < TN; ++j) row_quad(i, j);
        row_close();
      }
    }
  };
  // `pre`: the four bias / residual values of (m, n .. n + 3) already fetched with ONE 8-byte load each (N % 4 == 0), two bf16 per dword;
  // otherwise they are read element by element (ragged N).  Same operations in the same order either way.
  auto store4 = [&](int m, int n, float d0, float d1, float d2, float d3, bool pre, uint2 bias2, uint2 res2) __attribute__((always_inline)) {
    if (m >= p.M || n >= p.N) return;
    const uint32_t bw[2] = {bias2.x, bias2.y}, rw[2] = {res2.x, res2.y};
    auto bias_at = [&](int r) { return bf16_bits_to_f32(pre ? (bw[r >> 1] >> (16 * (r & 1))) & 0xffffu : (uint32_t)p.bias[n + r]); };
    if (kEpi == kEpiSiluMul) {                // columns n..n+3 = (gate_j, up_j, gate_j+1, up_j+1), j = n / 2; N % 4 == 0
      uint32_t y[4] = {f32_to_bf16_bits(alpha * d0), f32_to_bf16_bits(alpha * d1), f32_to_bf16_bits(alpha * d2), f32_to_bf16_bits(alpha * d3)};
      if (p.bias) {                             // `y = matmul(...); y = y + bias` of the separate GEMM, in bf16 (qLinearLayer.py:74-76)
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = f32_to_bf16_bits(bf16_bits_to_f32(y[e]) + bias_at(e));
      }
      const uint32_t a0 = silu_mul_bf16(y[0], y[1]);
      const uint32_t a1 = silu_mul_bf16(y[2], y[3]);
      *reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(p.D) + (size_t)m * (p.N >> 1) + (n >> 1)) = a0 | (a1 << 16);
      act_max = max(act_max, max(a0 & 0x7fffu, a1 & 0x7fffu));
      return;
    }
    if (p.splits > 1) {                       // raw partial sums; the launcher only splits when N % 4 == 0
      *reinterpret_cast<float4*>(p.partial + ((size_t)split * p.M + m) * p.N + n) = make_float4(d0, d1, d2, d3);
      return;
    }
    float d[4] = {alpha * d0, alpha * d1, alpha * d2, alpha * d3};
    if (p.bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (pre || n + r < p.N) d[r] = (p.out_dtype == ARCQ_OUT_F32 ? d[r] : bf16_bits_to_f32(f32_to_bf16_bits(d[r]))) + bias_at(r);
    }
    if (p.residual) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (pre || n + r < p.N) {
          const float res = bf16_bits_to_f32(pre ? (rw[r >> 1] >> (16 * (r & 1))) & 0xffffu : (uint32_t)p.residual[(size_t)m * p.N + n + r]);
          d[r] = (p.out_dtype == ARCQ_OUT_F32 ? d[r] : bf16_bits_to_f32(f32_to_bf16_bits(d[r]))) + res;
        }
    }
    if (p.out_dtype == ARCQ_OUT_F32) {
      float* o = reinterpret_cast<float*>(p.D) + (size_t)m * p.N + n;
      if (vec_ok) *reinterpret_cast<float4*>(o) = make_float4(d[0], d[1], d[2], d[3]);
      else for (int r = 0; r < 4; ++r) if (n + r < p.N) o[r] = d[r];
    } else {
      uint16_t* o = reinterpret_cast<uint16_t*>(p.D) + (size_t)m * p.N + n;
      if (vec_ok) *reinterpret_cast<uint2*>(o) = make_uint2(pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3]));
      else for (int r = 0; r < 4; ++r) if (n + r < p.N) o[r] = (uint16_t)f32_to_bf16_bits(d[r]);
    }
  };
  constexpr bool kInteriorPath = !kMfma32;
  static_assert(!kOverlapTail || kInteriorPath, "the final step carries the interior epilogue");
  bool interior = false;                      // (kOverlapTail: the launcher sends launches of interior tiles only; no other epilogue is compiled in)
  if constexpr (kInteriorPath && !kOverlapTail)
    interior = m0 + BM <= p.M && n0 + BN <= p.N && vec_ok && p.splits <= 1 && p.out_dtype == ARCQ_OUT_BF16 && (int64_t)BM * p.N < (1ll << 31) &&
               ((reinterpret_cast<uintptr_t>(p.bias) | reinterpret_cast<uintptr_t>(p.residual)) & 7) == 0;
  if constexpr (kOverlapTail) {
    interior_epilogue(std::bool_constant<(kEpiOps & 1) != 0>{}, std::bool_constant<(kEpiOps & 2) != 0>{});
  } else if (interior) {
    if constexpr (kInteriorPath) {
      using T = std::true_type;
      using F = std::false_type;
      if constexpr (kEpi == kEpiSiluMul) {            // (no residual: the silu-mul epilogue has none)
        if (p.bias) interior_epilogue(T{}, F{});
        else interior_epilogue(F{}, F{});
      } else if (p.bias) {
        if (p.residual) interior_epilogue(T{}, T{});
        else interior_epilogue(T{}, F{});
      } else {
        if (p.residual) interior_epilogue(F{}, T{});
        else interior_epilogue(F{}, F{});
      }
    }
  } else if constexpr (kMfma32) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int m = m0 + wr * WM + i * 32 + (lane & 31);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wc * WN + j * 32 + 8 * g + 4 * (lane >> 5);
          store4(m, n, acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], false, make_uint2(0, 0), make_uint2(0, 0));
        }
      }
  } else {
    // Epilogue operands, fetched AHEAD of their use: a lane's TN bias quads once (they do not depend on the row), the residual quads of
    // row tile i + 1 while row tile i is finished and stored.  (Element-wise loads inside store4, each awaited before the next, cost the
    // model's prefill GEMMs + 19 % with a bias, + 32 % with a residual: tools/tile_epilogue_cost.py.)
    const bool pre = vec_ok && p.splits <= 1 && ((reinterpret_cast<uintptr_t>(p.bias) | reinterpret_cast<uintptr_t>(p.residual)) & 7) == 0;   // (a sliced view may be misaligned)
    const int nb = n0 + wc * WN + 4 * (lane >> 4), mb = m0 + wr * WM + (lane & 15);
    if (pre) {                                 // (two copies of the store loops: `pre` as a constant inside each keeps store4 free of branches on it)
      uint2 bias_v[TN], res_cur[TN], res_nxt[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bias_v[j] = res_cur[j] = res_nxt[j] = make_uint2(0, 0);
        if (p.bias && nb + j * 16 < p.N) bias_v[j] = *reinterpret_cast<const uint2*>(p.bias + nb + j * 16);
      }
      auto res_load = [&](int i, uint2 (&r)[TN]) {
        if (!p.residual) return;
        const int m = mb + i * 16;
#pragma unroll
        for (int j = 0; j < TN; ++j)
          if (m < p.M && nb + j * 16 < p.N) r[j] = *reinterpret_cast<const uint2*>(p.residual + (size_t)m * p.N + nb + j * 16);
      };
      res_load(0, res_cur);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if (i + 1 < TM) res_load(i + 1, res_nxt);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          store4(mb + i * 16, nb + j * 16, acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], true, bias_v[j], res_cur[j]);
          if (i == 0 && j == 0) ARCQ_TILE_STAMP(3);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) res_cur[j] = res_nxt[j];
      }
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          store4(mb + i * 16, nb + j * 16, acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], false, make_uint2(0, 0), make_uint2(0, 0));
          if (i == 0 && j == 0) ARCQ_TILE_STAMP(3);
        }
    }
  }
  ARCQ_TILE_STAMP(4);
  if (kEpi == kEpiSiluMul) {
    __shared__ uint32_t wave_max[WAVES_M * WAVES_N];
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) act_max = max(act_max, (uint32_t)__shfl_down((int)act_max, sh, 64));
    if (lane == 0) wave_max[wave] = act_max;
    __syncthreads();
    if (tid == 0) {
      uint32_t m = 0;
#pragma unroll
      for (int w = 0; w < WAVES_M * WAVES_N; ++w) m = max(m, wave_max[w]);
      p.slots[blockIdx.x] = m;
    }
  }
