// The statements of the tiled MXFP4 GEMM kernel (design: gemm_mx.hip), included inside the braces of a kernel definition.
//
// The kernel header in front of it supplies the template parameter kEpi, the parameter block `MxArgs p` and the constant kRepackedB:
//   false  mx_tile_kernel (gemm_mx.hip): p.B / p.SFB are the reference layout, [N, Kp/2] codes and [N, Kp/32] E8M0 bytes;
//   true   mx_tile_rw_kernel (gemm_mx_tile_rw.hip): p.B / p.SFB are MRW / MRSF of arcq.h "MXFP4 repacked weight".
// Only the global addresses B's codes and scale bytes are fetched from differ (and the lane that carries a chunk to its place): the LDS
// image of a step -- 128 rows x 64 code bytes per operand at mx_lds_off, one dword of four scale bytes per row -- is the same, byte for
// byte, in every row n < N, and compute() and the epilogues are ONE text.  The same MFMAs on the same operands in the same order: the two
// kernels' results are identical bits.  (Included as text, as gemm_tile_body.inc is: mx_tile_kernel's code stays what it was.)
//
// kRepackedB staging.  Codes: the tile's B rows are row blocks b0 .. b0 + 7 (b0 = n0 / 16, clamped to N/16 - 1); step t of row block b is
// the 1 KB at MRW + ((b * steps + t) * 64 + lane) * 16, lane 16 q + r holding chunk q of row r.  Wave w fetches the spans of row blocks
// b0 + w and b0 + w + 4, ONE contiguous 1 KB request each (the reference layout: 16 pieces of 64 bytes from 16 rows), and its lane
// stores the chunk to mx_lds_off(16 j + r, q).  Scales: compute() wants one dword per B row, the row's four E8M0 bytes of step t; MRSF
// keeps them in four dwords, 64 bytes apart, (((b R + t / 32) 8 + t % 8) 64 + 16 q + r) 4 for q = 0 .. 3, byte (t / 8) % 4 of each.  The
// 128 threads that stage B's scale dword (waves 2 and 3) fetch the four and assemble the row's dword when they stash it: the LDS image
// is written by the same one ds_write_b32 per thread, no byte stores.  The other three bytes of each dword belong
// to other steps of the round -- or are MRSF's padding in a partial last round -- and are dropped: no result depends on the padding.
// Every address is inside its operand: row blocks clamped to N/16 - 1, steps to steps - 1 (whose MRSF dwords exist: the array is padded
// to whole rounds), A rows to M - 1.
  __shared__ __attribute__((aligned(16))) uint8_t lds[2 * kMxBufBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kMxTile, n0 = blockIdx.x * kMxTile;
  const size_t rowb = (size_t)(p.Kp >> 1), rows = (size_t)(p.Kp >> 5);
  const int steps = p.Kp >> 7;

  // staging: thread t moves 16-byte chunks t and t + 256 of each operand tile (row = chunk / 4) and one scale dword
  const int cr = tid >> 2, cc = tid & 3;
  const uint8_t* gA0 = p.A + (size_t)min(m0 + cr, p.M - 1) * rowb + cc * 16;
  const uint8_t* gA1 = p.A + (size_t)min(m0 + cr + 64, p.M - 1) * rowb + cc * 16;
  // kRepackedB: the wave's two 1 KB spans of step 0 (row blocks b0 + wave and b0 + wave + 4) and, for a B-scale thread, dword q = 0 of its
  // row in round 0, wave slot 0
  const int nb = p.N >> 4, b0 = n0 >> 4, rounds = (steps + kMxRwRoundSteps - 1) / kMxRwRoundSteps;
  const int sr = (tid - kMxTile) & (kMxTile - 1);              // B row of the tile whose scale dword this thread stages (tid >= kMxTile)
  const uint8_t* gB0 = kRepackedB ? p.B + ((size_t)min(b0 + wave, nb - 1) * (size_t)steps * 64 + (size_t)lane) * 16
                                  : p.B + (size_t)min(n0 + cr, p.N - 1) * rowb + cc * 16;
  const uint8_t* gB1 = kRepackedB ? p.B + ((size_t)min(b0 + wave + 4, nb - 1) * (size_t)steps * 64 + (size_t)lane) * 16
                                  : p.B + (size_t)min(n0 + cr + 64, p.N - 1) * rowb + cc * 16;
  const uint8_t* gS = tid < kMxTile ? p.SFA + (size_t)min(m0 + tid, p.M - 1) * rows
                      : kRepackedB  ? p.SFB + ((size_t)min(b0 + (sr >> 4), nb - 1) * (size_t)rounds * 512 + (size_t)(sr & 15)) * 4
                                    : p.SFB + (size_t)min(n0 + tid - kMxTile, p.N - 1) * rows;
  const int l0 = mx_lds_off(cr, cc), l1 = mx_lds_off(cr + 64, cc);
  const int lb0 = kRepackedB ? mx_lds_off(16 * wave + (lane & 15), lane >> 4) : l0;     // lane 16 q + r: chunk q of row 16 wave + r
  const int lb1 = kRepackedB ? mx_lds_off(16 * wave + (lane & 15) + 64, lane >> 4) : l1;
  // the load of a step past the end re-reads the last step (stashed where nothing reads it): no branch around the loads
  uint4 ra0, ra1, rb0, rb1;
  uint32_t rs;
  // kRepackedB: the dwords of q = 1 .. 3 (qs = 64 bytes apart) and 8 x the byte of the loaded step in them.  Branch-free: an A-scale thread
  // has qs = 0, requests its own dword again (the same address: no further line) and keeps it when it stashes
  [[maybe_unused]] uint32_t rs1, rs2, rs3;
  [[maybe_unused]] int rsh;
  [[maybe_unused]] const bool bscale = tid >= kMxTile;
  [[maybe_unused]] const int qs = bscale ? 64 : 0;
  auto load = [&](int s) __attribute__((always_inline)) {
    const size_t o = (size_t)min(s, steps - 1) * 64;
    ra0 = *reinterpret_cast<const uint4*>(gA0 + o);
    ra1 = *reinterpret_cast<const uint4*>(gA1 + o);
    if constexpr (kRepackedB) {
      const int t = min(s, steps - 1);
      rb0 = *reinterpret_cast<const uint4*>(gB0 + o * 16);
      rb1 = *reinterpret_cast<const uint4*>(gB1 + o * 16);
      const uint8_t* g = gS + (bscale ? (size_t)((t >> 5) * 8 + (t & 7)) * 256 : o / 16);
      rs = *reinterpret_cast<const uint32_t*>(g);
      rs1 = *reinterpret_cast<const uint32_t*>(g + qs);
      rs2 = *reinterpret_cast<const uint32_t*>(g + 2 * qs);
      rs3 = *reinterpret_cast<const uint32_t*>(g + 3 * qs);
      rsh = 8 * ((t >> 3) & 3);
    } else {
      rb0 = *reinterpret_cast<const uint4*>(gB0 + o);
      rb1 = *reinterpret_cast<const uint4*>(gB1 + o);
      rs = *reinterpret_cast<const uint32_t*>(gS + o / 16);
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
    uint8_t* L = lds + buf * kMxBufBytes;
    if constexpr (kRepackedB) {
      const uint32_t row = ((rs >> rsh) & 0xffu) | (((rs1 >> rsh) & 0xffu) << 8) | (((rs2 >> rsh) & 0xffu) << 16) | (((rs3 >> rsh) & 0xffu) << 24);
      rs = bscale ? row : rs;
    }
    *reinterpret_cast<uint4*>(L + l0) = ra0;
    *reinterpret_cast<uint4*>(L + l1) = ra1;
    *reinterpret_cast<uint4*>(L + kMxOpBytes + lb0) = rb0;
    *reinterpret_cast<uint4*>(L + kMxOpBytes + lb1) = rb1;
    reinterpret_cast<uint32_t*>(L + 2 * kMxOpBytes)[tid] = rs;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int r32 = lane & 31, h = lane >> 5;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const uint8_t* L = lds + buf * kMxBufBytes;
    const uint32_t* LS = reinterpret_cast<const uint32_t*>(L + 2 * kMxOpBytes);
    uint32_t sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      sa[i] = LS[wm * 64 + i * 32 + r32];
      sb[i] = LS[kMxTile + wn * 64 + i * 32 + r32];
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {            // two K-64 halves of the step: logical chunk 2 sub + h of each row
      const int sh = 8 * (2 * sub + h);
      i32x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = frag(*reinterpret_cast<const uint4*>(L + mx_lds_off(wm * 64 + i * 32 + r32, 2 * sub + h)));
        b[i] = frag(*reinterpret_cast<const uint4*>(L + kMxOpBytes + mx_lds_off(wn * 64 + i * 32 + r32, 2 * sub + h)));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], 4, 4, 0, (int)(sa[i] >> sh), 0,
                                                                      (int)(sb[j] >> sh));
    }
  };

  // the loads of step s + 1 are issued before step s computes and stored to the other LDS buffer after it.  The scheduling
  // barriers pin that order: left to itself the compiler hoists the LDS stores above the MFMAs (or sinks the loads below
  // them), and every step then waits out the full global latency.
  load(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    load(s + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(s & 1);
    __builtin_amdgcn_sched_barrier(0);
    stash((s + 1) & 1);
    __syncthreads();
  }

  const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
  if constexpr (kEpi == kEpiSiluMulQuant) {
    // every wave is past its last read of the staging buffers (the barrier that ends the K loop); N % 128 == 0: no column is outside
    const bool odd = lane & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nl = wn * 64 + j * 32 + r32;                 // y-column within the tile
        const float bias = p.bias ? bf16_bits_to_f32(p.bias[n0 + nl]) : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, acc[i][j][r], p.bias, bias), mx_y_bits(alpha, acc[i][j][r + 1], p.bias, bias), odd);
          const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h + (odd ? 1 : 0);
          if (!(lane & 2)) *reinterpret_cast<uint32_t*>(lds + ml * kMxActRowBytes + (nl >> 1) * 2) = pk;   // rows >= M hold clamped rows' values
        }
      }
    __syncthreads();
    const int ml = tid >> 1, bl = tid & 1;                     // thread -> (row, block): a lane pair stores 32 adjacent code bytes
    if (m0 + ml < p.M) mx_quantize_act_block(p, lds + ml * kMxActRowBytes + bl * 64, m0 + ml, (n0 >> 6) + bl);
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + r32;
      if (n >= p.N) continue;
      if constexpr (kEpi == kEpiSiluMul) {
        const bool odd = lane & 1;
        const float bias = p.bias ? bf16_bits_to_f32(p.bias[n]) : 0.0f;
        uint16_t* act = reinterpret_cast<uint16_t*>(p.D) + (n >> 1);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {                    // rows r and r + 1 of the register tile are adjacent rows of D
          const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, acc[i][j][r], p.bias, bias), mx_y_bits(alpha, acc[i][j][r + 1], p.bias, bias), odd);
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h + (odd ? 1 : 0);
          if (!(lane & 2) && m < p.M) *reinterpret_cast<uint32_t*>(act + (size_t)m * (size_t)(p.N >> 1)) = pk;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (m < p.M) mx_store(p, alpha, m, n, acc[i][j][r]);
        }
      }
    }
