"""Every host limit of the offset ledger from both sides, through the C boundary and without a GPU.

No call here can launch.  The REFUSED side of a limit returns the status and text the code has today.  The ACCEPTED side is shown by
what the boundary reports next: the checks run in a pinned order (arcq_internal.hpp), so the last shape inside a limit, called with a
pointer that fails a LATER check (a misaligned or NULL operand), reports that later fault instead of the limit's -- or by the route
and predicate functions where the limit lives behind one.  Two limits sit immediately in front of a launch (the tile kernel's K and
the decode kernels' 4 GiB): their refused side is here, and their accepted side is the arithmetic below against Python's integers;
shapes inside them run in tests/test_large_operands_nvfp4_gpu.py.

The pure size helpers are checked at extreme arguments (rows near 2^31, K at its maximum) against Python's unbounded integers."""
import pytest

from arcquant_amd import _lib

P = 4096                    # a fake, 16-byte aligned device pointer: never dereferenced on these paths
I31, I32 = (1 << 31) - 1, 1 << 32
DIM = I31 // 2              # the boundary's cap of M, N, K: INT32_MAX / 2
BIG_WS = 1 << 50


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _err(L):
    return L.arcq_last_error().decode()


def _gemm(L, M, N, K, A=P, fn="arcq_gemm_nvfp4", ws=BIG_WS):
    return getattr(L, fn)(A, P, P, P, P, M, N, K, 1.0, None, None, None, 0, P, ws, None)


def _accepted_by_size_check(L, st):
    """The call was made with A misaligned: the size check passed iff the alignment check reports."""
    return st == -1 and "must be 16-byte aligned" in _err(L)


# ---- "shape too large" --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["arcq_gemm_nvfp4", "arcq_gemm_nvfp4_rw"])
def test_gemm_dimension_caps(L, fn):
    for inside, outside in [((DIM, 1024, 64), (DIM + 1, 1024, 64)), ((1024, DIM, 64), (1024, DIM + 1, 64)),
                            ((1024, 1024, DIM - DIM % 64), (1024, 1024, DIM + 1)),
                            ((1 << 21, 1 << 19, 64), (1 << 21, (1 << 19) + 1, 64))]:          # M N <= 2^40
        assert _accepted_by_size_check(L, _gemm(L, *inside, A=P + 2, fn=fn)), (inside, _err(L))
        assert _gemm(L, *outside, fn=fn) == -2 and _err(L) == f"{fn}: shape too large", (outside, _err(L))


def test_mx_gemm_row_cap_keeps_grid_y_below_65536(L):
    top = 65535 * 128
    for fn in ("arcq_gemm_mxfp4", "arcq_gemm_mxfp4_rw"):
        call = lambda M, A: (getattr(L, fn)(A, P, P, P, P, M, 1024, 128, 1.0, None, None, None, 0, None, 0, None) if fn == "arcq_gemm_mxfp4"
                             else getattr(L, fn)(A, P, P, P, P, M, 1024, 128, 1.0, None, None, None, 0, None))
        assert (top + 127) // 128 == 65535 and (top + 1 + 127) // 128 == 65536
        assert _accepted_by_size_check(L, call(top, P + 2)), _err(L)
        assert call(top + 1, P) == -2 and _err(L) == f"{fn}: shape too large"


def test_repacked_and_fused_entries_cap_m_at_int32(L):
    """The repacked and fused entries leave M to their kernels' predicates, which see it as int: M beyond INT32_MAX is refused before."""
    for fn in ("arcq_gemm_nvfp4_repacked", "arcq_gemm_nvfp4_repacked_stream"):
        call = lambda M, A: getattr(L, fn)(A, P, P, P, P, M, 4096, 64, 1.0, None, None, None, 0, None)
        assert _accepted_by_size_check(L, call(I31, P + 2)), _err(L)
        assert call(I31 + 1, P) == -2 and _err(L) == f"{fn}: shape too large"
        assert call(I32 + 8, P) == -2 and _err(L) == f"{fn}: shape too large"          # (it ran as M = 8 before)
    lin = lambda M, X: L.arcq_linear_rmsnorm_repacked(X, P, 1e-6, P, P, P, P, M, 4096, 4096, 64, 0, 1.0, None, None, None, 0, None)
    assert _accepted_by_size_check(L, lin(I31, P + 2)), _err(L)
    assert lin(I32 + 8, P) == -2 and _err(L) == "arcq_linear_rmsnorm_repacked: shape too large"


# ---- the M <= 16 repacked kernels' 32-bit element offset m * N + n (new refusal) ------------------------------------------------------
def test_repacked_output_offsets_fit_32_bits(L):
    text = "{}: M * N = {} elements exceed the decode kernels' 32-bit output offsets"
    for M, n_last in [(16, 1 << 28), (15, I32 // 15), (5, I32 // 5)]:
        n_last -= n_last % 4
        assert (M - 1) * n_last + n_last - 1 < I32 <= (M - 1) * (n_last + 4) + n_last + 3 or M * n_last == I32
        assert L.arcq_gemm_repacked_supported(M, n_last, 64) == 1
        assert L.arcq_gemm_repacked_supported(M, n_last + 4, 64) == 0
        for fn in ("arcq_gemm_nvfp4_repacked", "arcq_gemm_nvfp4_repacked_stream"):
            call = lambda N, A: getattr(L, fn)(A, P, P, P, P, M, N, 64, 1.0, None, None, None, 0, None)
            assert _accepted_by_size_check(L, call(n_last, P + 2))
            assert call(n_last + 4, P) == -2 and _err(L) == text.format("arcq_gemm_nvfp4_repacked", M * (n_last + 4)), _err(L)
    assert L.arcq_gemm_repacked_supported(1, DIM, 64) == 1 and L.arcq_gemm_repacked_supported(2, DIM, 64) == 1      # M N < 2^32 up to the caps
    assert L.arcq_gemm_rw_route(16, 1 << 28, 64) == 1 and L.arcq_gemm_rw_route(16, (1 << 28) + 4, 64) != 1
    N = (1 << 28) + 4
    assert L.arcq_linear_fused_supported(2, 16, 1 << 28, 64, 0) == 1 and L.arcq_linear_fused_supported(2, 16, N, 64, 0) == 0
    st = L.arcq_linear_dynamic_repacked(P, P, P, P, P, P, None, 0, 16, N, 64, 0, 0, 1.0, None, None, 0, None)
    assert st == -2 and _err(L) == text.format("arcq_linear_dynamic_repacked", 16 * N), _err(L)


# ---- gemm_regtile_fits ---------------------------------------------------------------------------------------------------------------
def test_register_tiled_kernel_keeps_every_operand_below_2gib(L):
    M, K = 16, 16384
    inside, outside = 262128, 262144
    assert inside * (K // 2) == 2147352576 < 1 << 31 == outside * (K // 2)
    assert L.arcq_gemm_rw_route(M, inside, K) == 2 and L.arcq_gemm_rw_route(M, outside, K) == 0
    assert L.arcq_gemm_workspace_bytes(M, inside, K) == 0 and L.arcq_gemm_workspace_bytes(M, outside, K) == 0
    st = _gemm(L, M, outside, K, fn="arcq_gemm_nvfp4_rw")
    assert st == -2 and _err(L) == f"arcq_gemm_nvfp4_rw: the repacked weight of N={outside} K={K} exceeds the register-tiled kernel's 32-bit offsets"


# ---- the limits in front of a launch: refused side ------------------------------------------------------------------------------------
def test_tile_kernel_refuses_a_k_whose_tile_rows_pass_32_bits(L):
    k_last = 33554176
    assert (k_last + 255) // 256 * 256 * 128 <= 0xFFFFFFFF < (k_last + 64 + 255) // 256 * 256 * 128
    assert 256 * (k_last // 2) < I32                                           # 256 rows of codes: what the lane offsets span
    for K in (k_last + 64, 1 << 25, DIM - DIM % 64):
        assert _gemm(L, 256, 256, K) == -1
        assert _err(L) == f"arcq_gemm_nvfp4 (tile): K = {K}: a tile's rows of an operand exceed 32-bit offsets"
    assert _gemm(L, 256, 256, k_last + 64, fn="arcq_gemm_nvfp4_rw") == -1 and "a tile's rows of an operand exceed 32-bit offsets" in _err(L)


def test_decode_kernels_refuse_operands_of_4gib(L):
    # 32-row decode kernel (wide N): N K / 2 = 2^32; the last N inside keeps 16 N < 2^32 for finish4<uint32_t>
    N, K = 1 << 27, 64
    assert N * (K // 2) == I32 and 16 * (N - 1) < I32
    assert _gemm(L, 4, N, K) == -2 and _err(L) == "arcq_gemm_nvfp4 (decode): operand larger than 4 GiB"
    assert L.arcq_gemm_nvfp4_silu_mul(P, P, P, P, P, P, 4, N, K, 1.0, None, None, None) == -2 and "operand larger than 4 GiB" in _err(L)
    # the scale buffer alone: roundup(N, 128) K / 16 reaches 2^32 only with the codes; both terms are pinned by the first
    # 16-row decode kernel (narrow N, long K)
    N, K = 4096, 1 << 21
    assert N * (K // 2) == I32 and (N + 127) // 128 * 4 < 160
    assert _gemm(L, 4, N, K) == -2 and _err(L) == "arcq_gemm_nvfp4 (skinny): operand larger than 4 GiB"


# ---- quantisers: "too many rows" -------------------------------------------------------------------------------------------------------
def test_quantisers_count_rows_in_int32(L):
    q = lambda fn, rows, Q: getattr(L, fn)(P, P, Q, P, rows, 4096, 64, 0, None)
    for fn in ("arcq_quantize_x", "arcq_quantize_w"):
        assert q(fn, I31, P + 4) == -1 and "aligned" in _err(L)               # the row check passed: the next one reports
        assert q(fn, I31 + 1, P) == -2 and _err(L) == f"{fn}: too many rows"
    mx = lambda fn, rows, Q: getattr(L, fn)(P, P, Q, P, rows, 4096, 64, None)
    for fn in ("arcq_mx_quantize_x", "arcq_mx_quantize_w"):
        assert mx(fn, I31, P + 4) == -1 and "aligned" in _err(L)
        assert mx(fn, I31 + 1, P) == -2 and _err(L) == f"{fn}: too many rows"
    rms = lambda rows, Q: L.arcq_rmsnorm_quantize_x(P, P, 1e-6, P, Q, P, rows, 4096, 64, 0, None)
    assert rms(I31, P + 4) == -1 and "aligned" in _err(L)
    assert rms(I31 + 1, P) == -2 and _err(L) == "arcq_rmsnorm_quantize_x: too many rows"


# ---- KV ----------------------------------------------------------------------------------------------------------------------------------
def test_kv_positions_fit_int32(L):
    Pg = 16
    nnz_last = I31 // Pg
    assert nnz_last * Pg <= I31 < (nnz_last + 1) * Pg
    dec = lambda nnz: L.arcq_kv_batch_decode(None, P, P, P, P, P, P, 2, 4, 2, 0, 2, Pg, nnz, 0, 0, None, 0, None)
    pre = lambda nnz: L.arcq_kv_batch_prefill(None, P, P, P, P, P, P, P, 8, 2, 4, 2, 0, 2, Pg, nnz, 0, 0, None)
    step = lambda nnz: L.arcq_kv_decode_step(None, P, P, P, 512, 256, P, P, P, P, P, 2, 4, 2, 0, 2, Pg, nnz, 0, 0, None, 0, None, 0, None)
    for who, f in (("arcq_kv_batch_decode", dec), ("arcq_kv_batch_prefill", pre), ("arcq_kv_decode_step", step)):
        assert f(nnz_last) == -4 and _err(L) == f"{who}: NULL pointer"         # the range check passed: the NULL output reports
        assert f(nnz_last + 1) == -1 and _err(L) == f"{who}: nnz={nnz_last + 1} pages of P={Pg} entries are out of range"


def test_kv_writer_grids_fit(L):
    lim = 16 * I31
    # RoPE + quantise: ntok (Nq + 2 N) rows
    Nq, N = 32, 8
    b_last = lim // (Nq + 2 * N)
    rope = lambda B: L.arcq_kv_rope_append_quantize(None, P, P, P, P, P, P, P, P, Nq * 128, N * 128, P, P, 4096, B, Nq, 2, 0, N, 16, 0, 0, None)
    assert b_last <= DIM and rope(b_last) == -4 and _err(L) == "arcq_kv_rope_append_quantize: NULL pointer"
    assert rope(b_last + 1) == -1 and _err(L) == "arcq_kv_rope_append_quantize: ntok * (Nq + 2 N) rows are out of range"
    # arcq_rope_qk: ntok (Nq + N) rows
    t_last = lim // (Nq + N)
    qk = lambda n: L.arcq_rope_qk(None, P, Nq * 128, N * 128, P, 1, P, P, 4096, n, Nq, N, 0, None)
    assert qk(t_last) == -4 and qk(t_last + 1) == -1 and _err(L) == "arcq_rope_qk: ntok * (Nq + N) rows are out of range"
    # the plain quantising writers: ntok 2 N rows, 16 per workgroup (new refusal: the count was cut to 32 bits before)
    N = 65535
    b_last = lim // (2 * N)
    assert (b_last * 2 * N + 15) // 16 <= I31 < ((b_last + 1) * 2 * N + 15) // 16
    app = lambda B: L.arcq_kv_append_quantize(None, P, P, P, P, P, P, B, 2, 0, N, 16, 0, 0, None)
    ini = lambda n: L.arcq_kv_init_quantize(None, P, P, P, P, P, P, P, n, 4, 2, 0, N, 16, 0, 0, None)
    for who, f in (("arcq_kv_append_quantize", app), ("arcq_kv_init_quantize", ini)):
        assert f(b_last) == -4 and _err(L) == f"{who}: NULL pointer"
        assert f(b_last + 1) == -1 and _err(L) == f"{who}: ntok * 2 N rows are out of range"
    # the copying writers launch one workgroup per token: no such limit below the ntok cap
    assert L.arcq_kv_append(None, P, P, P, P, P, P, P, P, DIM, 2, 0, N, 16, 0, None) == -4


# ---- pure helpers against Python's integers ----------------------------------------------------------------------------------------------
def _sf_offset(r, p, K):
    return ((r // 128) * (K // 64) + p // 4) * 512 + (r % 32) * 16 + ((r // 32) % 4) * 4 + p % 4


ROWS = [1, 127, 128, 129, (1 << 31) - 129, (1 << 31) - 128, (1 << 31) - 1]
KS = [64, 4160, DIM - DIM % 256, DIM - DIM % 64]


def test_scale_layout_helpers_at_extreme_arguments(L):
    for K in KS:
        for rows in ROWS:
            assert L.arcq_sf_alloc_bytes(rows, K) == (rows // 128 + 1) * 128 * K // 16
            assert L.arcq_sf_used_bytes(rows, K) == (rows + 127) // 128 * 128 * K // 16
            for p in (0, 1, 3, 4, K // 16 - 1):
                assert L.arcq_sf_offset(rows - 1, p, K) == _sf_offset(rows - 1, p, K)
            assert L.arcq_sf_offset(rows - 1, K // 16 - 1, K) < L.arcq_sf_used_bytes(rows, K) < 1 << 63


def test_repacked_size_helpers_at_extreme_arguments(L):
    for K in KS:
        for N in (1, 15, 16, 17, DIM - 1, DIM):
            pairs = (K + 255) // 256
            assert L.arcq_repacked_w_bytes(N, K) == (N + 15) // 16 * pairs * 2048
            assert L.arcq_repacked_sf_bytes(N, K) == (N + 15) // 16 * pairs * 256
    for Kp in (128, 4096, 4224, DIM - DIM % 128):
        for N in (16, 4096, DIM - DIM % 16):
            assert L.arcq_mx_repacked_w_bytes(N, Kp) == N * Kp // 2
            assert L.arcq_mx_repacked_sf_bytes(N, Kp) == N // 16 * ((Kp + 4095) // 4096) * 2048
    assert L.arcq_mx_repacked_w_bytes(DIM, 128) == 0 and L.arcq_mx_repacked_sf_bytes(16, DIM) == 0       # (N % 16, K % 128: no such weight)


def test_gemm_workspace_helpers_at_extreme_arguments(L):
    # many tiles: no split-K, whatever the size
    for fn in (L.arcq_gemm_workspace_bytes, L.arcq_gemm_rw_workspace_bytes):
        assert fn(DIM, 1024, 64) == 0 and fn(1 << 21, 1 << 19, 64) == 0 and fn(4096, DIM, DIM - DIM % 64) == 0
    # one 64 x 256 tile over the longest K: the split rule (tile_split) doubles while tiles * s < 256, >= 16 atoms stay per split and s < 32
    M, N, K = 64, 256, DIM - DIM % 64
    atoms, s = K // 64, 1
    while 1 * s < 256 and atoms // (s * 2) >= 8 and s < 32:
        s *= 2
    per = (atoms + s - 1) // s
    splits = (atoms + per - 1) // per
    assert splits == 32 and L.arcq_gemm_workspace_bytes(M, N, K) == splits * M * N * 4
    assert L.arcq_gemm_workspace_bytes(0, N, K) == 0 and L.arcq_gemm_rw_workspace_bytes(M, 0, K) == 0


def _kv_splits(B, Nq, N, nnz, Pg):
    g = Nq // N
    gc = 1 if g == 1 else 2 if g == 2 else 4
    chunks = (g + gc - 1) // gc
    S = min((1024 + B * N * chunks - 1) // (B * N * chunks), (nnz * Pg // B) // 128, 32)
    return max(S, 1), chunks


def test_kv_size_helpers_at_extreme_arguments(L):
    for B, Nq, N, nnz, Pg in [(1, 4, 1, I31 // 16, 16), (DIM, 1, 1, DIM, 2), (3, 65535, 65535, 1 << 20, 16), (16383, 65535, 1, 1 << 24, 128),
                              (2, 28, 4, 4096, 16), (7, 8, 8, 7, 1)]:
        S, chunks = _kv_splits(B, Nq, N, nnz, Pg)
        assert L.arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, Pg) == (0 if S <= 1 else B * Nq * S * 130 * 4), (B, Nq, N, nnz, Pg)
        assert L.arcq_kv_decode_step_state_bytes(B, Nq, N) == B * N * chunks * 4
    assert L.arcq_kv_decode_step_state_bytes(DIM, 65535, 65535) == DIM * 65535 * 4 > 1 << 47
