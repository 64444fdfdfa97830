"""arcq_gemm_nvfp4 and its siblings with an operand across the 2 GiB and 4 GiB byte marks (``-m gpu``; DESIGN.md 5.2 is the ledger of
the index arithmetic these cases hold in place, tests/bigmem.py the method).

Operands are banded: 7 kinds of 256 rows, each quantised by the oracle from outlier activations / uniform weights with one row of
zeroed scale bytes and one ue4m3-subnormal scale byte (as tests/test_tile_pair_loads_gpu.py), repeated down the operand.  The first
period (1792 rows of D, or 1792 columns where the WEIGHT is the large operand) is held to the project's bound against an fp64 product
of the dequantised operands (tests/test_gpu_parity.py::test_gemm_matches_oracle: fp32 within 2e-6 sum|a b|; bf16 within one ulp of
the fp64 result's rounding and equal on > 99 %); every later band must equal its kind's bits (bigmem.check_bands), the guards of the
output must be unchanged and no 0xFF of its fill may survive.

Which kernel a shape takes is asserted with the library's route functions where one exists (arcq_gemm_rw_route uses arcq_gemm_nvfp4's
own dispatch: 2 = register-tiled, 3 = LDS-tiled) and stated from the dispatch rule otherwise."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as O
from tests import bigmem as BM
from tests.test_gpu_parity import _torch_dequant
from tests.test_tile_pair_loads_gpu import _sf_offsets
from tests.util import bits, outlier_activations, prescale, random_perm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PERIOD = BM.PERIOD


@pytest.fixture(autouse=True)
def _release():
    yield
    BM.release()


def _lib():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _kinds(role, K):
    """7 band kinds of a [256, K] operand, quantised by the oracle -> (codes [7] u8 [256, K/2], scale buffers [7] u8, per-tensor scale of
    kind 0), on the device.  Kind k: its own seed, scale bytes of row 37 + 3 k zeroed, one subnormal scale byte in row 201 - 5 k."""
    KE = 64 if K > 64 else 0
    KQ = K - KE
    idx = random_perm(KQ, 4242 + K).numpy()
    codes, sfs, scale = [], [], None
    for k in range(BM.KINDS):
        seed = 9100 + 17 * k + K + (0 if role == "x" else 5000)
        if role == "x":
            t, s = prescale(outlier_activations(BM.BAND, KQ, seed))
            q, sf = O.quantize_x(bits(t), idx, KE, O.G16, sf_fill=0)
        else:
            t, s = prescale((torch.rand(BM.BAND, KQ, generator=torch.Generator().manual_seed(seed)) * 3 - 1.0).to(torch.bfloat16))
            q, sf = O.quantize_w(bits(t), idx, KE, O.G16, sf_fill=0)
        sf[_sf_offsets(37 + 3 * k, K)] = 0
        sf[_sf_offsets(201 - 5 * k, K)[min(1, K // 16 - 1)]] = 0x03
        scale = float(s) if scale is None else scale
        codes.append(torch.from_numpy(q).to(DEV))
        sfs.append(torch.from_numpy(sf).to(DEV))
    return codes, sfs, scale


def _operand(role, rows, K):
    """The banded [rows, K] operand -> (codes u8 [rows, K/2], swizzled scales u8, scale)."""
    codes, sfs, s = _kinds(role, K)
    return BM.banded_rows(codes, rows), BM.banded_sf_nvfp4(sfs, rows, K), s


def _reference(A, SFA, B, SFB, K, alpha):
    """fp64 alpha * a b^T and alpha * |a| |b|^T of the dequantised operands (torch, on the GPU)."""
    a, b = _torch_dequant(A, SFA, K), _torch_dequant(B, SFB, K)
    return alpha * (a @ b.T), alpha * (a.abs() @ b.abs().T)


def _bf16_key(t):
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where((b & 0x8000) != 0, -(b & 0x7FFF), b & 0x7FFF)


def _check_first_period(got, want, want_abs):
    """test_gemm_matches_oracle's bounds for ``got`` (fp32 or bf16), on the device."""
    if got.dtype == torch.float32:
        err = (got.double() - want).abs()
        worst = float((err / (want_abs + 1e-30)).max())
        print(f"    fp32 vs fp64: max err / sum|ab| = {worst:.3e}")
        assert bool((err <= 2e-6 * want_abs + 1e-30).all()), worst
    else:
        d = (_bf16_key(got) - _bf16_key(want.float().to(torch.bfloat16))).abs()
        ulp, same = int(d.max()), float((d == 0).float().mean())
        print(f"    bf16 vs fp64: max ulp {ulp}, equal {same:.5f}")
        assert ulp <= 1 and same > 0.99, (ulp, same)


def _gemm(A, B, SFA, SFB, out, alpha, bias=None, residual=None, fn="arcq_gemm_nvfp4"):
    M, N, K = A.shape[0], out.shape[1], A.shape[1] * 2
    L = _lib()
    rw = fn.endswith("_rw")
    nbytes = int((L.arcq_gemm_rw_workspace_bytes if rw else L.arcq_gemm_workspace_bytes)(M, N, K))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    st = getattr(L, fn)(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), out.data_ptr(), M, N, K, alpha, None,
                        bias.data_ptr() if bias is not None else None, residual.data_ptr() if residual is not None else None,
                        0 if out.dtype == torch.bfloat16 else 1, ws.data_ptr() if nbytes else None, nbytes, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())


def _tall(M, N, K, dtype, mark=1 << 32):
    """D = A B^T with A banded over M rows -> (A, SFA, B, SFB, alpha, buf, D, want, want_abs of the first period); D checked."""
    esz = 2 if dtype == torch.bfloat16 else 4
    BM.need(M * N * esz + 2 * BM.GUARD + PERIOD * N * 24 + M * K)
    assert M * N * esz > mark
    BM.assert_wrap_visible(BM.BAND * N * esz, M * N * esz, "D")
    A, SFA, sx = _operand("x", M, K)
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw
    buf, D = BM.guarded((M, N), dtype, DEV)
    _gemm(A, B, SFA, SFB, D, alpha)
    want, want_abs = _reference(A[:PERIOD], SFA, B, SFB, K, alpha)
    BM.assert_kinds_differ(want)
    _check_first_period(D[:PERIOD], want, want_abs)
    BM.check_bands(D, buf=buf, what=f"D [{M}, {N}] {dtype}")
    return A, SFA, B, SFB, alpha, buf, D


def _assert_column_wrap_visible(rows, N, esz):
    """D [rows, N] whose bands run over COLUMNS (256 columns of ``esz`` bytes, 7 kinds): an address that is wrong by a mark lands
    ``mark // row_bytes`` rows further and ``mark % row_bytes`` bytes along the row.  Either the column moves by a non-zero amount that is
    no multiple of the 7-band period -- another kind, which check_bands sees -- or it lands in ANOTHER ROW at the same column: the rows
    of A are 256 distinct rows of one kind, the owed element keeps its 0xFF fill, and the first period's reference and fill checks see it."""
    row_bytes, period = N * esz, BM.KINDS * BM.BAND * esz
    for mark in (m for m in (1 << 31, 1 << 32) if rows * row_bytes > m):
        along, down = mark % row_bytes, mark // row_bytes
        assert along % period != 0 or (along == 0 and 0 < down < rows), (N, mark, along, down)


# ---- 1, 2: D past 4 GiB ---------------------------------------------------------------------------------------------------------------
def test_d_past_4gib_all_tiles_interior():
    """(68096, 32768, 64) bf16, 4.16 GiB of D: whole 256 x 256 tiles, >= 192 of them, plain epilogue, BM N < 2^31: the quad-load sibling
    of the overlapped-tail kernel, every tile on the interior epilogue (32-bit ``off`` against a 64-bit tile origin)."""
    M, N, K = 38 * PERIOD, 32768, 64
    assert _lib().arcq_gemm_rw_route(M, N, K) == 3 and M % 256 == 0 and N % 256 == 0 and (M // 256) * (N // 256) >= 192 and 256 * N < 1 << 31
    _tall(M, N, K, torch.bfloat16)


@pytest.mark.parametrize("M,dtype", [(38 * PERIOD + 77, torch.bfloat16), (19 * PERIOD + 77, torch.float32)])
def test_d_past_4gib_ragged_m(M, dtype):
    """The same with 77 more rows: the kept kernel, interior tiles and edge tiles (general epilogue) in one launch; and fp32 output
    (never the interior path) at 4.17 GiB."""
    assert _lib().arcq_gemm_rw_route(M, 32768, 64) == 3
    _tall(M, 32768, 64, dtype)


# ---- 3: epilogue operands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True])
def test_d_past_4gib_bias_and_residual(alias):
    """Case 1 with a bias and a banded residual (4.16 GiB too), and with the residual aliasing D.  Expected bits of the first period: the
    plain fp32 result of its 1792 rows (the same tile configuration, general epilogue), then the torch expression of
    test_gemm_epilogue_operands_on_every_kernel; every later band equals its kind (the residual is banded like A)."""
    M, N, K = 38 * PERIOD, 32768, 64
    nbytes = M * N * 2
    BM.need((1 if alias else 2) * nbytes + PERIOD * N * 16)
    assert nbytes > 1 << 32
    BM.assert_wrap_visible(BM.BAND * N * 2, nbytes, "D")
    BM.assert_wrap_visible(BM.BAND * N * 2, nbytes, "the residual")
    A, SFA, sx = _operand("x", M, K)
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw
    g = torch.Generator().manual_seed(33)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    res_kinds = [torch.randn(BM.BAND, N, generator=g).to(torch.bfloat16).to(DEV) for _ in range(BM.KINDS)]
    plain32 = torch.empty((PERIOD, N), dtype=torch.float32, device=DEV)
    _gemm(A[:PERIOD], B, SFA, SFB, plain32, alpha)
    want = torch.cat(res_kinds) + (plain32.to(torch.bfloat16) + bias)
    del plain32
    buf, D = BM.guarded((M, N), torch.bfloat16, DEV)
    if alias:
        D.copy_(BM.banded_rows(res_kinds, M))
        res = D
    else:
        res = BM.banded_rows(res_kinds, M)
    _gemm(A, B, SFA, SFB, D, alpha, bias=bias, residual=res)
    assert not torch.equal(want, torch.cat(res_kinds)), "the product took no part"
    BM.assert_kinds_differ(want.float())
    if not torch.equal(D[:PERIOD], want):
        r, c = BM._first_diff(D[:PERIOD].view(torch.int16), want.view(torch.int16))
        raise AssertionError(f"first period differs from the torch expression first at (row {r}, column {c}), byte offset {(r * N + c) * 2}")
    BM.check_bands(D, buf=buf, what="D with bias + residual" + (" (aliased)" if alias else ""))


# ---- 4: the interior epilogue's 32-bit offset from both sides -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [(1 << 31) // 256 - 256, (1 << 31) // 256])
def test_interior_guard_from_both_sides(N):
    """M = 256 takes BM = 256 (>= 192 tiles of 256 x 256).  N = 2^31 / 256 - 256: the largest N on the interior path, ``off`` up to
    2^31 - 256 - 1 elements; N = 2^31 / 256: BM N < 2^31 fails and the launch must take the general epilogue.  The WEIGHT rows are
    banded, so D's bands run over its columns.  D is 4 GiB, B 256 MiB."""
    M, K = 256, 64
    assert _lib().arcq_gemm_rw_route(M, N, K) == 3 and (N // 256) >= 192 and N % 256 == 0
    assert (256 * N < 1 << 31) == (N < (1 << 31) // 256)
    BM.need(M * N * 2 + N * K + PERIOD * M * 24)
    _assert_column_wrap_visible(M, N, 2)
    assert N * K // 2 < 1 << 31                   # (B, 256 MiB, crosses no mark)
    assert M * N * 2 >= (1 << 32) - 256 * 512 and (M - 1) * N * 2 > 1 << 31       # (rows past the 2 GiB mark; the last row ends at 4 GiB)
    codes, sfs, sx = _kinds("x", K)
    A, SFA = codes[0], sfs[0]
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw
    buf, D = BM.guarded((M, N), torch.bfloat16, DEV)
    _gemm(A, B, SFA, SFB, D, alpha)
    want, want_abs = _reference(A, SFA, B[:PERIOD], SFB, K, alpha)
    BM.assert_kinds_differ(want, axis=1)
    _check_first_period(D[:, :PERIOD].contiguous(), want, want_abs)
    BM.check_bands(D, axis=1, buf=buf, what=f"D [256, {N}]")


# ---- 5, 6: A past 4 GiB; the repacked-weight entry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_past_4gib(dtype):
    """(600 * 1792, 16, 8192): 4.1 GiB of codes and 525 MiB of scale bytes on the A side (descriptors at the tile origin, 64-bit), and
    arcq_gemm_nvfp4_rw over the repacked weight (route 3) bit-equal to it."""
    from arcquant_amd import agemm as ag
    M, N, K = 600 * PERIOD, 16, 8192
    assert _lib().arcq_gemm_rw_route(M, N, K) == 3
    BM.need(M * K // 2 + M * K // 16 + (1 << 30))
    assert M * K // 2 > 1 << 32
    BM.assert_wrap_visible(BM.BAND * K // 2, M * K // 2, "A")
    A, SFA, sx = _operand("x", M, K)
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw
    buf, D = BM.guarded((M, N), dtype, DEV)
    _gemm(A, B, SFA, SFB, D, alpha)
    want, want_abs = _reference(A[:PERIOD], SFA, B, SFB, K, alpha)
    BM.assert_kinds_differ(want)
    _check_first_period(D[:PERIOD], want, want_abs)
    BM.check_bands(D, buf=buf, what=f"D of A past 4 GiB, {dtype}")
    RW, RSF = ag.repack_w(B, SFB)
    buf2, D2 = BM.guarded((M, N), dtype, DEV)
    _gemm(A, RW, SFA, RSF, D2, alpha, fn="arcq_gemm_nvfp4_rw")
    assert torch.equal(D2.view(torch.int16), D.view(torch.int16)), "arcq_gemm_nvfp4_rw differs from arcq_gemm_nvfp4"
    BM.check_guards(buf2, "D of arcq_gemm_nvfp4_rw")


def test_rw_entry_d_past_4gib():
    """arcq_gemm_nvfp4_rw on case 1 (route 3, the paired-load kernel over RW) bit-equal to arcq_gemm_nvfp4."""
    from arcquant_amd import agemm as ag
    M, N, K = 38 * PERIOD, 32768, 64
    assert _lib().arcq_gemm_rw_route(M, N, K) == 3
    BM.need(2 * M * N * 2 + (1 << 30))
    A, SFA, B, SFB, alpha, buf, D = _tall(M, N, K, torch.bfloat16)
    RW, RSF = ag.repack_w(B, SFB)
    buf2, D2 = BM.guarded((M, N), torch.bfloat16, DEV)
    _gemm(A, RW, SFA, RSF, D2, alpha, fn="arcq_gemm_nvfp4_rw")
    for r0 in range(0, M, 2 * PERIOD):
        if not torch.equal(D2[r0:r0 + 2 * PERIOD].view(torch.int16), D[r0:r0 + 2 * PERIOD].view(torch.int16)):
            r, c = BM._first_diff(D2[r0:r0 + 2 * PERIOD].view(torch.int16), D[r0:r0 + 2 * PERIOD].view(torch.int16))
            raise AssertionError(f"arcq_gemm_nvfp4_rw differs first at (row {r0 + r}, column {c}), byte offset {((r0 + r) * N + c) * 2}")
    BM.check_guards(buf2, "D of arcq_gemm_nvfp4_rw")


@pytest.mark.parametrize("rw", [False, True])
def test_silu_mul_act_past_4gib(rw):
    """arcq_gemm_nvfp4_silu_mul / _rw_silu_mul at (68096, 65536, 64): ACT bf16 [M, N / 2] is 4.16 GiB.  First period: bit-equal to
    silu(y[:, 0::2]) * y[:, 1::2] of the plain fp32 result rounded to bf16 (tests/test_tile_epilogue_gpu.py); the abs-max slots, one per
    workgroup, must hold the maximum of ACT."""
    from arcquant_amd import agemm as ag
    M, N, K = 38 * PERIOD, 65536, 64
    L = _lib()
    BM.need(M * N + PERIOD * N * 12 + (1 << 30))
    assert M * (N // 2) * 2 > 1 << 32
    BM.assert_wrap_visible(BM.BAND * N, M * N, "ACT")
    A, SFA, sx = _operand("x", M, K)
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw * 40.0
    x32 = torch.empty((PERIOD, N), dtype=torch.float32, device=DEV)
    _gemm(A[:PERIOD], B, SFA, SFB, x32, alpha)
    y = x32.to(torch.bfloat16)
    del x32
    want = F.silu(y[:, 0::2]) * y[:, 1::2]
    del y
    BM.assert_kinds_differ(want.float())
    nslots = int((L.arcq_gemm_rw_silu_mul_slots if rw else L.arcq_gemm_silu_mul_slots)(M, N, K))
    assert nslots == (M // 256) * (N // 256)
    slots = torch.full((nslots,), -1, dtype=torch.int32, device=DEV)
    buf, ACT = BM.guarded((M, N // 2), torch.bfloat16, DEV)
    W, SW = ag.repack_w(B, SFB) if rw else (B, SFB)
    fn = L.arcq_gemm_nvfp4_rw_silu_mul if rw else L.arcq_gemm_nvfp4_silu_mul
    st = fn(A.data_ptr(), W.data_ptr(), SFA.data_ptr(), SW.data_ptr(), ACT.data_ptr(), slots.data_ptr(), M, N, K, alpha, None, None, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    assert torch.equal(ACT[:PERIOD], want), "first period differs from silu(gate) * up of the plain result"
    BM.check_bands(ACT, buf=buf, what="ACT")
    assert int(slots.min()) >= 0 and int(slots.max()) == int((want.view(torch.int16).to(torch.int32) & 0x7FFF).max()), "abs-max slots"


# ---- 7: the weight at the register-tiled kernel's limit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [262128, 262144])
def test_weight_at_the_register_tiled_limit(N):
    """M = 16, K = 16384.  N = 262128: the weight is 2 147 352 576 bytes, below 2^31 -- gemm_regtile_fits holds, 16 x 16 register tiles with
    32-bit operand offsets up to the last row.  N = 262144: exactly 2^31 -- it must take the 32-row decode kernel (64-bit bases, 32-bit
    offsets below 4 GiB).  Route 2 / 0 of arcq_gemm_rw_route is the same predicate over the repacked weight of the same size.  The
    weight rows are banded, D's bands run over columns; fp32 output.  arcq_gemm_nvfp4_repacked runs over the same weight at M = 4,
    where arcq_gemm_repacked_supported says yes (M = 16: the fp16 image of 16 x 16384 does not fit LDS)."""
    from arcquant_amd import agemm as ag
    M, K = 16, 16384
    L = _lib()
    fits = N * (K // 2) < 1 << 31
    assert fits == (N == 262128) and L.arcq_gemm_rw_route(M, N, K) == (2 if fits else 0) and L.arcq_gemm_workspace_bytes(M, N, K) == 0
    assert L.arcq_gemm_repacked_supported(16, N, K) == 0 and L.arcq_gemm_repacked_supported(4, N, K) == 1
    BM.need(5 * N * (K // 2))
    # the weight ends AT the 2 GiB mark or 128 KiB in front of it: no byte of it lies at or beyond a mark, so no in-range address can
    # wrap; what a signed or 31-bit offset would get wrong are its LAST rows, whose bands (1022 and up) check_bands holds to their kinds.
    # D (16 x N fp32, 16 MiB) crosses nothing.
    assert (1 << 31) - (1 << 20) < N * (K // 2) <= 1 << 31 and 16 * N * 4 < 1 << 31
    codes, sfs, sx = _kinds("x", K)
    A, SFA = codes[1][:M].contiguous(), sfs[1]
    B, SFB, sw = _operand("w", N, K)
    alpha = sx * sw
    want, want_abs = _reference(A, SFA, B[:PERIOD], SFB, K, alpha)
    BM.assert_kinds_differ(want, axis=1, min_distinct=64)
    buf, D = BM.guarded((M, N), torch.float32, DEV)
    _gemm(A, B, SFA, SFB, D, alpha)
    _check_first_period(D[:, :PERIOD].contiguous(), want, want_abs)
    BM.check_bands(D, axis=1, buf=buf, what=f"D [16, {N}]")
    # the repacked decode kernel over the same weight
    RW, RSF = ag.repack_w(B, SFB)
    del B
    BM.release()
    buf4, D4 = BM.guarded((4, N), torch.float32, DEV)
    st = L.arcq_gemm_nvfp4_repacked(A.data_ptr(), RW.data_ptr(), SFA.data_ptr(), RSF.data_ptr(), D4.data_ptr(), 4, N, K, alpha, None, None, None, 1,
                                    _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _check_first_period(D4[:, :PERIOD].contiguous(), want[:4], want_abs[:4])
    BM.check_bands(D4, axis=1, buf=buf4, what=f"D [4, {N}] of arcq_gemm_nvfp4_repacked")
