"""The tile GEMM's operand staging (arcquant_amd/csrc/gemm_tile_body.inc, gemm_tile_common.hpp) on EXACT results (``-m gpu``).

The staging loads address an operand as [descriptor at the tile origin] + [32-bit lane offset] + [scalar byte offset of the K step], and
the two scale bytes of a staging unit become ONE packed fp16 pair whose halves the dequantising multiplies select.  A wrong half, a
lost mantissa bit of a scale, a lane offset taken against the wrong origin, a K step offset of the wrong layout or a descriptor that
ends short of the tile all give wrong products -- in some rows, some K atoms or some scale values only -- that a tolerance could absorb.
So operands are built directly (code bytes and scale bytes in the swizzled layout of tests/test_gpu_parity._torch_dequant; no quantiser)
such that the fp32 result is exact in ANY summation order, and ``torch.equal`` against the fp64 product of the dequantised operands is
the bar -- for the fp32 output, and for the bf16 output against its round-to-nearest-even rounding:

  * ONE-HOT: every row of one operand holds a single non-zero code (the other 2 K - 1 codes are +0 / -0), the other operand is dense;
    scale bytes are drawn from all 127 finite ue4m3 bytes 0x00 .. 0x7e and codes from all 16 on both operands.  Every output is a single
    product of two values of at most 6 significant bits: exact at any K.  Run with the weight one-hot, and with the activations one-hot.
  * MANTISSA: dense codes, scale bytes the ue4m3 codes of {0.5, 0.75, 1, 1.5, 2, 3} (both values of the top mantissa bit, three
    exponents).  A dequantised value is a multiple of 2^-3 (code: of 2^-1, scale: of 2^-2) of magnitude <= 18, a product a multiple of
    2^-6 of magnitude <= 324.  The sums of |products| of the cases below stay under 2^24 units of 2^-6 (asserted on the reference:
    the worst case 832 x 324 x 64 would not), so every partial sum in any order is representable in fp32.

The premises are asserted on the reference itself.  Shapes: (3841, 3072) -- 16 x 12 tiles of 256 x 256 whose last tile row holds ONE
row of the matrix: every staged row of it is clamped -- and (3072, 4100) -- ragged last tile column --, K = 64 a for a in {1, 2, 5, 13}
(prologue only, one loop iteration, odd step counts); (130, 304, 1088) takes the 128 x 256 tile with two K ranges (the second starts
at atom 9) and (48, 512, 1088) / (20, 512, 1088) the 64- and 32-row tiles, also split -- asserted through the split-K workspace the
boundary asks for; (200, 384, 1088) is served by the register-tiled kernel, which needs none, and is held to the same results.  Every case runs through ``matmul`` and through
``repack_w`` + ``matmul_rw``, one through ``matmul_silu_mul``; each output is written by 4 launches into NaN-filled tensors."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_parity import _torch_dequant

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAUNCHES = 4
BIG = [(3841, 3072), (3072, 4100)]
BIG_ATOMS = [1, 2, 5, 13]
SMALL = [(130, 304, 1088, 2), (48, 512, 1088, 2), (20, 512, 1088, 2), (200, 384, 1088, 0)]       # M, N, K, K ranges of the LDS-tiled kernel (0: another kernel)
FAMILIES = ["onehot_w", "onehot_x", "mantissa"]
MANTISSA_SCALES = [0x30, 0x34, 0x38, 0x3c, 0x40, 0x44]      # ue4m3 (e4m3, bias 7) codes of 0.5, 0.75, 1, 1.5, 2, 3
NONZERO_CODES = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]


def _dense(rows, K, g):
    return torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8)


def _one_hot(rows, K, g):
    """One non-zero e2m1 code per row at a random K position; every other nibble is +0 (0x0) or -0 (0x8)."""
    q = torch.randint(0, 2, (rows, K // 2), generator=g, dtype=torch.uint8) * 0x08 + torch.randint(0, 2, (rows, K // 2), generator=g, dtype=torch.uint8) * 0x80
    pos = torch.randint(0, K, (rows,), generator=g)
    code = torch.tensor(NONZERO_CODES, dtype=torch.uint8)[torch.randint(0, len(NONZERO_CODES), (rows,), generator=g)]
    r = torch.arange(rows)
    byte = q[r, pos // 2]
    hi = (pos % 2).to(torch.uint8)
    q[r, pos // 2] = torch.where(hi == 1, (byte & 0x0f) | (code << 4), (byte & 0xf0) | code)
    return q


@functools.lru_cache(maxsize=2)
def _problem(M, N, K, family):
    """Packed operands built directly and the fp64 product of their dequantised values (computed once per case, never modified)."""
    from arcquant_amd import agemm as ag
    g = torch.Generator().manual_seed(100003 * M + 101 * N + K + FAMILIES.index(family))

    def scales(rows):
        n = ag.sf_buffer_bytes(rows, K)
        if family == "mantissa":
            return torch.tensor(MANTISSA_SCALES, dtype=torch.uint8)[torch.randint(0, len(MANTISSA_SCALES), (n,), generator=g)]
        return torch.randint(0, 0x7f, (n,), generator=g, dtype=torch.uint8)        # every finite ue4m3 byte: 0x00 (zero) .. 0x7e (448)

    A = (_one_hot if family == "onehot_x" else _dense)(M, K, g)
    B = (_one_hot if family == "onehot_w" else _dense)(N, K, g)
    SFA, SFB = scales(M), scales(N)
    if family != "mantissa" and M * K >= 1 << 16 and N * K >= 1 << 16:             # every scale byte and every code on both operands
        for q, sf in ((A, SFA), (B, SFB)):
            assert torch.unique(sf).numel() == 127 and torch.unique(torch.cat([q & 0xf, q >> 4])).numel() == 16
    A, B, SFA, SFB = A.to(DEV), B.to(DEV), SFA.to(DEV), SFB.to(DEV)
    a64, b64 = _torch_dequant(A, SFA, K), _torch_dequant(B, SFB, K)
    want64 = a64 @ b64.T
    # the premises of exactness, checked on the operands themselves
    if family == "mantissa":
        want_abs = a64.abs() @ b64.abs().T
        assert float(want_abs.max()) * 64 < 2 ** 24 and bool((want64 * 64 == (want64 * 64).round()).all())
    else:
        hot = a64 if family == "onehot_x" else b64
        assert bool(((hot != 0).sum(dim=1) <= 1).all()), "at most one product per output (none where the code's scale byte is 0x00)"
    assert bool((want64.float().double() == want64).all())
    want32 = want64.float()
    return A, SFA, B, SFB, want32, want32.to(torch.bfloat16)


def _fresh(M, N, dtype):
    # an output no launch has written: every byte 0xff (NaN in fp32 and bf16)
    return torch.full((M, N), -1, dtype=torch.int8, device=DEV).repeat(1, dtype.itemsize).view(dtype)


def _launch_all(f, M, N, want32, want16, what):
    outs32 = [_fresh(M, N, torch.float32) for _ in range(LAUNCHES)]
    outs16 = [_fresh(M, N, torch.bfloat16) for _ in range(LAUNCHES)]
    for o32, o16 in zip(outs32, outs16):
        f(o32, torch.float32)
        f(o16, torch.bfloat16)
    for i, (o32, o16) in enumerate(zip(outs32, outs16)):
        bad32, bad16 = int((o32 != want32).sum()), int((o16 != want16).sum())
        print(f"    {what} launch {i}: fp32 mismatches {bad32}, bf16 mismatches {bad16}")
        assert torch.equal(o32, want32), (what, "fp32", i, bad32)
        assert torch.equal(o16, want16), (what, "bf16", i, bad16)


def _run(M, N, K, family, path):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, want32, want16 = _problem(M, N, K, family)
    if path == "matmul":
        _launch_all(lambda o, dt: ag.matmul(A, B, SFA, SFB, 1.0, out_dtype=dt, out=o), M, N, want32, want16, f"matmul {family} K={K}")
    else:
        RW, RSF = ag.repack_w(B, SFB)
        print(f"    matmul_rw route {ag.rw_route(M, N, K)}")
        _launch_all(lambda o, dt: ag.matmul_rw(A, RW, SFA, RSF, 1.0, N, out_dtype=dt, out=o), M, N, want32, want16, f"matmul_rw {family} K={K}")


@pytest.mark.parametrize("path", ["matmul", "matmul_rw"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("atoms", BIG_ATOMS)
@pytest.mark.parametrize("M,N", BIG)
def test_256_tiles_exact(M, N, atoms, family, path):
    from arcquant_amd import agemm as ag
    K = 64 * atoms
    if path == "matmul_rw":
        assert ag.rw_route(M, N, K) == 3, "the LDS-tiled kernel over the repacked weight serves these shapes"
    _run(M, N, K, family, path)


@pytest.mark.parametrize("path", ["matmul", "matmul_rw"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,K,splits", SMALL)
def test_small_tiles_split_k_exact(M, N, K, splits, family, path):
    from arcquant_amd import _lib
    # the LDS-tiled kernel with two K ranges: its split-K workspace is two fp32 partial outputs (the other kernels need none)
    assert int(_lib.lib().arcq_gemm_workspace_bytes(M, N, K)) == splits * M * N * 4
    _run(M, N, K, family, path)


def test_silu_mul_exact():
    """SiLU * up on the exact bf16 product: y = RNE(fp64 product), act = silu(y[:, 0::2]) * y[:, 1::2] with torch's ops (the order
    documented for matmul_silu_mul)."""
    from arcquant_amd import agemm as ag
    M, N = BIG[0]
    K = 64 * 5
    A, SFA, B, SFB, _, y = _problem(M, N, K, "mantissa")
    want = F.silu(y[:, 0::2]) * y[:, 1::2]
    for i in range(LAUNCHES):
        act, _slots = ag.matmul_silu_mul(A, B, SFA, SFB, 1.0)
        bad = int((act != want).sum())
        print(f"    silu * up K={K} launch {i}: mismatches {bad}")
        assert act.shape == (M, N // 2) and torch.equal(act, want), (i, bad)
