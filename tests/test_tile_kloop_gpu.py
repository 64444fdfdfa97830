"""The K loop of the 256 x 256 8-wave tile GEMM (arcquant_amd/csrc/gemm_tile_body.inc, k_step_pipe) on EXACT sums (``-m gpu``).

The loop keeps two LDS buffers and one barrier per K step; fragments of the next step are read behind that barrier while the current
step is still being multiplied.  A fragment read that runs ahead of the barrier that publishes it, or a staging write that lands in a
buffer still being read, yields a wrong product in a few lanes of a few launches -- which a tolerance would absorb.  So the operands
here are built directly (random e2m1 code bytes, scale bytes in the swizzled layout of tests/test_gpu_parity._torch_dequant; no
quantiser) such that fp32 accumulation is exact in ANY order:

  * scale bytes are the ue4m3 codes of {0.5, 1, 2, 4}, alpha = 1;
  * every product a sa b sb is then a multiple of 2^-4 (codes are multiples of 0.5, scales of 0.5) of magnitude <= 6 * 4 * 6 * 4 = 576;
  * over K <= 512 every partial sum is below 512 * 576 * 16 = 4.7 * 10^6 < 2^24 units of 2^-4: representable in fp32.

The fp32 output must EQUAL the fp64 matmul of the dequantised operands bit for bit and the bf16 output its round-to-nearest-even
rounding, on each of 8 launches into outputs pre-filled with NaN patterns.

Shapes (M, N) = (4096, 3072) -- 16 x 12 = 192 tiles, all interior -- and (3900, 3332) -- 16 x 14 = 224 tiles with edge tiles in the last
tile row and column, N % 4 == 0: both take gemm_tile_kernel<256, 256, 2, 4, ...> by default (>= 192 tiles of 256 x 256, and M N K above
what the register-tiled kernel is given).  K = 64 a for a in {1, 2, 3, 4, 5, 8}: the prologue alone with the single (tail) step, one
loop iteration, odd and even step counts; the boundary accepts every one of them (K % 64 == 0).
a = 3 and a = 8 run again through matmul_silu_mul (N % 8 == 0: the first shape only) and through repack_w + matmul_rw (both shapes;
route 3, the LDS-tiled kernel over the repacked weight), and one case at a = 5 has arbitrary valid ue4m3 scale bytes (and non-negative codes:
its sums are inexact in fp32 and must not cancel for a bound relative to the result) and is held to the bounds of
tests/test_tile_epilogue_gpu._check_against_oracle.  Split-K and the smaller tiles are covered by the parity files run
under tools/scripts/tile_cfg_tests.sh."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_parity import _torch_dequant
from tests.test_tile_epilogue_gpu import _check_against_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(4096, 3072), (3900, 3332)]
ATOMS = [1, 2, 3, 4, 5, 8]
LAUNCHES = 8
POW2_SCALES = [0x30, 0x38, 0x40, 0x48]          # ue4m3 (e4m3, bias 7) codes of 0.5, 1, 2, 4


@functools.lru_cache(maxsize=2)
def _problem(M, N, K, scales):
    """Packed operands built directly, and the fp64 product of their dequantised values (computed once per case, never modified)."""
    from arcquant_amd import agemm as ag
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + (7 if scales == "any" else 0))

    def operand(rows):
        q = torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8)
        if scales == "any":
            # non-negative codes: with scales over 2^-9 .. 448 the products span 2^36 and an fp32 sum is no longer exact, so the bf16
            # bound of _check_against_oracle (one ulp of the RESULT) can only be asked of sums that do not cancel
            q &= 0x77
        n = ag.sf_buffer_bytes(rows, K)
        if scales == "pow2":
            sf = torch.tensor(POW2_SCALES, dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]
        else:                                   # every finite ue4m3 byte: 0x00 (zero) .. 0x7e (448); 0x7f is NaN, the sign bit is not a scale's
            sf = torch.randint(0, 0x7f, (n,), generator=g, dtype=torch.uint8)
        return q.to(DEV), sf.to(DEV)

    A, SFA = operand(M)
    B, SFB = operand(N)
    a64, b64 = _torch_dequant(A, SFA, K), _torch_dequant(B, SFB, K)
    want64 = a64 @ b64.T
    want_abs = a64.abs() @ b64.abs().T
    if scales == "pow2":                        # the premises of exactness, checked on the operands themselves
        assert float(want_abs.max()) * 16 < 2 ** 24 and bool((want64 * 16 == (want64 * 16).round()).all())
        assert bool((want64.float().double() == want64).all())
    return A, SFA, B, SFB, want64, want_abs


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


@pytest.mark.parametrize("atoms", ATOMS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_exact_sums(M, N, atoms):
    from arcquant_amd import agemm as ag
    K = 64 * atoms
    A, SFA, B, SFB, want64, _ = _problem(M, N, K, "pow2")
    want32 = want64.float()
    _launch_all(lambda o, dt: ag.matmul(A, B, SFA, SFB, 1.0, out_dtype=dt, out=o), M, N, want32, want32.to(torch.bfloat16), f"matmul K={K}")


@pytest.mark.parametrize("atoms", [3, 8])
@pytest.mark.parametrize("M,N", SHAPES)
def test_exact_sums_repacked_weight(M, N, atoms):
    from arcquant_amd import agemm as ag
    K = 64 * atoms
    assert ag.rw_route(M, N, K) == 3, "the LDS-tiled kernel over the repacked weight serves these shapes"
    A, SFA, B, SFB, want64, _ = _problem(M, N, K, "pow2")
    RW, RSF = ag.repack_w(B, SFB)
    want32 = want64.float()
    _launch_all(lambda o, dt: ag.matmul_rw(A, RW, SFA, RSF, 1.0, N, out_dtype=dt, out=o), M, N, want32, want32.to(torch.bfloat16),
                f"matmul_rw K={K}")


@pytest.mark.parametrize("atoms", [3, 8])
def test_exact_sums_silu_mul(atoms):
    """SiLU * up on the exact bf16 product: y = RNE(fp64 product), act = silu(y[:, 0::2]) * y[:, 1::2] with torch's ops (the order
    documented for matmul_silu_mul); (3900, 3332) has N % 8 != 0, which the epilogue refuses."""
    from arcquant_amd import agemm as ag
    M, N = SHAPES[0]
    K = 64 * atoms
    A, SFA, B, SFB, want64, _ = _problem(M, N, K, "pow2")
    y = want64.float().to(torch.bfloat16)
    want = F.silu(y[:, 0::2]) * y[:, 1::2]
    for i in range(LAUNCHES):
        act, _slots = ag.matmul_silu_mul(A, B, SFA, SFB, 1.0)
        bad = int((act != want).sum())
        print(f"    silu * up K={K} launch {i}: mismatches {bad}")
        assert act.shape == (M, N // 2) and torch.equal(act, want), (i, bad)


def test_arbitrary_scales_within_oracle_bounds():
    from arcquant_amd import agemm as ag
    M, N = SHAPES[1]
    K = 64 * 5
    A, SFA, B, SFB, want64, want_abs = _problem(M, N, K, "any")
    got32 = ag.matmul(A, B, SFA, SFB, 1.0, out_dtype=torch.float32)
    got16 = ag.matmul(A, B, SFA, SFB, 1.0)
    _check_against_oracle(got32, got16, want64, want_abs)
