"""The paired-load sibling of the 256 x 256 8-wave tile GEMM (arcquant_amd/csrc/gemm_tile_pl.hip: gemm_tile_pl_kernel) against the
overlapped-tail kernel it stands in for (``-m gpu``).

The sibling requests the code bytes of TWO K atoms per row back to back in every even K step and nothing in the odd one; the
staged bytes, the LDS image, the K order, every MFMA and the epilogue are the overlapped-tail kernel's, so its output must EQUAL that
kernel's bit for bit.  arcq_debug_set_tile_pair_loads selects: 1 (the default) = launches that are eligible for the overlapped tail
with the plain epilogue take the sibling, 0 = they take gemm_tile_ot_kernel, which tests/test_tile_overlap_tail_gpu.py and the parity
tests tie to the oracle.  arcq_debug_set_tile_overlap_tail(2) sends every shape made of whole 256 x 256 tiles to that tile, so that the
small shapes below run the kernel under test; under 0 the new setter must change nothing.

Shapes: (256, 256) one tile, (512, 256) and (256, 512) two of them along either axis (the second tile's descriptors start inside the
operand).  K = 64 a for a = 1, 2, 3, 4, 5, 7 atoms: the final step alone; one unchanged step and no loop iteration; one iteration whose
second atom is clamped (a = 3); an iteration and the step behind it (a = 4); two iterations, the second clamped (a = 5); three
iterations, the last clamped (a = 7).  Bias, residual and both at a = 5; the repacked weight at (256, 256) and a = 5.

Inputs: activations with the outlier recipe and weights of tests/test_gpu_parity._make_operands, quantised by the oracle; then per
operand every scale byte of one row set to 0 and one scale byte of another row set to a ue4m3 subnormal.  The plain cases are also held
to test_gemm_matches_oracle's bounds against the oracle's fp64 product (tests/test_tile_epilogue_gpu._check_against_oracle)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.test_gpu_parity import _make_operands
from tests.test_tile_epilogue_gpu import _check_against_oracle
from tests.util import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(256, 256), (512, 256), (256, 512)]
K_AUGS = [64, 128, 192, 256, 320, 448]
K_OPS = 320
ZERO_ROW, SUBNORMAL_ROW, SUBNORMAL_BYTE = 37, 201, 0x03      # (rows of the first tile; the second group of 16 of the subnormal's row)


@pytest.fixture(autouse=True)
def _setters():
    from arcquant_amd import agemm as ag
    ag._debug_set_tile_overlap_tail(2)
    yield
    ag._debug_set_tile_overlap_tail(1)
    ag._debug_set_tile_pair_loads(1)


def _sf_offsets(row, K):
    # the scale bytes of one row: 512 bytes per block of 128 rows and atom of 64 K (tests/test_gpu_parity._torch_dequant)
    p = np.arange(K // 16)
    return ((row // 128) * (K // 64) + p // 4) * 512 + (row % 32) * 16 + ((row // 32) % 4) * 4 + p % 4


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """Operands on the GPU, the oracle's fp64 product and product of magnitudes, a bias and a residual (built once, never modified)."""
    KE = 64 if K > 64 else 0
    qx, sfx, qw, sfw, alpha = _make_operands(M, N, K - KE, KE, O.G16, 7000 + M + N + K)
    for sf in (sfx, sfw):
        sf[_sf_offsets(ZERO_ROW, K)] = 0
        sf[_sf_offsets(SUBNORMAL_ROW, K)[min(1, K // 16 - 1)]] = SUBNORMAL_BYTE
    _, want, want_abs = O.gemm(qx, qw, sfx, sfw, alpha, want_abs=True)
    assert not want[ZERO_ROW].any() and not want[:, ZERO_ROW].any() and want[SUBNORMAL_ROW].any()
    g = torch.Generator().manual_seed(M + N + K)
    amp = float(np.abs(want).mean())
    bias = (torch.randn(N, generator=g) * amp).to(torch.bfloat16).to(DEV)
    res = (torch.randn(M, N, generator=g) * amp).to(torch.bfloat16).to(DEV)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return dev(qx), dev(sfx), dev(qw), dev(sfw), alpha, torch.from_numpy(want).to(DEV), torch.from_numpy(want_abs).to(DEV), bias, res


def _fresh(M, N):
    # an output no launch has written: every byte 0xff (NaN in bf16)
    return torch.full((M, 2 * N), -1, dtype=torch.int8, device=DEV).view(torch.bfloat16)


def _arms(f):
    """f() through gemm_tile_ot_kernel, then through the paired-load sibling."""
    from arcquant_amd import agemm as ag
    ag._debug_set_tile_pair_loads(0)
    kept = f()
    ag._debug_set_tile_pair_loads(1)
    return kept, f()


def _same_bits(a, b):
    bad = int((bits(a) != bits(b)).sum())
    print(f"    elements that differ: {bad} of {a.numel()}")
    return bad == 0 and torch.equal(a, b)


@pytest.mark.parametrize("K", K_AUGS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_plain_equals_the_kept_kernel_and_meets_the_oracle(M, N, K):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, alpha, want, want_abs, _, _ = _problem(M, N, K)
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    _check_against_oracle(ag.matmul(A, B, SFA, SFB, alpha, out_dtype=torch.float32), new, want, want_abs)


@pytest.mark.parametrize("with_bias,with_res", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N", SHAPES)
def test_epilogue_operands_equal_the_kept_kernel(M, N, with_bias, with_res):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, alpha, _, _, bias, res = _problem(M, N, K_OPS)
    kw = {"bias": bias if with_bias else None, "residual": res if with_res else None}
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N), **kw))
    assert _same_bits(kept, new)
    assert not torch.equal(new, ag.matmul(A, B, SFA, SFB, alpha)), "the epilogue operands took no part"


def test_repacked_weight_equals_the_kept_kernel_and_the_reference_layout():
    from arcquant_amd import agemm as ag
    M, N, K = 256, 256, K_OPS
    A, SFA, B, SFB, alpha, _, _, bias, res = _problem(M, N, K)
    RW, RSF = ag.repack_w(B, SFB)
    kept, new = _arms(lambda: ag.matmul_rw(A, RW, SFA, RSF, alpha, N, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    assert _same_bits(new, ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N)))
    both0, both1 = _arms(lambda: ag.matmul_rw(A, RW, SFA, RSF, alpha, N, bias=bias, residual=res, out=_fresh(M, N)))
    assert _same_bits(both0, both1)


def test_the_setter_changes_nothing_while_the_overlapped_tail_is_off():
    """Mode 0 of arcq_debug_set_tile_overlap_tail means the kept kernel, whatever the new setter says: the shape keeps the route it has
    under 0 and gives the same bits with the new setter at 1 and at 0."""
    from arcquant_amd import agemm as ag
    M, N, K = 256, 512, K_OPS
    A, SFA, B, SFB, alpha, _, _, _, _ = _problem(M, N, K)
    ag._debug_set_tile_overlap_tail(0)
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N)))
    assert _same_bits(kept, new)
