"""The quad-load sibling of the 256 x 256 8-wave tile GEMM (arcquant_amd/csrc/gemm_tile_ql.hip: gemm_tile_ql_kernel) against the paired-load
kernel it stands in for and the overlapped-tail kernel both derive from (``-m gpu``).

The sibling's loop iteration is four K steps: step 0 requests the code bytes of A's FOUR following K atoms of a row back to back, step 2
B's, steps 1 and 3 only scale bytes; the 1 - 3 steps left between the loop and the final step request A's next atom alone.  The staged
bytes, the LDS image, the K order, every MFMA and the epilogue are the overlapped-tail kernel's, so the three kernels must give the SAME
bits.  Arms: ``ot`` = arcq_debug_set_tile_pair_loads(0) (gemm_tile_ot_kernel, which tests/test_tile_overlap_tail_gpu.py ties to the
oracle), ``pl`` = pair loads 1 and arcq_debug_set_tile_quad_loads(0) (gemm_tile_pl_kernel), ``ql`` = both 1 (the default).
arcq_debug_set_tile_overlap_tail(2) sends every shape made of whole 256 x 256 tiles to that tile, so the small shapes below run the
kernels under test.

Shapes: (256, 256) one tile, (512, 256) and (256, 512) two of them along either axis.  K = 64 a, by what the quad kernel does with a
atoms (the prologue requests A's atoms 0, 1 and B's 0 .. 3, every index clamped to a - 1):
  a = 1  the final step alone;                 a = 2, 3, 4  no loop iteration and 1, 2, 3 single steps ahead of the final step;
  a = 5  one iteration, nothing left: A's quad 2 .. 5 has its last atom clamped, B's 4 .. 7 its last three;
  a = 6, 7  one iteration and 1, 2 steps left: B's quad clamped from its third / fourth atom;
  a = 9  two iterations: in the second A's quad 6 .. 9 is clamped in its last atom and B's 8 .. 11 in three;
  a = 10  two iterations and one step left: A's second quad whole, B's clamped from its third atom.
Bias, residual and both at a = 9.  One case (a = 9) runs with every operand at the very end of a poisoned allocation (tests/arena.py):
a load past the clamped atom of the last row would read the poison and change the result; nothing there waits for a fault.

Inputs: those of tests/test_tile_pair_loads_gpu.py (outlier activations and weights quantised by the oracle, one row of zeroed scale
bytes and one ue4m3-subnormal scale byte per operand); the plain cases are also held to test_gemm_matches_oracle's bounds against the
oracle's fp64 product (tests/test_tile_epilogue_gpu._check_against_oracle)."""
import pytest
import torch

from tests.test_tile_epilogue_gpu import _check_against_oracle
from tests.test_tile_pair_loads_gpu import SHAPES, _fresh, _problem, _same_bits

pytestmark = pytest.mark.gpu

K_AUGS = [64 * a for a in (1, 2, 3, 4, 5, 6, 7, 9, 10)]
K_OPS = 64 * 9
assert SHAPES == [(256, 256), (512, 256), (256, 512)]


@pytest.fixture(autouse=True)
def _setters():
    from arcquant_amd import agemm as ag
    ag._debug_set_tile_overlap_tail(2)
    yield
    ag._debug_set_tile_overlap_tail(1)
    ag._debug_set_tile_pair_loads(1)
    ag._debug_set_tile_quad_loads(1)


def _arms(f):
    """f() through gemm_tile_ot_kernel, through gemm_tile_pl_kernel and through the quad-load sibling."""
    from arcquant_amd import agemm as ag
    ag._debug_set_tile_pair_loads(0)
    ot = f()
    ag._debug_set_tile_pair_loads(1)
    ag._debug_set_tile_quad_loads(0)
    pl = f()
    ag._debug_set_tile_quad_loads(1)
    return ot, pl, f()


@pytest.mark.parametrize("K", K_AUGS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_plain_equals_both_kept_kernels_and_meets_the_oracle(M, N, K):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, alpha, want, want_abs, _, _ = _problem(M, N, K)
    ot, pl, ql = _arms(lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N)))
    assert _same_bits(ot, pl)
    assert _same_bits(ot, ql)
    _check_against_oracle(ag.matmul(A, B, SFA, SFB, alpha, out_dtype=torch.float32), ql, want, want_abs)


@pytest.mark.parametrize("with_bias,with_res", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N", SHAPES)
def test_epilogue_operands_equal_both_kept_kernels(M, N, with_bias, with_res):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, alpha, _, _, bias, res = _problem(M, N, K_OPS)
    kw = {"bias": bias if with_bias else None, "residual": res if with_res else None}
    ot, pl, ql = _arms(lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N), **kw))
    assert _same_bits(ot, pl)
    assert _same_bits(ot, ql)
    assert not torch.equal(ql, ag.matmul(A, B, SFA, SFB, alpha)), "the epilogue operands took no part"


def test_the_setter_is_inert_while_pair_loads_are_off():
    """Pair-loads mode 0 means gemm_tile_ot_kernel, whatever the new setter says (the existing pair-load tests keep comparing the kept
    kernel with the default route): same bits with the new setter at 1 and at 0; and with the overlapped tail off altogether."""
    from arcquant_amd import agemm as ag
    M, N, K = 256, 512, K_OPS
    A, SFA, B, SFB, alpha, _, _, _, _ = _problem(M, N, K)
    f = lambda: ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N))
    for tail in (2, 0):
        ag._debug_set_tile_overlap_tail(tail)
        ag._debug_set_tile_pair_loads(0)
        ag._debug_set_tile_quad_loads(1)
        on = f()
        ag._debug_set_tile_quad_loads(0)
        assert _same_bits(on, f())
        ag._debug_set_tile_pair_loads(1)


def test_repacked_weight_keeps_the_paired_load_kernel():
    """Launches over the repacked weight are not routed to the quad kernel (reference layout only): same bits either way, and the
    reference layout's."""
    from arcquant_amd import agemm as ag
    M, N, K = 256, 256, K_OPS
    A, SFA, B, SFB, alpha, _, _, _, _ = _problem(M, N, K)
    RW, RSF = ag.repack_w(B, SFB)
    ot, pl, ql = _arms(lambda: ag.matmul_rw(A, RW, SFA, RSF, alpha, N, out=_fresh(M, N)))
    assert _same_bits(ot, pl)
    assert _same_bits(ot, ql)
    assert _same_bits(ql, ag.matmul(A, B, SFA, SFB, alpha, out=_fresh(M, N)))


def test_operands_at_the_end_of_their_allocations():
    """arcq_gemm_nvfp4 on (256, 512) x 576 through the quad kernel, every operand between poisoned guards with its last byte followed at
    once by the tail guard, under three poisons: the output must equal the tight run's byte for byte and no guard byte may change."""
    from tests.test_arena_nvfp4_gpu import _run_gemm
    _run_gemm("nvfp4", 256, 512, K_OPS)
    _run_gemm("nvfp4", 256, 512, K_OPS, epi=True)
