"""The overlapped tail of the 256 x 256 8-wave tile GEMM (arcquant_amd/csrc/gemm_tile_ot.hip: gemm_tile_ot_kernel) against the kernels
it stands in for (``-m gpu``).

The sibling multiplies the last K step of its range without staging another one, pair of row tiles by pair, and finishes and stores a
pair under the MFMAs of the next.  Every accumulator takes the same MFMAs in the same order and the epilogue's operations are the
interior epilogue's, so its output must EQUAL the kept kernel's bit for bit.  arcq_debug_set_tile_overlap_tail selects: 0 = never the
sibling, 1 = by the launcher's rule (launches of that tile made of whole tiles; not SiLU * up, whose sibling keeps its epilogue behind
the final step and is not the default), 2 = whenever legal: SiLU * up too, and every shape made of whole 256 x 256 tiles takes the
256 x 256 tile and with it the sibling.

Under 0 the small shapes below take the routes of the parent commit -- the register-tiled kernel or a smaller LDS tile, which sum K in
another order -- so their operands are built such that fp32 accumulation is EXACT in any order (tests/test_tile_kloop_gpu.py: random
e2m1 codes, scale bytes of {0.5, 1, 2, 4}, K <= 512), and per case
  (a) mode 2 == mode 0, torch.equal, into outputs pre-filled with NaN patterns;
  (b) both equal the fp64 product of the dequantised operands rounded once to bf16, then the documented order in torch ops for a
      bias, a residual and SiLU * up -- zero error, inside every bound of tests/test_gpu_parity.py;
  (c) with arbitrary finite scale bytes (inexact sums) the sibling is held to test_gemm_matches_oracle's bounds
      (tests/test_tile_epilogue_gpu._check_against_oracle).
One shape large enough for the 256 x 256 tile by the default rule (3072 x 4096: 192 tiles) compares mode 1 with mode 0 on inexact
sums: there both arms run that tile, the kept kernel and the sibling, and must still be equal.

Shapes: the smallest at which each new path can go wrong.  K = 64 a, a = 1 .. 5, on one tile: the final step alone, after one
unchanged step (second buffer), after a loop iteration (first buffer), after an iteration and a step, after two iterations.
512 x 768: six tiles through the XCD remap.  256 x 512 x 192 carries the operand cases, SiLU * up (N % 8 == 0; abs-max slots are one
per workgroup, so their number differs between the tiles of the two modes and their maximum is compared), the repacked weight and
the device scale.  M = 300 is not made of whole tiles: mode 2 must leave it to the kept kernels."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_parity import _torch_dequant
from tests.test_tile_epilogue_gpu import _add_bf16, _check_against_oracle
from tests.test_tile_kloop_gpu import POW2_SCALES
from tests.util import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEVER, BY_RULE, WHENEVER_LEGAL = 0, 1, 2
OPS = (256, 512, 192)                                # the shape of the operand, SiLU * up, repacked-weight and device-scale cases


@pytest.fixture(autouse=True)
def _restore_setter():
    from arcquant_amd import agemm as ag
    yield
    ag._debug_set_tile_overlap_tail(BY_RULE)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, scales="pow2"):
    """Packed operands built directly, the fp64 product of their dequantised values and of their magnitudes, a bias and a residual
    (computed once per case, never modified)."""
    from arcquant_amd import agemm as ag
    g = torch.Generator().manual_seed(100000 * M + 100 * N + K + (7 if scales == "any" else 0))

    def operand(rows):
        q = torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8)
        n = ag.sf_buffer_bytes(rows, K)
        if scales == "pow2":
            sf = torch.tensor(POW2_SCALES, dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]
        else:                                       # every finite ue4m3 byte; non-negative codes, so that the sums do not cancel
            q &= 0x77
            sf = torch.randint(0, 0x7f, (n,), generator=g, dtype=torch.uint8)
        return q.to(DEV), sf.to(DEV)

    A, SFA = operand(M)
    B, SFB = operand(N)
    a64, b64 = _torch_dequant(A, SFA, K), _torch_dequant(B, SFB, K)
    want64, want_abs = a64 @ b64.T, a64.abs() @ b64.abs().T
    if scales == "pow2":                            # the premises of exactness, checked on the operands themselves
        assert float(want_abs.max()) * 16 < 2 ** 24 and bool((want64 * 16 == (want64 * 16).round()).all())
    bias = (torch.randn(N, generator=g) * 64).to(torch.bfloat16).to(DEV)
    res = (torch.randn(M, N, generator=g) * 64).to(torch.bfloat16).to(DEV)
    return A, SFA, B, SFB, want64, want_abs, bias, res


def _fresh(M, N):
    # an output no launch has written: every byte 0xff (NaN in bf16)
    return torch.full((M, 2 * N), -1, dtype=torch.int8, device=DEV).view(torch.bfloat16)


def _arms(f, new_mode=WHENEVER_LEGAL):
    """f() with the sibling switched off, then on."""
    from arcquant_amd import agemm as ag
    ag._debug_set_tile_overlap_tail(NEVER)
    kept = f()
    ag._debug_set_tile_overlap_tail(new_mode)
    return kept, f()


def _same_bits(a, b):
    bad = int((bits(a) != bits(b)).sum())
    print(f"    elements that differ: {bad} of {a.numel()}")
    return bad == 0


def _plain_case(M, N, K):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, want64, _, _, _ = _problem(M, N, K)
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, 1.0, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    assert torch.equal(new, want64.float().to(torch.bfloat16))
    # inexact sums: the oracle's bounds (the fp32 result is the kept kernels': the sibling has no fp32 output)
    A, SFA, B, SFB, want64, want_abs, _, _ = _problem(M, N, K, "any")
    got16 = ag.matmul(A, B, SFA, SFB, 1.0, out=_fresh(M, N))
    _check_against_oracle(ag.matmul(A, B, SFA, SFB, 1.0, out_dtype=torch.float32), got16, want64, want_abs)


@pytest.mark.parametrize("atoms", [1, 2, 3, 4, 5])
def test_k_tails_on_one_tile(atoms):
    _plain_case(256, 256, 64 * atoms)


def test_several_tiles():
    _plain_case(512, 768, 192)


def test_whole_tile_shapes_take_the_tile_kernel_under_the_setter():
    from arcquant_amd import agemm as ag
    M, N, K = OPS
    ag._debug_set_tile_overlap_tail(NEVER)
    ragged = ag.rw_route(300, N, K)
    ag._debug_set_tile_overlap_tail(WHENEVER_LEGAL)
    assert ag.rw_route(M, N, K) == 3 and ag.rw_route(300, N, K) == ragged


@pytest.mark.parametrize("with_bias,with_res", [(True, False), (False, True), (True, True)])
def test_epilogue_operands(with_bias, with_res):
    from arcquant_amd import agemm as ag
    M, N, K = OPS
    A, SFA, B, SFB, want64, _, bias, res = _problem(M, N, K)
    kw = {"bias": bias if with_bias else None, "residual": res if with_res else None}
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, 1.0, out=_fresh(M, N), **kw))
    assert _same_bits(kept, new)
    y = want64.float().to(torch.bfloat16)
    if with_bias:
        y = _add_bf16(y, bias)
    if with_res:
        y = _add_bf16(y, res)
    assert torch.equal(new, y)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("repacked", [False, True])
def test_silu_mul(with_bias, repacked):
    from arcquant_amd import agemm as ag
    M, N, K = OPS
    A, SFA, B, SFB, want64, _, bias, _ = _problem(M, N, K)
    b_ = (bias.float() / 64).to(torch.bfloat16) if with_bias else None
    a_s = 2.0 ** -7                                 # a power of two (the scaled sums stay exact): activations of order 1 .. 10
    if repacked:
        RW, RSF = ag.repack_w(B, SFB)
        f = lambda: ag.matmul_rw_silu_mul(A, RW, SFA, RSF, a_s, N, bias=b_)
    else:
        f = lambda: ag.matmul_silu_mul(A, B, SFA, SFB, a_s, bias=b_)
    (act0, slots0), (act2, slots2) = _arms(f)
    assert act2.shape == (M, N // 2) and _same_bits(act0, act2)
    assert slots2.numel() == (M // 256) * (N // 256), "one abs-max slot per 256 x 256 tile"
    assert int(slots0.max().item()) == int(slots2.max().item()) == int(bits(act2.abs().max().reshape(1))[0])
    assert int(slots2.min().item()) > 0, "every workgroup writes its slot"
    y = (want64 * a_s).float().to(torch.bfloat16)
    if with_bias:
        y = _add_bf16(y, b_)
    assert torch.equal(act2, F.silu(y[:, 0::2]) * y[:, 1::2])


@pytest.mark.parametrize("M,N,K", [OPS, (256, 256, 128), (256, 256, 64)])
def test_repacked_weight_twin(M, N, K):
    from arcquant_amd import agemm as ag
    A, SFA, B, SFB, want64, _, bias, res = _problem(M, N, K)
    RW, RSF = ag.repack_w(B, SFB)
    kept, new = _arms(lambda: ag.matmul_rw(A, RW, SFA, RSF, 1.0, N, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    y = want64.float().to(torch.bfloat16)
    assert torch.equal(new, y)
    both0, both2 = _arms(lambda: ag.matmul_rw(A, RW, SFA, RSF, 1.0, N, bias=bias, residual=res, out=_fresh(M, N)))
    assert _same_bits(both0, both2)
    assert torch.equal(both2, _add_bf16(_add_bf16(y, bias), res))


def test_device_scale_present_and_absent():
    from arcquant_amd import agemm as ag
    M, N, K = OPS
    A, SFA, B, SFB, want64, _, _, _ = _problem(M, N, K)
    dev_scale = torch.tensor(0.25, dtype=torch.float32, device=DEV)
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, dev_scale, scale_host=0.5, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    assert torch.equal(new, (want64 * 0.125).float().to(torch.bfloat16))
    assert torch.equal(ag.matmul(A, B, SFA, SFB, 0.125), new)           # (mode 2 still: the host scale alone)


def test_a_launch_that_is_not_whole_tiles_keeps_its_kernel():
    from arcquant_amd import agemm as ag
    M, N, K = 300, 512, 192
    A, SFA, B, SFB, want64, _, bias, res = _problem(M, N, K)
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, 1.0, bias=bias, residual=res, out=_fresh(M, N)))
    assert _same_bits(kept, new)
    assert torch.equal(new, _add_bf16(_add_bf16(want64.float().to(torch.bfloat16), bias), res))


@pytest.mark.parametrize("K", [192, 256])
def test_kept_kernel_and_sibling_on_the_same_tile_with_inexact_sums(K):
    """192 tiles of 256 x 256: the default rule picks that tile in both modes, so mode 0 runs gemm_tile_kernel and mode 1 its sibling
    over the same operands in the same order -- equal bits on sums that are not exact, with every epilogue operand."""
    from arcquant_amd import agemm as ag
    M, N = 3072, 4096
    A, SFA, B, SFB, want64, want_abs, bias, res = _problem(M, N, K, "any")
    kept, new = _arms(lambda: ag.matmul(A, B, SFA, SFB, 2.0 ** -10, out=_fresh(M, N)), BY_RULE)
    assert _same_bits(kept, new)
    x32 = ag.matmul(A, B, SFA, SFB, 2.0 ** -10, out_dtype=torch.float32)
    _check_against_oracle(x32, new, want64 * 2.0 ** -10, want_abs * 2.0 ** -10)
    assert torch.equal(new, x32.to(torch.bfloat16))
    both0, both1 = _arms(lambda: ag.matmul(A, B, SFA, SFB, 2.0 ** -10, bias=bias, residual=res, out=_fresh(M, N)), BY_RULE)
    assert _same_bits(both0, both1)
    assert torch.equal(both1, _add_bf16(_add_bf16(x32.to(torch.bfloat16), bias), res))
    # (SiLU * up takes its sibling under 2 alone; the tile is the same in every mode here, so the slots compare one by one)
    (act0, slots0), (act2, slots2) = _arms(lambda: ag.matmul_silu_mul(A, B, SFA, SFB, 2.0 ** -22, bias=bias))
    assert _same_bits(act0, act2) and torch.equal(slots0, slots2)
