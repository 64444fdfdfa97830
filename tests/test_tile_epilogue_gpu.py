"""The tile GEMM's epilogues (arcquant_amd/csrc/gemm_tile_body.inc) on shapes that take its straight-line interior-tile path, its general
path, or both in one launch (``-m gpu``).

Which kernel each shape runs BY DEFAULT (tile_choice / the dispatch of c_api.hip; seen in a kernel trace of this file):
  (4096, 4096)  gemm_tile_kernel<256, 256, 2, 4, ...>: 256 tiles, every one interior
  (4000, 4100)  the same kernel, 16 x 17 tiles: interior tiles and edge tiles (last tile row and column) in one launch, N % 4 == 0
  (4000, 4104)  the same; N % 8 == 0, so the SiLU * up epilogue (which needs it) also sees interior and edge tiles in one launch
  (2050, 4098)  gemm_tile_kernel<128, 128, 2, 2, ...>: N % 4 != 0, never on the interior path (scalar stores)
  (128, 1024), (512, 1028)  gemm_regtile by default; under ARCQ_REGTILE_CFG=-1 with ARCQ_TILE_CFG = 1, 7 or 10 the 128 x 128, 64 x 256 and
                128 x 256 tiles with split-K (fp32 partials: never the interior path) -- the overrides are read once per process,
                so this file is run once per value (one pytest process each); under them the large shapes run those tiles unsplit.
KQ = 4096 and 3584, KE = 64.  Cases: plain, bias, residual, both, both as misaligned (2-byte-offset) views, fp32 output, SiLU * up.

Asserted for every case:
 (a) the oracle tolerance of tests/test_gpu_parity.py::test_gemm_matches_oracle for the same call, against an fp64 matmul of the
     dequantised operands (torch on the GPU, the independent format statement validated there): fp32 output within 2e-6 of
     sum |a b|, 1e-3 relative norm-wise and element-wise away from cancellation; bf16 output within one bf16 ulp of the oracle's
     rounding and equal to it on more than 99 % of the elements (the calls with operands are held to what
     test_gemm_epilogue_operands_on_every_kernel holds them to: equality with the torch ops on the plain result, which is (b));
 (b) BIT EQUALITY with a result that never takes the interior path: the same product launched with out_dtype = float32 and no
     operand (fp32 alpha * acc), then the documented order with torch ops -- y = x32.to(bf16); with a bias
     y = (y.float() + bias.float()).to(bf16); with a residual the same again.  torch's fp32 -> bf16 is round-to-nearest-even, so
     this also checks the hardware conversion of the interior path against an independent rounding."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_parity import _max_bf16_ulp_diff, _torch_dequant
from tests.util import bits, outlier_activations, prescale, random_perm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KE = 64
SHAPES = [(4096, 4096), (4000, 4100), (4000, 4104), (2050, 4098), (128, 1024), (512, 1028)]


def _add_bf16(y, t):
    return (y.float() + t.float()).to(torch.bfloat16)


def _check_against_oracle(got32, got16, want64, want_abs):
    err = (got32.double() - want64).abs()
    assert bool((err <= 2e-6 * want_abs + 1e-30).all()), float((err / (want_abs + 1e-30)).max())
    assert float((got32.double() - want64).norm()) <= 1e-3 * float(want64.norm())
    big = want64.abs() > 1e-2 * want_abs
    assert bool((err[big] <= 1e-3 * want64.abs()[big]).all())
    want16 = bits(want64.float().to(torch.bfloat16))
    g16 = bits(got16)
    ulp, same = _max_bf16_ulp_diff(g16, want16), float((g16 == want16).mean())
    print(f"    bf16 vs oracle: max ulp {ulp}, equal {same:.5f}")
    assert ulp <= 1
    assert same > 0.99


@pytest.mark.parametrize("KQ", [4096, 3584])
@pytest.mark.parametrize("M,N", SHAPES)
def test_tile_epilogue_cases(M, N, KQ):
    from arcquant_amd import agemm as ag
    K = KQ + KE
    x, sx = prescale(outlier_activations(M, KQ, 11 + M))
    w, sw = prescale((torch.rand(N, KQ, generator=torch.Generator().manual_seed(N + KQ)) * 3 - 1.0).to(torch.bfloat16))
    idx = random_perm(KQ, 12).to(DEV)
    A, SFA = ag.reorder_quantize_x(x.to(DEV), idx, KE)
    B, SFB = ag.reorder_quantize_w(w.to(DEV), idx, KE)
    alpha = float(sx * sw)
    g = torch.Generator().manual_seed(M + N)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)

    a64, b64 = _torch_dequant(A, SFA, K), _torch_dequant(B, SFB, K)
    want64 = alpha * (a64 @ b64.T)
    want_abs = alpha * (a64.abs() @ b64.abs().T)
    del a64, b64

    # the reference result of (b): fp32 alpha * acc, no operand -- the general epilogue on every tile
    x32 = ag.matmul(A, B, SFA, SFB, alpha, out_dtype=torch.float32)
    y_plain = x32.to(torch.bfloat16)

    # plain (host scale and device scale)
    got = ag.matmul(A, B, SFA, SFB, alpha)
    _check_against_oracle(x32, got, want64, want_abs)
    assert torch.equal(got, y_plain), "plain"
    dev_scale = torch.tensor(alpha / 0.5, dtype=torch.float32, device=DEV)
    assert torch.equal(ag.matmul(A, B, SFA, SFB, dev_scale, scale_host=0.5), y_plain), "plain, device scale"

    # bias, residual, both
    y_bias = _add_bf16(y_plain, bias)
    y_res = _add_bf16(y_plain, res)
    y_both = _add_bf16(y_bias, res)
    assert torch.equal(ag.matmul(A, B, SFA, SFB, alpha, bias=bias), y_bias), "bias"
    assert torch.equal(ag.matmul(A, B, SFA, SFB, alpha, residual=res), y_res), "residual"
    got_both = ag.matmul(A, B, SFA, SFB, dev_scale, scale_host=0.5, bias=bias, residual=res)
    assert torch.equal(got_both, y_both), "bias + residual"

    # misaligned views: the 8-byte operand loads (and the interior path) are refused, element loads give the same bits
    bias_off = torch.empty(N + 1, dtype=torch.bfloat16, device=DEV)[1:]
    res_off = torch.empty(M * N + 1, dtype=torch.bfloat16, device=DEV)[1:].view(M, N)
    bias_off.copy_(bias)
    res_off.copy_(res)
    assert bias_off.data_ptr() % 8 == 2 and res_off.data_ptr() % 8 == 2
    assert torch.equal(ag.matmul(A, B, SFA, SFB, alpha, bias=bias_off, residual=res_off), y_both), "misaligned views"
    assert torch.equal(ag.matmul(A, B, SFA, SFB, alpha, bias=bias_off), y_bias), "misaligned bias"

    # fp32 output with operands: added in fp32, one result (never the interior path)
    got32 = ag.matmul(A, B, SFA, SFB, alpha, out_dtype=torch.float32, bias=bias, residual=res)
    assert torch.equal(got32, (x32 + bias.float()) + res.float()), "fp32 out"

    # SiLU * up on row-interleaved gate / up weights (N % 8 == 0): activations of order 1..10
    if N % 8 == 0:
        a_s = alpha * 40.0
        xs32 = ag.matmul(A, B, SFA, SFB, a_s, out_dtype=torch.float32)
        for b_ in (None, bias):
            y = xs32.to(torch.bfloat16)
            if b_ is not None:
                y = _add_bf16(y, b_)
            want = F.silu(y[:, 0::2]) * y[:, 1::2]
            act, slots = ag.matmul_silu_mul(A, B, SFA, SFB, a_s, bias=b_)
            assert act.shape == (M, N // 2) and torch.equal(act, want), ("silu * up", b_ is not None)
            if M > 512:                            # the tile kernel: one abs-max slot per workgroup, every one written
                assert int(slots.max().item()) == int(bits(want.abs().max().reshape(1))[0]), "abs-max slots"
