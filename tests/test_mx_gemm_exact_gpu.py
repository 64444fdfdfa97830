"""arcq_gemm_mxfp4, the anchor every fused MXFP4 test ends at, against fp64 on the MI355X: exact sums at every K split and tile edge
of both kernels, E8M0 scale bytes at the two ends of the range, and an element-wise error bound on the quantisers' own output that is
derived from the kernels' chains of fp32 additions (DESIGN.md 3.6 "How the plain GEMM is checked")."""
import json
import math

import numpy as np
import pytest
import torch

from arcquant_amd import agemm
from tests import mx_reference as R
from tests.test_mx_gpu import _exact_gemm_f32, _report, deq_torch
from tests.util import bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_M = 64                 # gemm_mx.hip kMxSmallM: mx_small_kernel up to here, mx_tile_kernel above

# ------------------------------------------------------------------------------------------------------------ exact sums
# codes of 0, 0.5, 1, -0.5, -1, -0: with exponents 0..2 a product is a multiple of 2^-2 of magnitude <= 16, so the sum over
# Kp = 8192 stays under 2^17 granules.  The budget is 2^20 granules, the magnitude at which test_dense_exact (512 full-alphabet
# products, <= 36 * 16 each, granule 2^-2) already holds on the hardware; nothing larger has been shown exact inside the MFMA.
ALPHABET = np.array([0, 1, 2, 9, 10, 8], dtype=np.uint8)
EXACT_GRANULES = 2.0 ** 20

LONG_K = [
    # mx_small_kernel: wave w takes steps w, w + 8, w + 16, w + 24 of a round of 32
    (1, 16, 128),        # one step, seven idle waves
    (15, 48, 1152),      # nine steps: wave 0 takes two, the others one
    (16, 32, 4096),      # exactly one full round: every wave and every unroll slot
    (17, 32, 4224),      # 33 steps: the second round is wave 0 with slots 1..3 clamped and skipped; second row block, 15 clamped rows
    (33, 48, 5120),      # 40 steps: every wave runs slot 0 only in the second round
    (64, 16, 8192),      # two full rounds, the last M of this kernel
    # mx_tile_kernel
    (65, 16, 128),       # one step, the first M of this kernel: 63 A rows and 112 B rows clamped
    (65, 144, 384),      # three steps (an odd buffer turnover), tiles ragged in both directions
    (129, 128, 4224),    # 33 steps, two row tiles
    (257, 272, 8192),    # 64 steps, a 3 x 3 tile grid
]


def _alphabet_operands(M, N, Kp, seed, a_bytes, b_bytes):
    rng = np.random.default_rng(seed)
    QA = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (M, Kp))])
    QB = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (N, Kp))])
    sa = rng.choice(np.asarray(a_bytes, dtype=np.uint8), (M, Kp // 32))
    sb = rng.choice(np.asarray(b_bytes, dtype=np.uint8), (N, Kp // 32))
    return QA, QB, sa, sb


def _assert_exact(QA, QB, sa, sb):
    """The CPU side first: the data cannot round in fp32 in any summation order, B is not symmetric, and the outputs take many values."""
    want = R.gemm(QA, QB, sa, sb)
    unit = 0.25 * 2.0 ** (int(sa.min()) - 127 + int(sb.min()) - 127)
    granules = R.abs_gemm(QA, QB, sa, sb).max() / unit
    assert granules <= EXACT_GRANULES, f"sum |a||b| reaches 2^{math.log2(granules):.1f} granules"
    assert np.array_equal(np.rint(want / unit) * unit, want)
    assert len(np.unique(QB, axis=0)) == QB.shape[0] and len(np.unique(QB.T, axis=0)) > QB.shape[1] // 2
    assert len(np.unique(want)) >= min(want.size, 512) // 2, f"only {len(np.unique(want))} distinct outputs"
    got = _exact_gemm_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


@pytest.mark.parametrize("M,N,Kp", LONG_K)
def test_long_k_exact(M, N, Kp):
    """Random codes of {0, +-0.5, +-1}, exponents 0..2 per (row, block), fp32 output, alpha = 1: bit-equal to the fp64 sum at the
    smallest shape that reaches each K split of mx_small_kernel and each tile edge / buffer turnover of mx_tile_kernel."""
    _assert_exact(*_alphabet_operands(M, N, Kp, 7 * M + 3 * N + Kp, (127, 128, 129), (127, 128, 129)))


@pytest.mark.parametrize("M,N,Kp", [(16, 32, 4224), (130, 144, 4224)])
def test_lane_map_exact_over_long_k(M, N, Kp):
    """test_lane_map_exact's construction -- one nonzero code per A row, so each output is ONE exact product -- with the nonzero
    position spread over all 33 K steps: kpos = (37 m + 5 + 37 M pass) mod Kp.  A pass holds M positions; where M rows cannot reach
    every step in one launch (M = 16) further passes shift the window, and the passes together must land in every step."""
    rng = np.random.default_rng(M * 131 + N * 7 + Kp)
    steps = Kp // 128
    passes = -(-Kp // (37 * M))
    cb = ((np.arange(N)[:, None] * 5 + np.arange(Kp)[None, :] * 3 + (np.arange(N)[:, None] * np.arange(Kp)[None, :]) % 7) % 16).astype(np.uint8)
    sa = (127 + (np.arange(M)[:, None] + 3 * np.arange(Kp // 32)[None, :]) % 7 - 3).astype(np.uint8)
    sb = (127 + (2 * np.arange(N)[:, None] + np.arange(Kp // 32)[None, :]) % 5 - 2).astype(np.uint8)
    QB = R.pack(cb)
    kpos = [(np.arange(M) * 37 + 5 + 37 * M * p) % Kp for p in range(passes)]
    assert set(np.concatenate(kpos) // 128) == set(range(steps)), "some K step holds no row's nonzero"
    if M >= steps:
        assert passes == 1
    for kp in kpos:
        ca = np.zeros((M, Kp), dtype=np.uint8)
        ca[np.arange(M), kp] = rng.integers(1, 16, M).astype(np.uint8) | 1
        QA = R.pack(ca)
        want = R.gemm(QA, QB, sa, sb)
        assert np.count_nonzero(want) > want.size // 2
        got = _exact_gemm_f32(QA, QB, sa, sb)
        assert np.array_equal(got, want), _report(got, want)


@pytest.mark.parametrize("low_side", ["A", "B"])
@pytest.mark.parametrize("M,N,Kp", [(16, 32, 512), (65, 144, 384)])
def test_extreme_scale_bytes_exact(M, N, Kp, low_side):
    """include/arcq.h: byte b means 2^(b - 127) for every b the quantisers can write.  One operand's bytes from {0..3}, the other's from
    {250..254}: each product is a code product times 2^(-4..+3), so the sums are far inside fp32's normal range and only the decoding of
    the bytes is under test.  255 is outside the contract."""
    lo, hi = (0, 1, 2, 3), (250, 251, 252, 253, 254)
    QA, QB, sa, sb = _alphabet_operands(M, N, Kp, M + N + Kp, lo if low_side == "A" else hi, hi if low_side == "A" else lo)
    assert {int(sa.min()), int(sb.min())} == {0, 250} and {int(sa.max()), int(sb.max())} == {3, 254}
    _assert_exact(QA, QB, sa, sb)


# ------------------------------------------------------------------------------------------------------------ element-wise bound
ALPHA = 0.75


def n_add(M, Kp):
    """fp32 additions (and the alpha multiply) behind one output, counted in gemm_mx.hip.  mx_tile_kernel: two 32x32x64 accumulations per
    128-step, then alpha.  mx_small_kernel: a wave accumulates ceil(steps / 8) MFMA results, seven LDS adds join the eight waves, then
    alpha."""
    return Kp // 64 + 1 if M > SMALL_M else -(-Kp // 1024) + 8


def gamma(M, Kp):
    """|got - ref| <= gamma * alpha * sum |a||b|: one unit roundoff 2^-24 per operation of n_add, times 2 as margin for the MFMA's own
    summation of a 64- or 128-term dot product of exact products (its internal precision is not documented)."""
    return 2.0 * n_add(M, Kp) * 2.0 ** -24


# every M, N and (KQ, KE) of the issue's grid; both kernels see (3584, 256) (Kp = 3840) and (4096, 64) (Kp = 4224, a 64-element tail)
ELEMENTWISE = [
    (1, 1024, 4096, 64), (16, 144, 3584, 256), (17, 16, 1088, 64), (64, 144, 64, 0), (64, 1024, 4096, 64),
    (65, 16, 4096, 64), (65, 144, 64, 0), (129, 1024, 3584, 256), (300, 144, 1088, 64), (300, 1024, 4096, 64),
]
_ops = {}


def _operands(M, N, KQ, KE):
    """(QX, QW, SX, SW, ref, wabs, sum_bits): the quantisers' bytes, on the host in fp64 alpha * deq(X) . deq(W)^T and
    alpha * |deq X| . |deq W|^T, and how many bits the exact result needs: every product of output (m, n) is a multiple of the granule
    0.25 * 2^(min e_a[m] + min e_b[n]) and alpha = 3/4, so alpha * (any partial sum) is an integer below 3 * sum |a||b| / granule in
    units of a quarter granule; sum_bits = log2 of the largest such count."""
    key = (M, N, KQ, KE)
    if key not in _ops:
        _ops.clear()
        g = torch.Generator().manual_seed(N + KQ)
        w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
        idx = random_perm(KQ, 3).to(DEV)
        QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE)
        QX, SX = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, M + 5).to(DEV), idx, KE)
        a, b = deq_torch(QX, SX), deq_torch(QW, SW)
        ref, wabs = ALPHA * (a @ b.T), ALPHA * (a.abs() @ b.abs().T)
        granule = 0.25 * torch.exp2(SX.min(dim=1).values.double() - 127)[:, None] * torch.exp2(SW.min(dim=1).values.double() - 127)[None, :]
        sum_bits = math.log2(float((3.0 * (wabs / ALPHA) / granule).max()))
        _ops[key] = (QX, QW, SX, SW, ref.cpu().numpy(), wabs.cpu().numpy(), sum_bits)
    return _ops[key]


def _assert_bf16_between(got_bits, lo_bits, hi_bits, what):
    k, klo, khi = R.bf16_key(got_bits), R.bf16_key(lo_bits), R.bf16_key(hi_bits)
    assert np.all(klo <= khi)
    bad = np.argwhere((k < klo) | (k > khi))
    assert len(bad) == 0, f"{what}: {len(bad)} of {k.size} outside; first D{tuple(bad[0])} bits {got_bits[tuple(bad[0])]:#06x} not in " \
                          f"[{lo_bits[tuple(bad[0])]:#06x}, {hi_bits[tuple(bad[0])]:#06x}]"


@pytest.mark.parametrize("M,N,KQ,KE", ELEMENTWISE)
def test_gemm_elementwise(M, N, KQ, KE):
    """Every element of the fp32 output within gamma * wabs of fp64, every element of the bf16 output between the RNE of the interval's
    ends, on the real quantisers' output for outlier activations; alpha = 0.75 from the host and, at one shape per kernel, from the
    device.  One wrong code or scale byte in one 32-block moves an element by about wabs / Kp, some 60 (tile) to 150 (small) gamma at
    Kp = 4224.  Largest |err| / (2^-24 wabs) seen on an MI355X: profiles/mxfp4_gemm_elementwise.json (tools/mx_elementwise_profile.py
    collates the lines printed here).  Those ratios are 0.0, and the assertion on sum_bits is why: on this data alpha times every partial
    sum fits fp32's 24 bits, so no operation of the chain rounds.  If other data breaks that assertion the bound below still stands, but
    the recorded ratios and DESIGN.md's account of them no longer describe the test."""
    QX, QW, SX, SW, ref, wabs, sum_bits = _operands(M, N, KQ, KE)
    Kp = QX.shape[1] * 2
    assert Kp == R.k_padded(KQ + KE) and np.all(wabs > 0)
    assert sum_bits < 24, f"alpha * sum |a||b| reaches 2^{sum_bits:.2f} quarter granules: fp32 additions can round on this data"
    tol = gamma(M, Kp) * wabs
    lo_bits, hi_bits = R.bf16_rne_bits(ref - tol), R.bf16_rne_bits(ref + tol)
    scales = [dict(scale=ALPHA)]
    if (M, N) in ((16, 144), (129, 1024)):
        scales.append(dict(scale=torch.tensor(0.5, dtype=torch.float32, device=DEV), scale_host=1.5))
    for kw in scales:
        got = agemm.mx_matmul(QX, QW, SX, SW, out_dtype=torch.float32, **kw).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)
        ratio = float((err / (2.0 ** -24 * wabs)).max())
        print("mxfp4_elementwise " + json.dumps({"kernel": "tile" if M > SMALL_M else "small", "M": M, "N": N, "Kp": Kp, "n_add": n_add(M, Kp),
                                                "bound_ulps": 2 * n_add(M, Kp), "max_err_ulps": round(ratio, 3), "sum_bits": round(sum_bits, 2),
                                                "alpha": "device" if "scale_host" in kw else "host"}))
        bad = np.argwhere(err > tol)
        assert len(bad) == 0, f"{len(bad)} of {err.size} outside; worst {ratio:.2f} x 2^-24 wabs against {2 * n_add(M, Kp)}; first D{tuple(bad[0])}"
        _assert_bf16_between(bits(agemm.mx_matmul(QX, QW, SX, SW, **kw)), lo_bits, hi_bits, f"bf16 {sorted(kw)}")


def _f32_of(b):
    return R.bf16_bits_to_f32(b)


@pytest.mark.parametrize("M,N,KQ,KE", [(16, 144, 3584, 256), (129, 1024, 3584, 256)])
def test_gemm_elementwise_epilogue(M, N, KQ, KE):
    """bias and residual on the bf16 output with fp64 as the truth: the kernel rounds bf16(alpha acc), + bias -> bf16, + residual -> bf16
    (arcq_gemm_nvfp4's order; each sum in fp32), every step is monotone, so the stored bits lie between the same chain applied to the two
    ends of the element's interval."""
    QX, QW, SX, SW, ref, wabs, _ = _operands(M, N, KQ, KE)
    tol = gamma(M, QX.shape[1] * 2) * wabs
    g = torch.Generator().manual_seed(M)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    res = (torch.randn(M, N, generator=g) * 4).to(torch.bfloat16)
    bf, rf = _f32_of(bits(bias))[None, :], _f32_of(bits(res))

    def chain(end):
        y = _f32_of(R.bf16_rne_bits(end))
        y = R.bf16_round(y + bf)                   # float32 + float32: the kernel's fp32 sum, then its bf16 rounding
        return (R.bf16_round(y + rf).view(np.uint32) >> 16).astype(np.uint16)

    got = agemm.mx_matmul(QX, QW, SX, SW, ALPHA, bias=bias.to(DEV), residual=res.to(DEV))
    _assert_bf16_between(bits(got), chain(ref - tol), chain(ref + tol), "bias + residual")
