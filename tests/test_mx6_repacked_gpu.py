"""arcq_gemm_mxfp6_repacked on the MI355X (``-m gpu``): the layout MRW6 and the MRSF bytes against the MFMA's lanes with exact integer
data, both weight formats element-wise against fp64 with tests/test_mx6_gpu.py's bound (gemm_mx6_rw.hip has mx6_small_kernel's count of
fp32 additions), the epilogue, and QLinearLayer(quant_type='MXFP6', mx6_repack_for_decode=True)."""
import functools

import numpy as np
import pytest
import torch

from arcquant_amd import agemm
from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
from tests import mx6_reference as R6
from tests import mx_reference as R
from tests.test_mx6_gpu import ALPHA, DEV, FORMATS, _dev, _operands, gamma
from tests.test_mx_gemm_exact_gpu import _assert_bf16_between
from tests.util import bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu


def _repack(QW, SW, b_format):
    return (agemm.mx6_repack_w if b_format == "e3m2" else agemm.mx_repack_w)(QW, SW)


@functools.lru_cache(maxsize=None)
def _exact(Kp, b_format):
    """test_lane_and_bit_map_exact's construction for 64 x 32 outputs: integer-valued operands (e3m2 codes of magnitude <= 3.5 under scale
    bytes 2^4 / 2^5, e2m1 codes under 2^1 / 2^2) whose every partial sum is an integer below 2^24 (asserted), so fp32 is exact in any order."""
    N, rng = 32, np.random.default_rng(Kp + len(b_format))
    ca = (rng.integers(0, 20, (64, Kp)) | (rng.integers(0, 2, (64, Kp)) << 5)).astype(np.uint8)
    sa = rng.integers(131, 133, (64, Kp // 32)).astype(np.uint8)
    if b_format == "e3m2":
        cb = (rng.integers(0, 20, (N, Kp)) | (rng.integers(0, 2, (N, Kp)) << 5)).astype(np.uint8)
        QB, sb = R6.pack6(cb), rng.integers(131, 133, (N, Kp // 32)).astype(np.uint8)
        b = R6.dequantize(QB, sb)
    else:
        QB, sb = R.pack(rng.integers(0, 16, (N, Kp)).astype(np.uint8)), rng.integers(128, 130, (N, Kp // 32)).astype(np.uint8)
        b = R.dequantize(QB, sb)
    QA = R6.pack6(ca)
    a = R6.dequantize(QA, sa)
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)) and (np.abs(a) @ np.abs(b).T).max() < 2 ** 24
    QAd, QBd, sad, sbd = _dev(QA, QB, sa, sb)
    return QAd, sad, _repack(QBd, sbd, b_format), torch.from_numpy(a @ b.T)


@pytest.mark.parametrize("Kp", [128, 1152, 4224])          # one step; 9: only wave 0 takes a second; 33: a second, partial MRSF round
@pytest.mark.parametrize("M", [1, 16, 17, 64])
@pytest.mark.parametrize("b_format", FORMATS)
def test_lane_and_bit_map_exact(M, Kp, b_format):
    """A byte of MRW6 or MRSF read by another lane, step or wave, a row clamped wrongly or a padding scale byte multiplied is another integer."""
    QA, sa, (MRW, MRSF), want = _exact(Kp, b_format)
    got = agemm.mx6_matmul_repacked(QA[:M].contiguous(), MRW, sa[:M].contiguous(), MRSF, 1.0, 32, b_format=b_format, out_dtype=torch.float32)
    assert torch.equal(got.double().cpu(), want[:M])


@pytest.mark.parametrize("M,N,KQ,KE", [(1, 16, 64, 0), (16, 144, 1088, 64), (17, 16, 1088, 64), (48, 144, 1088, 64), (64, 144, 4096, 64)])
@pytest.mark.parametrize("b_format", FORMATS)
def test_gemm_elementwise(M, N, KQ, KE, b_format):
    """Every element of the fp32 output within gamma * wabs of fp64 on the quantisers' bytes for outlier activations (the data that
    exposed the MFMA's 14-bit cut: a missing split fails here); an e2m1 weight is bit for bit mx6_matmul."""
    QX, QW, SX, SW, ref, wabs = _operands(M, N, KQ, KE, b_format)
    Kp = SX.shape[1] * 32
    MRW, MRSF = _repack(QW, SW, b_format)
    got = agemm.mx6_matmul_repacked(QX, MRW, SX, MRSF, ALPHA, N, b_format=b_format, out_dtype=torch.float32)
    err, tol = np.abs(got.cpu().numpy().astype(np.float64) - ref), gamma(M, Kp, b_format) * wabs
    print(f"mxfp6_repacked_elementwise {b_format} M={M} N={N} Kp={Kp} max_err_ulps={float((err / (2.0 ** -24 * wabs)).max()):.3f} bound_ulps={gamma(M, Kp, b_format) * 2 ** 24:.0f}")
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, f"{len(bad)} of {err.size} outside; first D{tuple(bad[0])}: {got[tuple(bad[0])]!r} against {ref[tuple(bad[0])]!r}"
    if b_format == "e2m1":
        assert torch.equal(got, agemm.mx6_matmul(QX, QW, SX, SW, ALPHA, b_format=b_format, out_dtype=torch.float32))


@pytest.mark.parametrize("b_format", FORMATS)
def test_gemm_epilogue(b_format):
    """bias and a residual that aliases D on the bf16 output: between the roundings of the ends of the element's interval
    (tests/test_mx6_gpu.py::test_gemm_epilogue's chain)."""
    M, N = 17, 144
    QX, QW, SX, SW, ref, wabs = _operands(M, N, 1088, 64, b_format)
    tol = gamma(M, SX.shape[1] * 32, b_format) * wabs
    g = torch.Generator().manual_seed(M)
    bias, res = torch.randn(N, generator=g).to(torch.bfloat16), (torch.randn(M, N, generator=g) * 4).to(torch.bfloat16)
    bf, rf = R.bf16_bits_to_f32(bits(bias))[None, :], R.bf16_bits_to_f32(bits(res))

    def chain(end):
        y = R.bf16_round(R.bf16_bits_to_f32(R.bf16_rne_bits(end)) + bf)
        return (R.bf16_round(y + rf).view(np.uint32) >> 16).astype(np.uint16)

    D = res.to(DEV)
    MRW, MRSF = _repack(QW, SW, b_format)
    got = agemm.mx6_matmul_repacked(QX, MRW, SX, MRSF, ALPHA, N, b_format=b_format, bias=bias.to(DEV), residual=D, out=D)
    assert got.data_ptr() == D.data_ptr()
    _assert_bf16_between(bits(got), chain(ref - tol), chain(ref + tol), "bias + residual in place")


@pytest.mark.parametrize("mx6_weight", FORMATS)
def test_qlinear_mx6_repack_for_decode(mx6_weight):
    """At most MX6_REPACKED_MAX_M tokens: mx6_matmul_repacked on the layer's operands, bit for bit; above: mx6_matmul."""
    torch.manual_seed(3)
    KQ, N, KE = 128, 48, 64
    lin = torch.nn.Linear(KQ, N, bias=True).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 5).to(DEV)
    layer = QLinearLayer(lin, KE, idx, quant_type="MXFP6", mx6_weight=mx6_weight, mx6_repack_for_decode=True)
    assert layer.MRW.numel() == layer.W.numel() and agemm.MX6_REPACKED_MAX_M >= 3
    for M in (3, 70):
        qx, sx, scale = reorder_quantize_x(outlier_activations(M, KQ, 6).to(DEV), idx, KE, quant_type="MXFP6")
        y = layer((qx, sx, scale, 1, M))[0]
        if M == 3:
            assert torch.equal(y, agemm.mx6_matmul_repacked(qx, layer.MRW, sx, layer.MRSF, 1.0, N, b_format=mx6_weight, bias=lin.bias))
        else:
            assert torch.equal(y, agemm.mx6_matmul(qx, layer.W, sx, layer.scale_w, 1.0, b_format=mx6_weight, bias=lin.bias))
