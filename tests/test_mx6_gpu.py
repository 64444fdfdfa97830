"""MXFP6 on the MI355X (``-m gpu``): the storage format against the scaled MFMA's e3m2 operand with exact data, the quantisers byte for
byte against tests/mx6_reference.py, arcq_gemm_mxfp6 (both weight formats, both kernels) element-wise against fp64 with a bound counted
from gemm_mx6.hip's chains of fp32 additions, and QLinearLayer(quant_type='MXFP6')."""
import numpy as np
import pytest
import torch

from arcquant_amd import agemm
from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
from tests import mx6_reference as R6
from tests import mx_reference as R
from tests.test_mx_gemm_exact_gpu import _assert_bf16_between
from tests.test_mx_gpu import deq_torch
from tests.util import bits, from_bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_M = 64                 # gemm_mx_common.hpp kMxSmallM: mx6_small_kernel up to here, mx6_tile_kernel above
ALPHA = 0.75
FORMATS = ["e3m2", "e2m1"]


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


# -------------------------------------------------------------------------------------------------------------- lane and bit map
@pytest.mark.parametrize("M", [16, 65])
@pytest.mark.parametrize("b_format", FORMATS)
def test_lane_and_bit_map_exact(M, b_format):
    """Operands built by pack6 / pack, not by the quantisers: random e3m2 codes of magnitude <= 3.5 (multiples of 1/16; every one of the
    six bits takes both values) under scale bytes 2^4 / 2^5 per (row, block), so every A value is an integer <= 112 -- and so is every
    e3m2 B value; an e2m1 B (multiples of 1/2 under 2^1 / 2^2) is an integer <= 24.  Every partial sum over Kp = 256 is an integer below
    256 * 112 * 112 < 2^22: exact in fp32 in any order, so the output equals the fp64 product of the dequantised operands.  A code read
    from another lane, block or bit position, or a scale byte from another block, is another integer."""
    N, Kp = 32, 256
    rng = np.random.default_rng(M + len(b_format))
    ca = (rng.integers(0, 20, (M, Kp)) | (rng.integers(0, 2, (M, Kp)) << 5)).astype(np.uint8)
    sa = rng.integers(131, 133, (M, Kp // 32)).astype(np.uint8)
    QA = R6.pack6(ca)
    if b_format == "e3m2":
        cb = (rng.integers(0, 20, (N, Kp)) | (rng.integers(0, 2, (N, Kp)) << 5)).astype(np.uint8)
        sb = rng.integers(131, 133, (N, Kp // 32)).astype(np.uint8)
        QB, b = R6.pack6(cb), R6.dequantize(R6.pack6(cb), sb)
    else:
        cb = rng.integers(0, 16, (N, Kp)).astype(np.uint8)
        sb = rng.integers(128, 130, (N, Kp // 32)).astype(np.uint8)
        QB, b = R.pack(cb), R.dequantize(R.pack(cb), sb)
    a = R6.dequantize(QA, sa)
    assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)) and (np.abs(a) @ np.abs(b).T).max() < 2 ** 24
    assert {int(c) & 31 for c in np.unique(ca)} == set(range(20)) and len(np.unique(a @ b.T)) > M * N // 2
    got = agemm.mx6_matmul(*_dev(QA, QB, sa, sb), 1.0, b_format=b_format, out_dtype=torch.float32)
    assert torch.equal(got.double().cpu(), torch.from_numpy(a @ b.T))


# -------------------------------------------------------------------------------------------------------------- quantisers
@pytest.mark.parametrize("rows,KQ,KE", [(3, 64, 0), (5, 128, 64), (17, 1088, 64), (16, 4096, 256), (2, 2112, 64)])
@pytest.mark.parametrize("is_x", [True, False], ids=["x", "w"])
def test_quantisers_byte_exact(rows, KQ, KE, is_x):
    """Q and SF byte-equal to the numpy reference, padding included (the outputs start as 0xA5), under a random reorder_index; the last
    row holds mx6_reference.EDGE_BLOCKS.  (16, 4096) splits each row over four workgroups, (2, 2112) over two of 33 blocks: the second starts at an odd block, 8-byte aligned only."""
    idx = random_perm(KQ, KQ + 7)
    X = outlier_activations(rows, KQ, rows + KQ) if is_x else (torch.randn(rows, KQ, generator=torch.Generator().manual_seed(KQ)) * 0.05).to(torch.bfloat16)
    X[-1] = from_bits(R6.edge_row(KQ, idx.numpy()))
    want_q, want_s = (R6.quantize_x if is_x else R6.quantize_w)(R.bf16_bits_to_f32(bits(X)), idx.numpy(), KE)
    Q, SF = (agemm.mx6_reorder_quantize_x if is_x else agemm.mx6_reorder_quantize_w)(X.to(DEV), idx.to(DEV), KE)
    assert Q.shape == want_q.shape and SF.shape == want_s.shape
    Q.fill_(0xA5), SF.fill_(0xA5)
    from arcquant_amd import _lib
    fn = _lib.lib().arcq_mx6_quantize_x if is_x else _lib.lib().arcq_mx6_quantize_w
    Xd, idxd = X.to(DEV), idx.to(DEV)
    _lib.check(fn(Xd.data_ptr(), idxd.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, torch.cuda.current_stream().cuda_stream), "mx6 quantise")
    assert np.array_equal(SF.cpu().numpy(), want_s), "scale bytes differ"
    assert np.array_equal(Q.cpu().numpy(), want_q), "codes differ"


# -------------------------------------------------------------------------------------------------------------- element-wise bound
_LUT6 = torch.from_numpy(R6.e3m2_value(np.arange(64)))


def deq6_torch(Q: torch.Tensor, SF: torch.Tensor) -> torch.Tensor:
    """fp64 dequantisation on the device: [rows, 3 Kp/4] + [rows, Kp/32] -> [rows, Kp] (four codes in every three bytes)."""
    t = Q.reshape(Q.shape[0], -1, 3).long()
    w = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    c = torch.stack([(w >> s) & 63 for s in (0, 6, 12, 18)], dim=-1).reshape(Q.shape[0], SF.shape[1], 32)
    return (_LUT6.to(Q.device)[c] * torch.exp2(SF.double() - 127)[..., None]).reshape(Q.shape[0], -1)


def gamma(M, Kp, b_format):
    """|got - ref| <= gamma * alpha * sum |a||b|.  The fp32 operations behind one output, counted in gemm_mx6.hip "Summation order":
    mx6_tile_kernel Kp / 64 accumulations and alpha; mx6_small_kernel ceil(Kp / 1024) accumulations in a wave, 7 additions over the
    waves and alpha; against an e3m2 weight every accumulation is two (A's large codes, then its small ones).  One unit roundoff 2^-24
    each, times 2 for the MFMA's own sum of a 64- or 128-term dot product of exact products (tests/test_mx_gemm_exact_gpu.py's margin)."""
    per = 2 if b_format == "e3m2" else 1
    n_add = per * (Kp // 64) + 1 if M > SMALL_M else per * -(-Kp // 1024) + 8
    return 2.0 * n_add * 2.0 ** -24


_ops = {}


def _operands(M, N, KQ, KE, b_format):
    """The quantisers' bytes for outlier activations and a randn * 0.05 weight, with fp64 alpha deq(A) deq(B)^T and alpha |deq A| |deq B|^T."""
    key = (M, N, KQ, KE, b_format)
    if key not in _ops:
        _ops.clear()
        w = (torch.randn(N, KQ, generator=torch.Generator().manual_seed(N + KQ)) * 0.05).to(torch.bfloat16).to(DEV)
        idx = random_perm(KQ, 3).to(DEV)
        QX, SX = agemm.mx6_reorder_quantize_x(outlier_activations(M, KQ, M + 5).to(DEV), idx, KE)
        QW, SW = (agemm.mx6_reorder_quantize_w if b_format == "e3m2" else agemm.mx_reorder_quantize_w)(w, idx, KE)
        a, b = deq6_torch(QX, SX), (deq6_torch if b_format == "e3m2" else deq_torch)(QW, SW)
        _ops[key] = (QX, QW, SX, SW, (ALPHA * (a @ b.T)).cpu().numpy(), (ALPHA * (a.abs() @ b.abs().T)).cpu().numpy())
    return _ops[key]


# one row; the edges of the small / tile split; a ragged tile in M and N; a 64-element K tail; one K step; long K
ELEMENTWISE = [(1, 16, 64, 0), (16, 144, 1088, 64), (17, 16, 1088, 64), (64, 144, 64, 0), (65, 144, 64, 0), (65, 16, 4096, 64),
               (129, 1024, 3584, 256), (300, 144, 1088, 64)]


@pytest.mark.parametrize("M,N,KQ,KE", ELEMENTWISE)
@pytest.mark.parametrize("b_format", FORMATS)
def test_gemm_elementwise(M, N, KQ, KE, b_format):
    """Every element of the fp32 output within gamma * wabs of fp64; no element is left out."""
    QX, QW, SX, SW, ref, wabs = _operands(M, N, KQ, KE, b_format)
    Kp = SX.shape[1] * 32
    assert Kp == R.k_padded(KQ + KE) and QX.shape[1] == 3 * Kp // 4 and np.all(wabs > 0)
    got = agemm.mx6_matmul(QX, QW, SX, SW, ALPHA, b_format=b_format, out_dtype=torch.float32).cpu().numpy().astype(np.float64)
    err, tol = np.abs(got - ref), gamma(M, Kp, b_format) * wabs
    print(f"mxfp6_elementwise {b_format} M={M} N={N} Kp={Kp} max_err_ulps={float((err / (2.0 ** -24 * wabs)).max()):.3f} bound_ulps={gamma(M, Kp, b_format) * 2 ** 24:.0f}")
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, f"{len(bad)} of {err.size} outside; first D{tuple(bad[0])}: {got[tuple(bad[0])]!r} against {ref[tuple(bad[0])]!r}"


@pytest.mark.parametrize("M,N,KQ,KE", [(16, 144, 1088, 64), (300, 144, 1088, 64)])
@pytest.mark.parametrize("b_format", FORMATS)
def test_gemm_epilogue(M, N, KQ, KE, b_format):
    """bias and a residual that aliases D on the bf16 output: the kernel rounds bf16(alpha acc), + bias -> bf16, + residual -> bf16, every
    step monotone, so the stored bits lie between the same chain applied to the two ends of the element's interval."""
    QX, QW, SX, SW, ref, wabs = _operands(M, N, KQ, KE, b_format)
    tol = gamma(M, SX.shape[1] * 32, b_format) * wabs
    g = torch.Generator().manual_seed(M)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    res = (torch.randn(M, N, generator=g) * 4).to(torch.bfloat16)
    bf, rf = R.bf16_bits_to_f32(bits(bias))[None, :], R.bf16_bits_to_f32(bits(res))

    def chain(end):
        y = R.bf16_round(R.bf16_bits_to_f32(R.bf16_rne_bits(end)) + bf)
        return (R.bf16_round(y + rf).view(np.uint32) >> 16).astype(np.uint16)

    D = res.to(DEV)
    got = agemm.mx6_matmul(QX, QW, SX, SW, ALPHA, b_format=b_format, bias=bias.to(DEV), residual=D, out=D)
    assert got.data_ptr() == D.data_ptr()
    _assert_bf16_between(bits(got), chain(ref - tol), chain(ref + tol), "bias + residual in place")


# -------------------------------------------------------------------------------------------------------------- layer
@pytest.mark.parametrize("M", [3, 70])
@pytest.mark.parametrize("mx6_weight", FORMATS)
def test_qlinear_mxfp6(M, mx6_weight):
    """The layer's forward is mx6_matmul on its own operands bit for bit, and its bf16 output lies between the roundings of the ends of
    test_gemm_elementwise's interval."""
    torch.manual_seed(M)
    KQ, N, KE = 128, 48, 64
    lin = torch.nn.Linear(KQ, N, bias=True).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 5).to(DEV)
    layer = QLinearLayer(lin, KE, idx, quant_type="MXFP6", mx6_weight=mx6_weight)
    assert layer.W.shape == (N, 256 * 3 // 4 if mx6_weight == "e3m2" else 128)
    qx, sx, scale = reorder_quantize_x(outlier_activations(M, KQ, 6).to(DEV), idx, KE, quant_type="MXFP6")
    assert scale.dim() == 0 and scale.item() == 1.0
    y = layer((qx, sx, scale, 1, M))
    assert y.shape == (1, M, N) and y.dtype == torch.bfloat16
    assert torch.equal(y[0], agemm.mx6_matmul(qx, layer.W, sx, layer.scale_w, 1.0, b_format=mx6_weight, bias=lin.bias))
    a, b = deq6_torch(qx, sx), (deq6_torch if mx6_weight == "e3m2" else deq_torch)(layer.W, layer.scale_w)
    ref, tol = (a @ b.T).cpu().numpy(), gamma(M, 256, mx6_weight) * (a.abs() @ b.abs().T).cpu().numpy()
    bf = R.bf16_bits_to_f32(bits(lin.bias))[None, :]
    chain = lambda end: (R.bf16_round(R.bf16_bits_to_f32(R.bf16_rne_bits(end)) + bf).view(np.uint32) >> 16).astype(np.uint16)   # noqa: E731
    _assert_bf16_between(bits(y[0]), chain(ref - tol), chain(ref + tol), "layer")
