"""MXFP4 on the MI355X: the quantisers' bytes against tests/mx_reference.py (special values included), the operand / scale lane
map of the block-scaled fp4 MFMA pinned with exact integer data, the GEMM's accuracy against an fp64 dequantised product, the
epilogue's roundings, the extension module against the ctypes mirror, and QLinearLayer(quant_type='MXFP4')."""
import os

import numpy as np
import pytest
import torch

from arcquant_amd import _build_ext, _lib, agemm
from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
from tests import mx_reference as R
from tests.util import bits, from_bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _f32(x_bf16: torch.Tensor) -> np.ndarray:
    return R.bf16_bits_to_f32(bits(x_bf16))


def _inputs(rows, KQ, seed, kind="x"):
    if kind == "x":
        return outlier_activations(rows, KQ, seed)
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, KQ, generator=g) * 0.02).to(torch.bfloat16)


def _quantize_poisoned(is_x, X, idx, KE, poison):
    rows, KQ = X.shape
    Kp = R.k_padded(KQ + KE)
    Q = torch.full((rows, Kp // 2), poison, dtype=torch.uint8, device=DEV)
    SF = torch.full((rows, Kp // 32), poison, dtype=torch.uint8, device=DEV)
    L = _lib.lib()
    fn = L.arcq_mx_quantize_x if is_x else L.arcq_mx_quantize_w
    _lib.check(fn(X.data_ptr(), idx.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, None), "mx quantise")
    torch.cuda.synchronize()
    return Q.cpu().numpy(), SF.cpu().numpy()


PAIRS = [(KQ, KE) for KQ in (64, 3584, 4096, 18944) for KE in (0, 64, 256) if KE <= KQ]


@pytest.mark.parametrize("M", [1, 3, 130, 4096])
@pytest.mark.parametrize("KQ,KE", PAIRS)
@pytest.mark.parametrize("perm", ["identity", "random"])
@pytest.mark.parametrize("is_x", [True, False], ids=["x", "w"])
def test_quantiser_bytes_equal_reference(M, KQ, KE, perm, is_x):
    X = _inputs(M, KQ, 1000 + M + KQ + KE, "x" if is_x else "w")
    idx = torch.arange(KQ, dtype=torch.int16) if perm == "identity" else random_perm(KQ, KQ + 7)
    Xd, idxd = X.to(DEV), idx.to(DEV)
    Q0, S0 = _quantize_poisoned(is_x, Xd, idxd, KE, 0x00)
    Q1, S1 = _quantize_poisoned(is_x, Xd, idxd, KE, 0xFF)
    assert np.array_equal(Q0, Q1) and np.array_equal(S0, S1), "some output byte is not written"
    rows = np.arange(M) if M * KQ <= 4096 * 4096 else np.unique(np.r_[np.arange(0, M, 61), M - 1])
    wq, ws = (R.quantize_x if is_x else R.quantize_w)(_f32(X)[rows], idx.numpy().astype(np.int64), KE)
    assert np.array_equal(S0[rows], ws), "scale bytes differ"
    assert np.array_equal(Q0[rows], wq), "codes differ"
    # the mirror allocates and returns the same bytes
    Qm, Sm = (agemm.mx_reorder_quantize_x if is_x else agemm.mx_reorder_quantize_w)(Xd, idxd, KE)
    assert np.array_equal(Qm.cpu().numpy(), Q0) and np.array_equal(Sm.cpu().numpy(), S0)


@pytest.mark.parametrize("perm", ["identity", "random"])
@pytest.mark.parametrize("KE", [0, 64, "KQ"])
@pytest.mark.parametrize("KQ", [128, 4096])
def test_quantiser_special_values_byte_exact(KQ, KE, perm):
    """R.special_value_rows through arcq_mx_quantize_x / _w: zero and -0.0 blocks, bf16 subnormals (the exponent clamp at -127), the
    smallest normals, the largest finite values, amax on and one ulp above the exponent rule's boundaries, the e2m1 ties, and subnormal
    blocks beside ordinary ones -- each kind also inside the outlier tail, where the residual block is quantised too.  The reference
    runs first (its residual-exact and no-saturation assertions hold on this input); Inf and NaN are outside the contract."""
    KE = KQ if KE == "KQ" else KE
    idx = torch.arange(KQ, dtype=torch.int16) if perm == "identity" else random_perm(KQ, KQ + 7)
    idxn = idx.numpy().astype(np.int64)
    Xb = R.special_value_rows(KQ, idxn, KQ + KE)
    xf = R.bf16_bits_to_f32(Xb)
    want = {True: R.quantize_x(xf, idxn, KE), False: R.quantize_w(xf, idxn, KE)}
    wq, ws = want[True]
    B, P = KQ // 32, (KQ - KE) // 32
    assert {0, 126, 127, 128, 253} <= set(np.unique(ws[:, :B]))
    assert np.all(ws[:2] == 127) and np.all(R.unpack(wq[0]) == 0) and np.all(R.unpack(wq[1, :KQ // 2]) == 8)
    if KE:
        mag = Xb[:, idxn].reshape(8, B, 32)[:, P:] & 0x7FFF             # the tail of the reordered rows, whatever the permutation
        assert np.all((mag[2] >= 1) & (mag[2] <= 0x7F)) and np.all(mag[4].max(axis=-1) == 0x7F7F)
        assert {0x4041, 0x40C1} <= set(mag[5][:, 0]) and np.any(mag[7].max(axis=-1) <= 0x7F) and np.any(mag[7].min(axis=-1) >= 0x3F80)
        rs, rq = ws[:, B:B + KE // 32], R.unpack(wq[:, KQ // 2:(KQ + KE) // 2])
        # a subnormal's residual is at most a quarter of the clamped block's code step: it rounds to zero and leaves its sign in the code
        assert len(np.unique(rs)) >= 5 and all((rq[r] & 7).any() for r in (3, 4, 5, 7)) and set(np.unique(rq[2])) == {0, 8}, \
            "the tail's residual blocks are not exercised"
    Xd, idxd = from_bits(Xb).to(DEV), idx.to(DEV)
    for is_x in (True, False):
        Q0, S0 = _quantize_poisoned(is_x, Xd, idxd, KE, 0x00)
        Q1, S1 = _quantize_poisoned(is_x, Xd, idxd, KE, 0xFF)
        assert np.array_equal(Q0, Q1) and np.array_equal(S0, S1), "some output byte is not written"
        for r, name in enumerate(R.SPECIAL_ROWS):
            who = f"{'x' if is_x else 'w'} row {r} ({name})"
            bad = np.flatnonzero(S0[r] != want[is_x][1][r])
            assert len(bad) == 0, f"{who}: scale bytes differ at blocks {bad[:8]}: got {S0[r][bad[:8]]} want {want[is_x][1][r][bad[:8]]}"
            bad = np.flatnonzero(Q0[r] != want[is_x][0][r])
            assert len(bad) == 0, f"{who}: codes differ at bytes {bad[:8]}: got {Q0[r][bad[:8]]} want {want[is_x][0][r][bad[:8]]}"


# -------------------------------------------------------------------------------------------------------------- lane map
def _exact_gemm_f32(QA, QB, SA, SB):
    A, B, SFA, SFB = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (QA, QB, SA, SB))
    D = agemm.mx_matmul(A, B, SFA, SFB, 1.0, out_dtype=torch.float32)
    torch.cuda.synchronize()
    return D.cpu().numpy().astype(np.float64)


def _report(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {got.size} differ; first: " + ", ".join(f"D{tuple(b)} got {got[tuple(b)]!r} want {want[tuple(b)]!r}" for b in bad[:6])


@pytest.mark.parametrize("M,N,Kp", [(16, 32, 256), (5, 48, 384), (64, 64, 128), (256, 256, 256), (200, 144, 384)])
def test_lane_map_exact(M, N, Kp):
    """One nonzero code per A row (at a row-dependent K position), an asymmetric B, scale exponents that differ per (row, block):
    each output is ONE exact product, so a swapped row / column, a mis-ordered K element or a mis-mapped scale byte shows up as
    an exactly wrong value (another code, or another power of two)."""
    rng = np.random.default_rng(M * 131 + N * 7 + Kp)
    ca = np.zeros((M, Kp), dtype=np.uint8)
    kpos = (np.arange(M) * 37 + 5) % Kp
    ca[np.arange(M), kpos] = rng.integers(1, 16, M).astype(np.uint8) | 1           # nonzero magnitude, both signs
    cb = ((np.arange(N)[:, None] * 5 + np.arange(Kp)[None, :] * 3 + (np.arange(N)[:, None] * np.arange(Kp)[None, :]) % 7) % 16).astype(np.uint8)
    sa = (127 + (np.arange(M)[:, None] + 3 * np.arange(Kp // 32)[None, :]) % 7 - 3).astype(np.uint8)
    sb = (127 + (2 * np.arange(N)[:, None] + np.arange(Kp // 32)[None, :]) % 5 - 2).astype(np.uint8)
    QA, QB = R.pack(ca), R.pack(cb)
    want = R.gemm(QA, QB, sa, sb)
    got = _exact_gemm_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


@pytest.mark.parametrize("M,N,Kp", [(16, 64, 512), (64, 128, 256), (256, 256, 512), (129, 176, 384)])
def test_dense_exact(M, N, Kp):
    """Random codes everywhere, exponents 0..2 per (row, block): every partial sum is a multiple of 2^-2 below 2^20, exact in fp32."""
    rng = np.random.default_rng(M + N + Kp)
    QA = rng.integers(0, 256, (M, Kp // 2), dtype=np.uint8)
    QB = rng.integers(0, 256, (N, Kp // 2), dtype=np.uint8)
    sa = rng.integers(127, 130, (M, Kp // 32), dtype=np.uint8)
    sb = rng.integers(127, 130, (N, Kp // 32), dtype=np.uint8)
    want = R.gemm(QA, QB, sa, sb)
    got = _exact_gemm_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


# -------------------------------------------------------------------------------------------------------------- accuracy
_LUT = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float64)


def deq_torch(Q: torch.Tensor, SF: torch.Tensor) -> torch.Tensor:
    """fp64 dequantisation on the device: [rows, Kp/2] + [rows, Kp/32] -> [rows, Kp]."""
    lut = _LUT.to(Q.device)
    c = torch.stack([Q & 15, Q >> 4], dim=-1).reshape(Q.shape[0], -1).long()
    v = lut[c].reshape(Q.shape[0], SF.shape[1], 32)
    return (v * torch.exp2(SF.double() - 127)[..., None]).reshape(Q.shape[0], -1)


_W = {}


def _weight(N, KQ, KE):
    key = (N, KQ, KE)
    if key not in _W:
        _W.clear()
        g = torch.Generator().manual_seed(N + KQ)
        w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
        idx = random_perm(KQ, 3).to(DEV)
        QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE)
        _W[key] = (idx, QW, SW, deq_torch(QW, SW))
    return _W[key]


def _check(D, ref, bf16: bool):
    """fp32 output: within 1e-3 (Frobenius) of fp64.  bf16 output: >= 99 % equal to the RNE of the fp64 value (its own rounding
    alone is ~1e-3 relative, so the Frobenius bound applies to the un-rounded form)."""
    ref = ref.double()
    rel = (torch.linalg.norm(D.double() - ref) / torch.linalg.norm(ref)).item()
    if bf16:
        assert rel < 4e-3, rel
        same = (D.view(torch.int16) == ref.to(torch.bfloat16).view(torch.int16)).double().mean().item()
        assert same >= 0.99, same
    else:
        assert rel < 1e-3, rel


@pytest.mark.parametrize("N", [16, 3584, 4096, 10752, 37888])
@pytest.mark.parametrize("M", [1, 2, 4, 8, 15, 16, 17, 32, 33, 64, 128, 129, 1000, 4096])
def test_gemm_accuracy(M, N):
    KQ, KE = (4096, 64) if (M + N) % 2 == 0 else (3584, 256)        # K = 4160 (a 64-element tail) or 3840 (none)
    if M == 4096 and N == 37888:
        KQ, KE = 4096, 64
    idx, QW, SW, Wd = _weight(N, KQ, KE)
    x = outlier_activations(M, KQ, M + 5).to(DEV)
    QX, SX = agemm.mx_reorder_quantize_x(x, idx, KE)
    ref = deq_torch(QX, SX) @ Wd.T
    D = agemm.mx_matmul(QX, QW, SX, SW, 1.0)
    _check(D, ref, True)
    D32 = agemm.mx_matmul(QX, QW, SX, SW, 0.75, out_dtype=torch.float32)
    _check(D32, 0.75 * ref, False)


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("M,N", [(4, 4096), (17, 3584), (4096, 3584), (129, 10752)])
def test_epilogue_bias_residual_alpha(M, N):
    """bias / residual (also aliasing D) / device alpha / fp32 output, bit-exact against the epilogue applied to the kernel's own
    un-rounded fp32 result (arcq_gemm_nvfp4's roundings: bf16(acc), + bias -> bf16, + residual -> bf16)."""
    KQ, KE = 4096, 64
    idx, QW, SW, _ = _weight(N, KQ, KE)
    x = outlier_activations(M, KQ, 77).to(DEV)
    QX, SX = agemm.mx_reorder_quantize_x(x, idx, KE)
    g = torch.Generator().manual_seed(M)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    res = (torch.randn(M, N, generator=g) * 4).to(torch.bfloat16).to(DEV)
    alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    acc = agemm.mx_matmul(QX, QW, SX, SW, alpha, out_dtype=torch.float32, scale_host=1.5)      # alpha = 1.5 * 0.5 on the device
    base = agemm.mx_matmul(QX, QW, SX, SW, 0.75, out_dtype=torch.float32)
    assert torch.equal(acc, base)
    want_b = _bf(_bf(_bf(acc) + bias.float()) + res.float()).to(torch.bfloat16)
    got_b = agemm.mx_matmul(QX, QW, SX, SW, alpha, scale_host=1.5, bias=bias, residual=res)
    assert torch.equal(got_b.view(torch.int16), want_b.view(torch.int16))
    alias = res.clone()
    agemm.mx_matmul(QX, QW, SX, SW, 0.75, bias=bias, residual=alias, out=alias)
    assert torch.equal(alias.view(torch.int16), want_b.view(torch.int16))
    want_f = acc + bias.float() + res.float()
    got_f = agemm.mx_matmul(QX, QW, SX, SW, 0.75, bias=bias, residual=res, out_dtype=torch.float32)
    assert torch.equal(got_f, want_f)


# -------------------------------------------------------------------------------------------------------------- the two forms
@pytest.fixture(scope="module")
def ext():
    if not os.path.exists(_build_ext.OUT):
        _build_ext.build_agemm_extension()
    return _build_ext.import_agemm_extension()


@pytest.mark.parametrize("M,N,KQ,KE", [(4, 4096, 4096, 64), (300, 3584, 3584, 256)])
def test_extension_equals_mirror(ext, M, N, KQ, KE):
    x = outlier_activations(M, KQ, 9).to(DEV)
    w = _inputs(N, KQ, 10, "w").to(DEV)
    idx = random_perm(KQ, 11).to(DEV)
    qx, sx = agemm.mx_reorder_quantize_x(x, idx, KE)
    qw, sw = agemm.mx_reorder_quantize_w(w, idx, KE)
    eqx, esx = ext.mx_reorder_quantize_x(X=x, reorder_index=idx, KE=KE)
    eqw, esw = ext.mx_reorder_quantize_w(W=w, reorder_index=idx, KE=KE)
    for a, b in ((qx, eqx), (sx, esx), (qw, eqw), (sw, esw)):
        assert torch.equal(a, b)
    bias = torch.randn(N).to(torch.bfloat16).to(DEV)
    s = torch.tensor(0.25, dtype=torch.float32, device=DEV)
    d = agemm.mx_matmul(qx, qw, sx, sw, s, bias=bias, scale_host=2.0)
    e = ext.mx_matmul(A=qx, B=qw, SFA=sx, SFB=sw, scale=s, bias=bias, scale_host=2.0)
    assert torch.equal(d.view(torch.int16), e.view(torch.int16))
    d32 = agemm.mx_matmul(qx, qw, sx, sw, 0.5, out_dtype=torch.float32)
    e32 = ext.mx_matmul(qx, qw, sx, sw, 0.5, out_dtype=torch.float32)
    assert torch.equal(d32, e32)


# -------------------------------------------------------------------------------------------------------------- layer
@pytest.mark.parametrize("bsz,q_len,KQ,N,KE", [(1, 4, 4096, 4096, 64), (2, 100, 3584, 3584, 256)])
def test_qlinear_layer_mxfp4(bsz, q_len, KQ, N, KE):
    torch.manual_seed(KQ + KE)
    lin = torch.nn.Linear(KQ, N, bias=True).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 5).to(DEV)
    layer = QLinearLayer(lin, KE, idx, quant_type="MXFP4")
    x = outlier_activations(bsz * q_len, KQ, 6).to(DEV)
    qx, sx, scale = reorder_quantize_x(x, idx, KE, quant_type="MXFP4")
    assert scale.dim() == 0 and scale.item() == 1.0
    y = layer((qx, sx, scale, bsz, q_len))
    assert y.shape == (bsz, q_len, N) and y.dtype == torch.bfloat16
    acc = deq_torch(qx, sx) @ deq_torch(layer.W, layer.scale_w).T
    # the layer's bf16 output rounds twice (the product, then + bias: model/qLinearLayer.py:74-76); the fp64 reference is rounded
    # the same way, so what remains is the GEMM's own error
    ref = (acc.to(torch.bfloat16).double() + lin.bias.double()).to(torch.bfloat16).double()
    rel = (torch.linalg.norm(y.reshape(-1, N).double() - ref) / torch.linalg.norm(ref)).item()
    assert rel < 1e-3, rel
    rel_raw = (torch.linalg.norm(y.reshape(-1, N).double() - (acc + lin.bias.double())) / torch.linalg.norm(acc)).item()
    assert rel_raw < 4e-3, rel_raw
    for flag in ("repack_for_decode", "repacked_only"):
        with pytest.raises(ValueError):
            QLinearLayer(lin, KE, idx, quant_type="MXFP4", **{flag: True})
