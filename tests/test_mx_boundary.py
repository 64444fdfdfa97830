"""CPU checks of the MXFP4 boundary: the C-ABI rejects every shape, NULL and alignment violation with its documented status before
any HIP call (on a machine without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), its layout helpers
agree with tests/mx_reference.py, and the agemm mirror raises on a wrong dtype, shape or device."""
import pytest
import torch

from arcquant_amd import _lib, agemm
from tests import mx_reference as R

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation)


def L():
    return _lib.lib()


def test_layout_helpers():
    for K in (64, 128, 4160, 3840, 19008, 0):
        assert L().arcq_mx_k_padded(K) == (R.k_padded(K) if K > 0 else 0)
        assert L().arcq_mx_sf_bytes(7, K) == 7 * (R.k_padded(K) // 32 if K > 0 else 0)


@pytest.mark.parametrize("fn", ["arcq_mx_quantize_x", "arcq_mx_quantize_w"])
def test_quantisers_reject_before_any_hip_call(fn):
    f = getattr(L(), fn)
    for KQ, KE in [(96, 0), (4096, 32), (4096, 48), (64, 128), (32768, 0), (4096, -64)]:       # KQ % 64, KE % 64, KE > KQ, range
        assert f(P, P, P, P, 4, KQ, KE, None) == SHAPE, (KQ, KE)
    assert f(None, P, P, P, 4, 4096, 64, None) == NULL
    assert f(P, None, P, P, 4, 4096, 64, None) == NULL
    assert f(P, P, None, P, 4, 4096, 64, None) == NULL
    assert f(P, P, P, None, 4, 4096, 64, None) == NULL
    for bad in ((P + 8, P, P), (P, P + 2, P), (P, P, P + 8)):                                  # X, reorder_index, Q need 16 B
        assert f(bad[0], bad[1], bad[2], P, 4, 4096, 64, None) == SHAPE
    assert f(P, P, P, P, 0, 4096, 64, None) == 0                                              # no rows: nothing to do


def test_gemm_rejects_before_any_hip_call():
    g = L().arcq_gemm_mxfp4

    def call(A=P, B=P, SA=P, SB=P, D=P, M=4, N=4096, K=4224, bias=None, res=None, out=0):
        return g(A, B, SA, SB, D, M, N, K, 1.0, None, bias, res, out, None, 0, None)

    assert call(K=4160) == SHAPE            # K % 128
    assert call(K=0) == SHAPE
    assert call(N=4104) == SHAPE            # N % 16
    assert call(M=-1) == SHAPE
    assert call(out=2) == SHAPE             # out_dtype
    for kw in ("A", "B", "SA", "SB", "D"):
        assert call(**{kw: None}) == NULL, kw
    for kw in ("A", "B", "D"):
        assert call(**{kw: P + 4}) == SHAPE, kw
    for kw in ("SA", "SB"):
        assert call(**{kw: P + 2}) == SHAPE, kw
    assert call(bias=P + 1) == SHAPE
    assert call(res=P + 1) == SHAPE
    assert call(M=0) == 0 and call(N=0) == 0


def test_mirror_raises_on_dtype_shape_device():
    idx = torch.arange(128, dtype=torch.int16)
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="dtype|bfloat16"):
        agemm.mx_reorder_quantize_x(x.float(), idx, 64)
    with pytest.raises(RuntimeError, match="int16"):
        agemm.mx_reorder_quantize_w(x, idx.int(), 64)
    with pytest.raises(RuntimeError, match="2-D"):
        agemm.mx_reorder_quantize_x(x.reshape(-1), idx, 64)
    with pytest.raises(RuntimeError, match="not valid"):
        agemm.mx_reorder_quantize_x(x, idx, 32)
    with pytest.raises(RuntimeError, match="entries"):
        agemm.mx_reorder_quantize_x(x, idx[:64], 0)
    with pytest.raises(RuntimeError, match="GPU"):
        agemm.mx_reorder_quantize_x(x, idx, 64)
    A = torch.zeros(4, 128, dtype=torch.uint8)
    SA = torch.zeros(4, 8, dtype=torch.uint8)
    B = torch.zeros(32, 128, dtype=torch.uint8)
    SB = torch.zeros(32, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8"):
        agemm.mx_matmul(A.float(), B, SA, SB, 1.0)
    with pytest.raises(RuntimeError, match="K=192"):
        agemm.mx_matmul(A, B[:, :96].contiguous(), SA, SB, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        agemm.mx_matmul(A[:, :96].contiguous(), B[:, :96].contiguous(), SA, SB, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        agemm.mx_matmul(A, B[:24], SA, SB[:24], 1.0)
    with pytest.raises(RuntimeError, match="K/32"):
        agemm.mx_matmul(A, B, SA[:, :4].contiguous(), SB, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        agemm.mx_matmul(A, B, SA, SB, 1.0)


def test_qlinear_quant_types():
    from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
    lin = torch.nn.Linear(128, 32)
    idx = torch.arange(128)
    for flag in ("repack_for_decode", "repacked_only"):
        with pytest.raises(ValueError):
            QLinearLayer(lin, 64, idx, quant_type="MXFP4", **{flag: True})
    with pytest.raises(NotImplementedError):
        QLinearLayer(lin, 64, idx, quant_type="INT4")
    with pytest.raises(NotImplementedError):
        reorder_quantize_x(torch.zeros(2, 128, dtype=torch.bfloat16), idx.to(torch.int16), 64, quant_type="INT4")
    with pytest.raises(RuntimeError, match="GPU"):           # MXFP4 is dispatched (and then needs the GPU)
        reorder_quantize_x(torch.zeros(2, 128, dtype=torch.bfloat16), idx.to(torch.int16), 64, quant_type="MXFP4")
