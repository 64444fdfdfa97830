"""CPU checks of the MXFP6 boundary: the C-ABI rejects every shape, NULL and alignment violation with its documented status before any
HIP call (without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), and QLinearLayer's flags exclude each other."""
import pytest
import torch

from arcquant_amd import _lib

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or is empty)


def _gemm(A=P, B=P, SA=P, SB=P, D=P, M=4, N=4096, K=4224, fmt=0, bias=None, res=None, out=0):
    return _lib.lib().arcq_gemm_mxfp6(A, B, SA, SB, D, M, N, K, fmt, 1.0, None, bias, res, out, None)


@pytest.mark.parametrize("kw,status", [
    (dict(K=4160), SHAPE), (dict(K=0), SHAPE), (dict(N=4104), SHAPE), (dict(M=-1), SHAPE), (dict(fmt=2), SHAPE), (dict(fmt=-1), SHAPE),
    (dict(out=2), SHAPE), (dict(A=P + 8), SHAPE), (dict(B=P + 8), SHAPE), (dict(D=P + 4), SHAPE), (dict(SA=P + 2), SHAPE),
    (dict(SB=P + 2), SHAPE), (dict(bias=P + 1), SHAPE), (dict(res=P + 1), SHAPE),
    (dict(A=None), NULL), (dict(B=None), NULL), (dict(SA=None), NULL), (dict(SB=None), NULL), (dict(D=None), NULL),
    (dict(M=0), 0), (dict(N=0), 0), (dict(M=0, fmt=1), 0), (dict(K=4160, fmt=1), SHAPE), (dict(A=None, fmt=1), NULL),
])
def test_gemm_rejects_before_any_hip_call(kw, status):
    assert _gemm(**kw) == status
    if status:
        assert b"arcq_gemm_mxfp6" in _lib.lib().arcq_last_error()


@pytest.mark.parametrize("fn", ["arcq_mx6_quantize_x", "arcq_mx6_quantize_w"])
def test_quantisers_reject_before_any_hip_call(fn):
    f = getattr(_lib.lib(), fn)
    for KQ, KE in [(96, 0), (4096, 32), (64, 128), (32768, 0), (4096, -64)]:                   # KQ % 64, KE % 64, KE > KQ, range
        assert f(P, P, P, P, 4, KQ, KE, None) == SHAPE, (KQ, KE)
    for k in range(4):
        assert f(*[None if i == k else P for i in range(4)], 4, 4096, 64, None) == NULL
    for bad in ((P + 8, P, P), (P, P + 2, P), (P, P, P + 8)):                                  # X, reorder_index, Q need 16 B
        assert f(*bad, P, 4, 4096, 64, None) == SHAPE
    assert f(P, P, P, P, 0, 4096, 64, None) == 0                                              # no rows: nothing to do
    assert _lib.lib().arcq_mx6_code_bytes(7, 4160) == 7 * 3 * 4224 // 4 and _lib.lib().arcq_mx6_code_bytes(0, 64) == 0


def test_qlinear_flags():
    from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
    lin, idx = torch.nn.Linear(128, 32), torch.arange(128)
    for flag in ("repack_for_decode", "repacked_only", "mx_repack_for_decode", "mx_repacked_only"):
        with pytest.raises(ValueError):
            QLinearLayer(lin, 64, idx, quant_type="MXFP6", **{flag: True})
    for qt in ("NVFP4", "MXFP4"):
        with pytest.raises(ValueError):
            QLinearLayer(lin, 64, idx, quant_type=qt, mx6_weight="e2m1")
    with pytest.raises(ValueError):
        QLinearLayer(lin, 64, idx, quant_type="MXFP6", mx6_weight="e4m3")
    with pytest.raises(NotImplementedError):
        QLinearLayer(lin, 64, idx, quant_type="INT4")
    with pytest.raises(RuntimeError, match="GPU"):           # MXFP6 is dispatched (and then needs the GPU)
        QLinearLayer(lin, 64, idx, quant_type="MXFP6")
    with pytest.raises(RuntimeError, match="GPU"):
        reorder_quantize_x(torch.zeros(2, 128, dtype=torch.bfloat16), idx.to(torch.int16), 64, quant_type="MXFP6")
