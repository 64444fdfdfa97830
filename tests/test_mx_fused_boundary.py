"""CPU checks of the MXFP4 decoder-layer operators' boundary (arcq_mx_rmsnorm_quantize_x, arcq_mx_silu_mul_quantize_x,
arcq_gemm_mxfp4_silu_mul and the arcquant_amd.mx module): every shape, NULL and alignment violation is answered with its documented
status before any HIP call (on a machine without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), and the
module raises RuntimeError naming the broken argument from CPU tensors, refusing the unbroken CPU set last for living on the CPU."""
import pytest
import torch

from arcquant_amd import _lib, agemm, mx

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or has no rows)
BF16, U8, I16 = torch.bfloat16, torch.uint8, torch.int16


def L():
    return _lib.lib()


def test_rmsnorm_quantiser_rejects_before_any_hip_call():
    def call(X=P, W=P, idx=P, Q=P, SF=P, M=4, KQ=4096, KE=64):
        return L().arcq_mx_rmsnorm_quantize_x(X, W, 1e-6, idx, Q, SF, M, KQ, KE, None)

    for KQ in (1984, 8256):                                   # outside [2048, 8192], the range of the reduction tree
        assert call(KQ=KQ) == SHAPE, KQ
    for KQ in (2048, 8192):                                   # the ends of the range are not a shape error (NULL is what is left to find)
        assert call(KQ=KQ, X=None) == NULL, KQ
        assert call(KQ=KQ, M=0) == 0, KQ
    for KQ, KE in [(4096, 32), (4096, 48), (2048, 2112), (4096, -64), (4128, 0)]:        # KE % 64, KE > KQ, KE < 0, KQ % 64
        assert call(KQ=KQ, KE=KE) == SHAPE, (KQ, KE)
    assert call(M=-1) == SHAPE
    for kw in ("X", "W", "idx", "Q", "SF"):
        assert call(**{kw: None}) == NULL, kw
    for kw, off in (("X", 8), ("W", 8), ("idx", 2), ("Q", 8)):   # 16-byte alignment
        assert call(**{kw: P + off}) == SHAPE, kw
    assert call(M=0) == 0
    assert call(M=0, X=None, W=None, idx=None, Q=None, SF=None) == 0


def test_silu_mul_quantiser_rejects_before_any_hip_call():
    def call(GU=P, idx=P, Q=P, SF=P, M=4, KQ=4096, KE=64, layout=0):
        return L().arcq_mx_silu_mul_quantize_x(GU, idx, Q, SF, M, KQ, KE, layout, None)

    for KQ, KE in [(96, 0), (4096, 32), (4096, 48), (64, 128), (32768, 0), (4096, -64)]:      # arcq_mx_quantize_x's rules
        assert call(KQ=KQ, KE=KE) == SHAPE, (KQ, KE)
    for layout in (-1, 2, 7):
        assert call(layout=layout) == SHAPE, layout
        assert b"layout" in L().arcq_last_error()
    for layout in (0, 1):
        assert call(layout=layout, GU=None) == NULL
    for kw in ("GU", "idx", "Q", "SF"):
        assert call(**{kw: None}) == NULL, kw
    for kw, off in (("GU", 8), ("idx", 2), ("Q", 8)):
        assert call(**{kw: P + off}) == SHAPE, kw
    assert call(M=0) == 0 and call(M=0, layout=1) == 0


def test_silu_mul_gemm_rejects_before_any_hip_call():
    g = L().arcq_gemm_mxfp4_silu_mul

    def call(A=P, B=P, SA=P, SB=P, ACT=P, M=4, N=4096, K=4224, bias=None):
        return g(A, B, SA, SB, ACT, M, N, K, 1.0, None, bias, None)

    assert call(K=4160) == SHAPE            # K % 128
    assert call(K=0) == SHAPE
    assert call(N=4104) == SHAPE            # N % 16
    assert call(N=4088) == SHAPE
    assert call(M=-1) == SHAPE
    for kw in ("A", "B", "SA", "SB", "ACT"):
        assert call(**{kw: None}) == NULL, kw
    for kw in ("A", "B", "ACT"):
        assert call(**{kw: P + 4}) == SHAPE, kw
    for kw in ("SA", "SB"):
        assert call(**{kw: P + 2}) == SHAPE, kw
    assert call(bias=P + 1) == SHAPE
    assert call(M=0) == 0 and call(N=0) == 0
    for M in (4, 65):                       # both kernels' shapes share the checks
        assert call(M=M, A=None) == NULL


def _raises(pattern, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        fn(*a, **kw)


def _broken(t):
    """dtype, contiguity and rank faults of one tensor."""
    yield t.to(torch.float64)
    yield torch.stack([t, t], dim=-1)[..., 0]
    yield t.unsqueeze(0)


def test_module_rmsnorm_quantize_x_names_the_broken_argument():
    X, W, idx = torch.zeros(4, 2048, dtype=BF16), torch.ones(2048, dtype=BF16), torch.arange(2048, dtype=I16)
    for bad in _broken(X):
        _raises("X", mx.rmsnorm_quantize_x, bad, W, 1e-6, idx, 64)
    for bad in _broken(W):
        _raises("W", mx.rmsnorm_quantize_x, X, bad, 1e-6, idx, 64)
    for bad in _broken(idx):
        _raises("reorder_index", mx.rmsnorm_quantize_x, X, W, 1e-6, bad, 64)
    _raises("W / reorder_index", mx.rmsnorm_quantize_x, X, W[:1024].contiguous(), 1e-6, idx, 64)
    _raises("W / reorder_index", mx.rmsnorm_quantize_x, X, W, 1e-6, idx[:1024].contiguous(), 64)
    _raises("not valid", mx.rmsnorm_quantize_x, X, W, 1e-6, idx, 32)
    _raises("not valid", mx.rmsnorm_quantize_x, X, W, 1e-6, idx, 4096)
    _raises("not valid", mx.rmsnorm_quantize_x, X[:, :1984].contiguous(), W[:1984].contiguous(), 1e-6, idx[:1984].contiguous(), 64)
    _raises("GPU", mx.rmsnorm_quantize_x, X, W, 1e-6, idx, 64)


def test_module_silu_mul_quantize_x_names_the_broken_argument():
    GU, idx = torch.zeros(4, 256, dtype=BF16), torch.arange(128, dtype=I16)
    for bad in _broken(GU):
        _raises("GU", mx.silu_mul_quantize_x, bad, idx, 64)
    for bad in _broken(idx):
        _raises("reorder_index", mx.silu_mul_quantize_x, GU, bad, 64)
    _raises("GU", mx.silu_mul_quantize_x, GU[:, :255].contiguous(), idx, 64)
    _raises("layout", mx.silu_mul_quantize_x, GU, idx, 64, layout=2)
    _raises("reorder_index", mx.silu_mul_quantize_x, GU, idx[:64].contiguous(), 64)
    _raises("not valid", mx.silu_mul_quantize_x, GU, idx, 32)
    _raises("not valid", mx.silu_mul_quantize_x, GU, idx, 192)
    for layout in (agemm.GU_HALVES, agemm.GU_PAIRS):
        _raises("GPU", mx.silu_mul_quantize_x, GU, idx, 64, layout=layout)


def test_module_matmul_silu_mul_names_the_broken_argument():
    A, SA = torch.zeros(4, 128, dtype=U8), torch.zeros(4, 8, dtype=U8)
    B, SB = torch.zeros(32, 128, dtype=U8), torch.zeros(32, 8, dtype=U8)
    ok = dict(A=A, B=B, SFA=SA, SFB=SB)
    for name, t in ok.items():
        for bad in _broken(t):
            _raises(name, mx.matmul_silu_mul, **{**ok, name: bad}, scale=1.0)
    _raises("K=192", mx.matmul_silu_mul, A, B[:, :96].contiguous(), SA, SB, 1.0)
    _raises("multiple of 128", mx.matmul_silu_mul, A[:, :96].contiguous(), B[:, :96].contiguous(), SA, SB, 1.0)
    _raises("multiple of 16", mx.matmul_silu_mul, A, B[:24], SA, SB[:24], 1.0)
    _raises("K/32", mx.matmul_silu_mul, A, B, SA[:, :4].contiguous(), SB, 1.0)
    _raises("K/32", mx.matmul_silu_mul, A, B, SA, SB[:16], 1.0)
    bias = torch.zeros(32, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:16]]:
        _raises("bias", mx.matmul_silu_mul, A, B, SA, SB, 1.0, bias=bad)
    out = torch.zeros(4, 16, dtype=BF16)
    for bad in list(_broken(out)) + [torch.zeros(4, 32, dtype=BF16)]:
        _raises("out", mx.matmul_silu_mul, A, B, SA, SB, 1.0, out=bad)
    _raises("GPU", mx.matmul_silu_mul, A, B, SA, SB, 1.0, bias=bias, out=out)


def test_qlinear_mxfp4_rmsnorm_quantize_x_is_dispatched():
    from arcquant_amd.qlinear import MXFP4_rmsnorm_quantize_x
    X, W, idx = torch.zeros(2, 2048, dtype=BF16), torch.ones(2048, dtype=BF16), torch.arange(2048, dtype=I16)
    _raises("GPU", MXFP4_rmsnorm_quantize_x, X, W, 1e-6, idx, 64)           # it reaches the operator (which then needs the GPU)


def test_decoder_model_rejects_repacked_only_with_mxfp4():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    with pytest.raises(ValueError, match="MXFP4"):
        e2e.DecoderModel(cfg, 1, 8, torch.device("cpu"), fused=True, repacked_only=True, quant_type="MXFP4")
    with pytest.raises(NotImplementedError):
        e2e.DecoderModel(cfg, 1, 8, torch.device("cpu"), quant_type="INT4")
