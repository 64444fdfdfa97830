"""CPU checks of the boundary of the quantising gate|up GEMM (arcq_gemm_mxfp4_silu_mul_quantize, mx.matmul_silu_mul_quantize,
mx.gate_up_rows and DecoderModel's mx_quantised_epilogue flag): every shape, NULL and alignment violation is answered with its documented
status before any HIP call (on a machine without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), and the module
raises RuntimeError naming the broken argument from CPU tensors, refusing the unbroken CPU set last for living on the CPU."""
import pytest
import torch

from arcquant_amd import _lib, mx

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or has no rows)
BF16, U8 = torch.bfloat16, torch.uint8


def call(A=P, B=P, SA=P, SB=P, Q=P, SF=P, M=4, N=4096, K=4224, bias=None, KE=64):
    return _lib.lib().arcq_gemm_mxfp4_silu_mul_quantize(A, B, SA, SB, Q, SF, M, N, K, 1.0, None, bias, KE, None)


def test_shape_rules_are_answered_before_any_hip_call():
    for K in (4160, 64, 0, -128):                               # K % 128, K <= 0
        assert call(K=K) == SHAPE, K
    for N in (4160, 4032, 64, 16, -128):                        # (N / 2) % 64
        assert call(N=N) == SHAPE, N
    for KE in (32, 48, 96, -64, 2112):                          # KE % 64, KE < 0, KE > N / 2
        assert call(KE=KE) == SHAPE, KE
        assert b"KE" in _lib.lib().arcq_last_error()
    assert call(N=128, KE=128) == SHAPE
    assert call(N=65536 + 128, KE=64) == SHAPE                  # N / 2 > 32767
    assert call(N=65536, KE=64) == SHAPE
    assert call(M=-1) == SHAPE
    # the ends of the ranges are not shape errors: NULL is what is left to find
    for N, KE in ((128, 64), (128, 0), (4096, 2048), (65408, 64)):
        assert call(N=N, KE=KE, A=None) == NULL, (N, KE)
    for M in (1, 64, 65, 4096):                                 # both kernels' shapes share the checks
        assert call(M=M, A=None) == NULL, M
        assert call(M=M, KE=32) == SHAPE, M


def test_null_and_alignment_are_answered_before_any_hip_call():
    for kw in ("A", "B", "SA", "SB", "Q", "SF"):
        assert call(**{kw: None}) == NULL, kw
    for kw in ("A", "B", "Q"):
        assert call(**{kw: P + 4}) == SHAPE, kw
        assert call(**{kw: P + 8}) == SHAPE, kw
    assert b"QACT" in _lib.lib().arcq_last_error()
    for kw in ("SA", "SB"):
        assert call(**{kw: P + 2}) == SHAPE, kw
    assert call(bias=P + 1) == SHAPE
    # gemm_checks' order: a shape error before a NULL pointer, a NULL pointer before a misaligned one
    assert call(K=4160, A=None) == SHAPE
    assert call(KE=32, A=None) == SHAPE
    assert call(SF=None, A=P + 4) == NULL
    assert call(Q=None, B=P + 4) == NULL


def test_no_rows_is_ok():
    assert call(M=0) == 0
    assert call(M=0, A=None, B=None, SA=None, SB=None, Q=None, SF=None) == 0
    assert call(M=0, KE=32) == SHAPE                            # ... but only for a shape inside the contract


def _raises(pattern, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        fn(*a, **kw)


def _broken(t):
    """dtype, contiguity and rank faults of one tensor."""
    yield t.to(torch.float64)
    yield torch.stack([t, t], dim=-1)[..., 0]
    yield t.unsqueeze(0)


def test_module_matmul_silu_mul_quantize_names_the_broken_argument():
    A, SA = torch.zeros(4, 128, dtype=U8), torch.zeros(4, 8, dtype=U8)
    B, SB = torch.zeros(256, 128, dtype=U8), torch.zeros(256, 8, dtype=U8)
    f = mx.matmul_silu_mul_quantize
    ok = dict(A=A, B=B, SFA=SA, SFB=SB)
    for name, t in ok.items():
        for bad in _broken(t):
            _raises(name, f, **{**ok, name: bad}, scale=1.0, KE=64)
    _raises("K=192", f, A, B[:, :96].contiguous(), SA, SB, 1.0, 64)
    _raises("multiple of 128", f, A[:, :96].contiguous(), B[:, :96].contiguous(), SA, SB, 1.0, 64)
    _raises("N=192", f, A, B[:192], SA, SB[:192], 1.0, 64)
    for KE in (32, -64, 192):
        _raises("KE=%d is not valid" % KE, f, A, B, SA, SB, 1.0, KE)
    _raises("K/32", f, A, B, SA[:, :4].contiguous(), SB, 1.0, 64)
    _raises("K/32", f, A, B, SA, SB[:128], 1.0, 64)
    bias = torch.zeros(256, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:128]]:
        _raises("bias", f, A, B, SA, SB, 1.0, 64, bias=bad)
    _raises("GPU", f, A, B, SA, SB, 1.0, 64, bias=bias)
    _raises("GPU", f, A, B, SA, SB, 1.0, 0, scale_host=2.0)


def test_gate_up_rows_orders_the_pairs():
    g = torch.Generator().manual_seed(0)
    gate, up = torch.randn(8, 5, generator=g).to(BF16), torch.randn(8, 5, generator=g).to(BF16)
    gb, ub = torch.randn(8, generator=g).to(BF16), torch.randn(8, generator=g).to(BF16)
    idx = torch.tensor([3, 1, 7, 0, 2, 6, 5, 4], dtype=torch.int16)
    w = mx.gate_up_rows(gate, up)
    assert w.shape == (16, 5) and w.is_contiguous() and torch.equal(w[0::2], gate) and torch.equal(w[1::2], up)
    w, b = mx.gate_up_rows(gate, up, idx, gb, ub)
    for j, c in enumerate(idx.tolist()):                        # pair j is channel reorder_index[j]
        assert torch.equal(w[2 * j], gate[c]) and torch.equal(w[2 * j + 1], up[c])
        assert b[2 * j] == gb[c] and b[2 * j + 1] == ub[c]
    assert torch.equal(mx.gate_up_rows(gate, up, idx), w)
    _raises("permutation", mx.gate_up_rows, gate, up, torch.tensor([0, 1, 2, 3, 4, 5, 6, 6], dtype=torch.int16))
    _raises("permutation", mx.gate_up_rows, gate, up, idx[:4])
    _raises("one shape", mx.gate_up_rows, gate, up[:4])
    _raises("together", mx.gate_up_rows, gate, up, idx, gb)
    _raises("shape", mx.gate_up_rows, gate, up, idx, gb, ub[:4])


def test_decoder_model_flag_needs_fused_mxfp4():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    cpu = torch.device("cpu")
    for kw in (dict(fused=True), dict(fused=True, quant_type="NVFP4"), dict(fused=False, quant_type="MXFP4"), dict(fused=False)):
        with pytest.raises(ValueError, match="mx_quantised_epilogue"):
            e2e.DecoderModel(cfg, 1, 8, cpu, mx_quantised_epilogue=True, **kw)
