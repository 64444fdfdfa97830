"""CPU checks of the boundary of the MXFP4 decode GEMMs over the repacked weight: arcq_gemm_mxfp4_repacked and
arcq_gemm_mxfp4_repacked_silu_mul answer every violation with its documented status and text before any HIP call (on a machine without a
GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), in the order of include/arcq.h; the Python mirrors raise from CPU
tensors naming the broken argument and refuse the unbroken CPU set last for living on the CPU; and the layer / harness keywords follow
their rules."""
import pytest
import torch

from arcquant_amd import _lib, agemm, mx

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or has no rows)
BF16, U8 = torch.bfloat16, torch.uint8


def L():
    return _lib.lib()


def _plain(A=P, W=P, SA=P, SW=P, D=P, M=4, N=4096, K=4224, bias=None, residual=None, out_dtype=0):
    return L().arcq_gemm_mxfp4_repacked(A, W, SA, SW, D, M, N, K, 1.0, None, bias, residual, out_dtype, None)


def _silu(A=P, W=P, SA=P, SW=P, D=P, M=4, N=4096, K=4224, bias=None, residual=None, out_dtype=0):
    assert residual is None and out_dtype == 0
    return L().arcq_gemm_mxfp4_repacked_silu_mul(A, W, SA, SW, D, M, N, K, 1.0, None, bias, None)


ENTRIES = [(_plain, "arcq_gemm_mxfp4_repacked", "D"), (_silu, "arcq_gemm_mxfp4_repacked_silu_mul", "ACT")]


def _says(call, status, text, **kw):
    assert call(**kw) == status, kw
    assert L().arcq_last_error().decode() == text, kw


@pytest.mark.parametrize("call,who,d", ENTRIES)
def test_rejections_with_status_and_text(call, who, d):
    shape = who + ": need M,N >= 0, K % 128 == 0 and N % 16 == 0 (M={M} N={N} K={K})"
    _says(call, SHAPE, shape.format(M=4, N=4096, K=4160), K=4160)
    _says(call, SHAPE, shape.format(M=4, N=4096, K=0), K=0)
    _says(call, SHAPE, shape.format(M=4, N=4104, K=4224), N=4104)
    _says(call, SHAPE, shape.format(M=-1, N=4096, K=4224), M=-1)
    _says(call, SHAPE, who + ": need M <= 64 over the repacked weight (M=65)", M=65)
    for kw in ("A", "W", "SA", "SW", "D"):
        _says(call, NULL, who + ": NULL pointer", **{kw: None})
    for kw in ("A", "W", "D"):
        _says(call, SHAPE, f"{who}: A, MRW and {d} must be 16-byte aligned", **{kw: P + 8})
    for kw in ("SA", "SW"):
        _says(call, SHAPE, who + ": SFA and MRSF must be 4-byte aligned", **{kw: P + 2})
    assert call(bias=P + 1) == SHAPE and b"bias" in L().arcq_last_error()
    assert call(M=0) == 0 and call(N=0) == 0
    assert call(M=0, A=None, W=None, SA=None, SW=None, D=None) == 0
    for M in (1, 64):                                        # the ends of the M range pass the shape rules (NULL is what is left to find)
        assert call(M=M, A=None) == NULL


def test_plain_entry_out_dtype_and_residual():
    who = "arcq_gemm_mxfp4_repacked"
    _says(_plain, SHAPE, who + ": bad out_dtype 2", out_dtype=2)
    assert _plain(residual=P + 1) == SHAPE and b"residual" in L().arcq_last_error()
    assert _plain(out_dtype=1, A=None) == NULL


@pytest.mark.parametrize("call,who,d", ENTRIES)
def test_rejection_order(call, who, d):
    """arcq.h: divisibility, M > 64, out_dtype, the empty shape, NULL, 16-byte, 4-byte, bias / residual."""
    everything = dict(K=4160, M=65, A=None, W=P + 8, SA=P + 2, bias=P + 1)
    assert call(**everything) == SHAPE and b"K % 128" in L().arcq_last_error()
    del everything["K"]
    assert call(**everything) == SHAPE and b"M <= 64" in L().arcq_last_error()
    del everything["M"]
    if call is _plain:
        assert call(out_dtype=7, **everything) == SHAPE and b"out_dtype" in L().arcq_last_error()
        assert call(out_dtype=7, M=0) == SHAPE                 # out_dtype ahead of the empty shape
    assert call(M=0, **{k: v for k, v in everything.items()}) == 0          # the empty shape ahead of every pointer rule
    assert call(**everything) == NULL
    del everything["A"]
    assert call(**everything) == SHAPE and b"16-byte" in L().arcq_last_error()
    del everything["W"]
    assert call(**everything) == SHAPE and b"4-byte" in L().arcq_last_error()
    del everything["SA"]
    assert call(**everything) == SHAPE and b"bias" in L().arcq_last_error()
    assert call(M=65, K=4160) == SHAPE and b"K % 128" in L().arcq_last_error()     # M > 64 is reported once the divisibility rules hold


def test_abi_version_unchanged():
    assert L().arcq_abi_version() == 1


# ---- the Python mirrors -----------------------------------------------------------------------------------------------------------
def _raises(pattern, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        fn(*a, **kw)


def _broken(t):
    """dtype, contiguity and rank faults of one tensor."""
    yield t.to(torch.float64)
    yield torch.stack([t, t], dim=-1)[..., 0]
    yield t.unsqueeze(0)


def _cpu_set(M=4, N=32, K=128):
    A, SA = torch.zeros(M, K // 2, dtype=U8), torch.zeros(M, K // 32, dtype=U8)
    MRW, MRSF = agemm.mx_repack_w(torch.zeros(N, K // 2, dtype=U8), torch.zeros(N, K // 32, dtype=U8))
    return A, MRW, SA, MRSF


@pytest.mark.parametrize("fn", [agemm.mx_matmul_repacked, mx.matmul_silu_mul_repacked], ids=["plain", "silu_mul"])
def test_mirrors_name_the_broken_argument(fn):
    A, MRW, SA, MRSF = _cpu_set()
    ok = dict(A=A, MRW=MRW, SFA=SA, MRSF=MRSF)
    for name, t in ok.items():
        for bad in _broken(t):
            _raises(name, fn, **{**ok, name: bad}, scale=1.0, N=32)
    _raises("multiple of 128", fn, A[:, :48].contiguous(), MRW, SA, MRSF, 1.0, 32)
    _raises("multiple of 16", fn, A, MRW, SA, MRSF, 1.0, 24)
    _raises("multiple of 16", fn, A, MRW, SA, MRSF, 1.0, 0)
    _raises("do not belong", fn, A, MRW, SA, MRSF, 1.0, 48)
    _raises("do not belong", fn, A, MRW[:-16].contiguous(), SA, MRSF, 1.0, 32)
    _raises("do not belong", fn, A, MRW, SA, torch.cat([MRSF, MRSF]), 1.0, 32)
    _raises("K/32", fn, A, MRW, SA[:, :2].contiguous(), MRSF, 1.0, 32)
    _raises("K/32", fn, A, MRW, SA[:2].contiguous(), MRSF, 1.0, 32)
    A65, _, SA65, _ = _cpu_set(M=65)
    _raises("M=65", fn, A65, MRW, SA65, MRSF, 1.0, 32)
    _raises("M=0", fn, A[:0], MRW, SA[:0], MRSF, 1.0, 32)
    bias = torch.zeros(32, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:16]]:
        _raises("bias", fn, A, MRW, SA, MRSF, 1.0, 32, bias=bad)
    out = torch.zeros(4, 32 if fn is agemm.mx_matmul_repacked else 16, dtype=BF16)
    for bad in list(_broken(out)) + [torch.zeros(4, 8, dtype=BF16)]:
        _raises("out", fn, A, MRW, SA, MRSF, 1.0, 32, out=bad)
    _raises("GPU", fn, A, MRW, SA, MRSF, 1.0, 32, bias=bias, out=out)           # the device check comes last


def test_plain_mirror_out_dtype_and_residual():
    A, MRW, SA, MRSF = _cpu_set()
    _raises("out_dtype", agemm.mx_matmul_repacked, A, MRW, SA, MRSF, 1.0, 32, out_dtype=torch.float16)
    res = torch.zeros(4, 32, dtype=BF16)
    for bad in list(_broken(res)) + [res[:2]]:
        _raises("residual", agemm.mx_matmul_repacked, A, MRW, SA, MRSF, 1.0, 32, residual=bad)
    _raises("GPU", agemm.mx_matmul_repacked, A, MRW, SA, MRSF, 1.0, 32, residual=res, out_dtype=torch.float32)


# ---- layer and harness keywords -----------------------------------------------------------------------------------------------------
def test_qlinear_layer_keyword_rules():
    from arcquant_amd.qlinear import QLinearLayer
    lin = torch.nn.Linear(128, 32, bias=False)
    idx = torch.arange(128)
    with pytest.raises(ValueError, match="mx_repack_for_decode"):
        QLinearLayer(lin, 64, idx, quant_type="NVFP4", mx_repack_for_decode=True)
    with pytest.raises(ValueError, match="mx_repack_for_decode"):
        QLinearLayer(lin, 64, idx, mx_repack_for_decode=True)                  # NVFP4 is the default
    for kw in ("repack_for_decode", "repacked_only"):                          # the NVFP4 keywords keep raising for MXFP4
        with pytest.raises(ValueError, match="NVFP4 weight layout"):
            QLinearLayer(lin, 64, idx, quant_type="MXFP4", mx_repack_for_decode=True, **{kw: True})
    with pytest.raises(RuntimeError, match="GPU"):                             # the keyword itself is accepted: what is left is the device
        QLinearLayer(lin, 64, idx, quant_type="MXFP4", mx_repack_for_decode=True)


def test_decoder_model_keyword_rules():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="mx_repacked_decode"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, mx_repacked_decode=True)                       # NVFP4
    with pytest.raises(ValueError, match="mx_repacked_decode"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, quant_type="MXFP4", mx_quantised_epilogue=True, mx_repacked_decode=True)
    with pytest.raises(ValueError, match="mx_repacked_decode"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=False, quant_type="MXFP4", mx_repacked_decode=True)
    import inspect
    for fn in (e2e.bench_decode, e2e.bench_protocol):
        assert inspect.signature(fn).parameters["mx_repacked_decode"].default is False
