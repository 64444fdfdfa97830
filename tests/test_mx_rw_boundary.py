"""CPU checks of the boundary of the MXFP4 GEMMs that serve EVERY batch size from the repacked weight: arcq_gemm_mxfp4_rw,
arcq_gemm_mxfp4_rw_silu_mul and arcq_gemm_mxfp4_rw_silu_mul_quantize answer every violation with its documented status and text before any
HIP call (on a machine without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH instead), in the order of include/arcq.h;
arcq_gemm_mxfp4_rw_route names the kernel of a shape; the Python mirrors raise from CPU tensors naming the broken argument and refuse the
unbroken CPU set last for living on the CPU; and the layer / harness keyword mx_repacked_only follows its rules."""
import inspect

import pytest
import torch

from arcquant_amd import _lib, agemm, mx

SHAPE, UNSUPPORTED, NULL = -1, -2, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or has no rows)
BF16, U8 = torch.bfloat16, torch.uint8


def L():
    return _lib.lib()


def _plain(A=P, W=P, SA=P, SW=P, D=P, M=4, N=4096, K=4224, bias=None, residual=None, out_dtype=0):
    return L().arcq_gemm_mxfp4_rw(A, W, SA, SW, D, M, N, K, 1.0, None, bias, residual, out_dtype, None)


def _silu(A=P, W=P, SA=P, SW=P, D=P, M=4, N=4096, K=4224, bias=None, residual=None, out_dtype=0):
    assert residual is None and out_dtype == 0
    return L().arcq_gemm_mxfp4_rw_silu_mul(A, W, SA, SW, D, M, N, K, 1.0, None, bias, None)


def _quant(A=P, W=P, SA=P, SW=P, D=P, SF=P, M=4, N=4096, K=4224, bias=None, residual=None, out_dtype=0, KE=64):
    assert residual is None and out_dtype == 0
    return L().arcq_gemm_mxfp4_rw_silu_mul_quantize(A, W, SA, SW, D, SF, M, N, K, 1.0, None, bias, KE, None)


# (call, name, the output's name in the alignment text, N's divisor)
ENTRIES = [(_plain, "arcq_gemm_mxfp4_rw", "D", 16), (_silu, "arcq_gemm_mxfp4_rw_silu_mul", "ACT", 16),
           (_quant, "arcq_gemm_mxfp4_rw_silu_mul_quantize", "QACT", 128)]


def _says(call, status, text, **kw):
    assert call(**kw) == status, kw
    assert L().arcq_last_error().decode() == text, kw


@pytest.mark.parametrize("call,who,d,nm", ENTRIES)
def test_rejections_with_status_and_text(call, who, d, nm):
    shape = who + f": need M,N >= 0, K % 128 == 0 and N % {nm} == 0 (M={{M}} N={{N}} K={{K}})"
    _says(call, SHAPE, shape.format(M=4, N=4096, K=4160), K=4160)
    _says(call, SHAPE, shape.format(M=4, N=4096, K=0), K=0)
    _says(call, SHAPE, shape.format(M=4, N=4104, K=4224), N=4104)
    _says(call, SHAPE, shape.format(M=-1, N=4096, K=4224), M=-1)
    if nm == 128:
        _says(call, SHAPE, shape.format(M=4, N=4112, K=4224), N=4112)       # a multiple of 16 is not enough for the quantising form
    for kw in ("A", "W", "SA", "SW", "D"):
        _says(call, NULL, who + ": NULL pointer", **{kw: None})
    for kw in ("A", "W", "D"):
        _says(call, SHAPE, f"{who}: A, MRW and {d} must be 16-byte aligned", **{kw: P + 8})
    for kw in ("SA", "SW"):
        _says(call, SHAPE, who + ": SFA and MRSF must be 4-byte aligned", **{kw: P + 2})
    assert call(bias=P + 1) == SHAPE and b"bias" in L().arcq_last_error()
    assert call(M=0) == 0 and (call(N=0, KE=0) if call is _quant else call(N=0)) == 0       # (KE <= N/2, as in the namesake)
    assert call(M=0, A=None, W=None, SA=None, SW=None, D=None) == 0


@pytest.mark.parametrize("call,who,d,nm", ENTRIES)
def test_every_m_is_accepted_as_far_as_the_pointer_checks(call, who, d, nm):
    """No M <= 64 rule here: 1, 64, 65 and 100000 rows pass the shape rules (NULL is what is left to find); arcq_gemm_mxfp4's own limit
    stays."""
    for M in (1, 64, 65, 100000):
        assert call(M=M, A=None) == NULL, M
        _says(call, SHAPE, f"{who}: A, MRW and {d} must be 16-byte aligned", M=M, W=P + 8)
    assert call(M=65535 * 128, A=None) == NULL
    assert call(M=65535 * 128 + 1, A=None) == NULL                         # (the size limit is reported behind a NULL pointer)
    assert call(M=65535 * 128 + 1) == UNSUPPORTED
    said = L().arcq_last_error().decode()
    # ... and it is what arcq_gemm_mxfp4 says about that M
    assert L().arcq_gemm_mxfp4(P, P, P, P, P, 65535 * 128 + 1, 4096, 4224, 1.0, None, None, None, 0, None, 0, None) == UNSUPPORTED
    assert said == who + ": shape too large" and said.replace(who, "arcq_gemm_mxfp4") == L().arcq_last_error().decode()


def test_the_repacked_entry_points_keep_their_m_limit():
    assert L().arcq_gemm_mxfp4_repacked(P, P, P, P, P, 65, 4096, 4224, 1.0, None, None, None, 0, None) == SHAPE
    assert b"M <= 64" in L().arcq_last_error()
    assert L().arcq_gemm_mxfp4_repacked_silu_mul(P, P, P, P, P, 65, 4096, 4224, 1.0, None, None, None) == SHAPE
    assert b"M <= 64" in L().arcq_last_error()


def test_plain_entry_out_dtype_and_residual():
    who = "arcq_gemm_mxfp4_rw"
    _says(_plain, SHAPE, who + ": bad out_dtype 2", out_dtype=2)
    _says(_plain, SHAPE, who + ": bad out_dtype 2", out_dtype=2, M=4096)
    assert _plain(residual=P + 1) == SHAPE and b"residual" in L().arcq_last_error()
    assert _plain(out_dtype=1, A=None) == NULL


def test_quantising_entry_ke_rule_and_sfact():
    who = "arcq_gemm_mxfp4_rw_silu_mul_quantize"
    for KE in (32, 48, 96, -64, 2112):
        _says(_quant, SHAPE, f"{who}: need KE % 64 == 0 and 0 <= KE <= N/2 <= 32767 (N=4096 KE={KE})", KE=KE)
        assert _quant(KE=KE, M=4096) == SHAPE and _quant(KE=KE, M=0) == SHAPE
    assert _quant(N=128, KE=128) == SHAPE and b"KE" in L().arcq_last_error()
    assert _quant(N=65536, KE=64) == SHAPE and b"32767" in L().arcq_last_error()
    for N, KE in ((128, 64), (128, 0), (4096, 2048), (65408, 64)):          # the ends of the ranges: NULL is what is left to find
        assert _quant(N=N, KE=KE, A=None) == NULL, (N, KE)
    _says(_quant, NULL, who + ": NULL pointer", SF=None)
    assert _quant(SF=None, A=P + 8) == NULL                                  # a NULL SFACT where a NULL output is reported
    _says(_quant, SHAPE, who + ": A, MRW and QACT must be 16-byte aligned", SF=P + 1, D=P + 8)   # SFACT itself needs no alignment
    # the namesake's order: the KE rule is reported with the divisibility rules, once N % 128 == 0 holds
    assert _quant(KE=32, A=None) == SHAPE and _quant(K=4160, KE=32) == SHAPE and b"KE" in L().arcq_last_error()
    assert _quant(N=4112, KE=32) == SHAPE and b"N % 128" in L().arcq_last_error()
    same = L().arcq_gemm_mxfp4_silu_mul_quantize(P, P, P, P, P, P, 4, 4096, 4160, 1.0, None, None, 32, None)
    assert same == SHAPE and b"KE" in L().arcq_last_error()


@pytest.mark.parametrize("call,who,d,nm", ENTRIES)
def test_rejection_order(call, who, d, nm):
    """arcq.h: divisibility (then the KE rule), out_dtype, the empty shape, NULL, 16-byte, 4-byte, bias / residual."""
    everything = dict(K=4160, A=None, W=P + 8, SA=P + 2, bias=P + 1)
    assert call(**everything) == SHAPE and b"K % 128" in L().arcq_last_error()
    del everything["K"]
    if call is _quant:
        assert call(KE=32, **everything) == SHAPE and b"KE" in L().arcq_last_error()
    if call is _plain:
        assert call(out_dtype=7, **everything) == SHAPE and b"out_dtype" in L().arcq_last_error()
        assert call(out_dtype=7, M=0) == SHAPE                 # out_dtype ahead of the empty shape
    assert call(M=0, **everything) == 0                        # the empty shape ahead of every pointer rule
    assert call(**everything) == NULL
    del everything["A"]
    assert call(**everything) == SHAPE and b"16-byte" in L().arcq_last_error()
    del everything["W"]
    assert call(**everything) == SHAPE and b"4-byte" in L().arcq_last_error()
    del everything["SA"]
    assert call(**everything) == SHAPE and b"bias" in L().arcq_last_error()


ROUTES = [
    (1, 16, 128, 1), (4, 4096, 4224, 1), (64, 16, 128, 1), (64, 37888, 3712, 1),
    (65, 16, 128, 2), (128, 4096, 4224, 2), (4096, 37888, 3712, 2), (100000, 16, 128, 2),
    (0, 16, 128, 0), (-1, 16, 128, 0), (4, 24, 128, 0), (4, 0, 128, 0), (4, -16, 128, 0), (4, 16, 192, 0), (4, 16, 0, 0), (4, 16, -128, 0),
    (65, 24, 128, 0), (65, 16, 64, 0),
]


@pytest.mark.parametrize("M,N,K,route", ROUTES)
def test_route(M, N, K, route):
    assert L().arcq_gemm_mxfp4_rw_route(M, N, K) == route
    assert mx.mx_rw_route(M, N, K) == route and agemm.mx_rw_route(M, N, K) == route
    # route 1 is exactly where the decode entry point runs
    assert (route == 1) == bool(L().arcq_gemm_mxfp4_repacked_supported(M, N, K))


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


def _cpu_set(M=4, N=128, K=128):
    A, SA = torch.zeros(M, K // 2, dtype=U8), torch.zeros(M, K // 32, dtype=U8)
    MRW, MRSF = agemm.mx_repack_w(torch.zeros(N, K // 2, dtype=U8), torch.zeros(N, K // 32, dtype=U8))
    return A, MRW, SA, MRSF


def test_the_names_are_reachable_from_agemm():
    for name in ("mx_matmul_rw", "matmul_silu_mul_rw", "matmul_silu_mul_quantize_rw", "mx_rw_route"):
        assert getattr(agemm, name) is getattr(mx, name)


@pytest.mark.parametrize("M", [4, 65])
@pytest.mark.parametrize("fn", [mx.mx_matmul_rw, mx.matmul_silu_mul_rw], ids=["plain", "silu_mul"])
def test_mirrors_name_the_broken_argument(fn, M):
    A, MRW, SA, MRSF = _cpu_set(M=M)
    ok = dict(A=A, MRW=MRW, SFA=SA, MRSF=MRSF)
    for name, t in ok.items():
        for bad in _broken(t):
            _raises(name, fn, **{**ok, name: bad}, scale=1.0, N=128)
    _raises("multiple of 128", fn, A[:, :48].contiguous(), MRW, SA, MRSF, 1.0, 128)
    _raises("multiple of 16", fn, A, MRW, SA, MRSF, 1.0, 24)
    _raises("multiple of 16", fn, A, MRW, SA, MRSF, 1.0, 0)
    _raises("do not belong", fn, A, MRW, SA, MRSF, 1.0, 48)
    _raises("do not belong", fn, A, MRW[:-16].contiguous(), SA, MRSF, 1.0, 128)
    _raises("do not belong", fn, A, MRW, SA, torch.cat([MRSF, MRSF]), 1.0, 128)
    _raises("K/32", fn, A, MRW, SA[:, :2].contiguous(), MRSF, 1.0, 128)
    _raises("K/32", fn, A, MRW, SA[:2].contiguous(), MRSF, 1.0, 128)
    bias = torch.zeros(128, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:16]]:
        _raises("bias", fn, A, MRW, SA, MRSF, 1.0, 128, bias=bad)
    out = torch.zeros(M, 128 if fn is mx.mx_matmul_rw else 64, dtype=BF16)
    for bad in list(_broken(out)) + [torch.zeros(M, 8, dtype=BF16)]:
        _raises("out", fn, A, MRW, SA, MRSF, 1.0, 128, out=bad)
    _raises("GPU", fn, A, MRW, SA, MRSF, 1.0, 128, bias=bias, out=out)          # the device check comes last, whatever M is


def test_plain_mirror_out_dtype_and_residual():
    A, MRW, SA, MRSF = _cpu_set(M=65)
    _raises("out_dtype", mx.mx_matmul_rw, A, MRW, SA, MRSF, 1.0, 128, out_dtype=torch.float16)
    res = torch.zeros(65, 128, dtype=BF16)
    for bad in list(_broken(res)) + [res[:2]]:
        _raises("residual", mx.mx_matmul_rw, A, MRW, SA, MRSF, 1.0, 128, residual=bad)
    _raises("GPU", mx.mx_matmul_rw, A, MRW, SA, MRSF, 1.0, 128, residual=res, out_dtype=torch.float32)


@pytest.mark.parametrize("M", [4, 65])
def test_quantising_mirror_names_the_broken_argument(M):
    f = mx.matmul_silu_mul_quantize_rw
    A, MRW, SA, MRSF = _cpu_set(M=M, N=256)
    ok = dict(A=A, MRW=MRW, SFA=SA, MRSF=MRSF)
    for name, t in ok.items():
        for bad in _broken(t):
            _raises(name, f, **{**ok, name: bad}, scale=1.0, N=256, KE=64)
    _raises("multiple of 128", f, A[:, :48].contiguous(), MRW, SA, MRSF, 1.0, 256, 64)
    for N in (192, 16, 0, -128):
        _raises("N=%d" % N, f, A, MRW, SA, MRSF, 1.0, N, 64)
    for KE in (32, -64, 192):
        _raises("KE=%d is not valid" % KE, f, A, MRW, SA, MRSF, 1.0, 256, KE)
    _raises("do not belong", f, A, MRW, SA, MRSF, 1.0, 128, 64)
    _raises("do not belong", f, A, MRW[:-16].contiguous(), SA, MRSF, 1.0, 256, 64)
    _raises("K/32", f, A, MRW, SA[:, :2].contiguous(), MRSF, 1.0, 256, 64)
    bias = torch.zeros(256, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:128]]:
        _raises("bias", f, A, MRW, SA, MRSF, 1.0, 256, 64, bias=bad)
    _raises("GPU", f, A, MRW, SA, MRSF, 1.0, 256, 64, bias=bias)
    _raises("GPU", f, A, MRW, SA, MRSF, 1.0, 256, 0, scale_host=2.0)


# ---- layer and harness keywords -----------------------------------------------------------------------------------------------------
def test_qlinear_layer_keyword_rules():
    from arcquant_amd.qlinear import QLinearLayer
    lin = torch.nn.Linear(128, 32, bias=False)
    idx = torch.arange(128)
    with pytest.raises(ValueError, match="mx_repacked_only"):
        QLinearLayer(lin, 64, idx, quant_type="NVFP4", mx_repacked_only=True)
    with pytest.raises(ValueError, match="mx_repacked_only"):
        QLinearLayer(lin, 64, idx, mx_repacked_only=True)                      # NVFP4 is the default
    for kw in ("repack_for_decode", "repacked_only"):                          # the NVFP4 keywords keep raising for MXFP4, exactly as before
        with pytest.raises(ValueError, match="NVFP4 weight layout"):
            QLinearLayer(lin, 64, idx, quant_type="MXFP4", mx_repacked_only=True, **{kw: True})
    with pytest.raises(RuntimeError, match="GPU"):                             # the keyword itself is accepted: what is left is the device
        QLinearLayer(lin, 64, idx, quant_type="MXFP4", mx_repacked_only=True)
    assert inspect.signature(QLinearLayer.__init__).parameters["mx_repacked_only"].default is False


def test_decoder_model_keyword_rules():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="mx_repacked_only"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, mx_repacked_only=True)                         # NVFP4
    with pytest.raises(ValueError, match="mx_repacked_only"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=False, quant_type="MXFP4", mx_repacked_only=True)
    with pytest.raises(ValueError, match="mx_repacked_only"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, quant_type="MXFP4", mx_repacked_decode=True, mx_repacked_only=True)
    # mx_repacked_decode's own rule and message are what they were
    with pytest.raises(ValueError, match="mx_repacked_decode needs quant_type='MXFP4' and fused=True, and has no form of the quantising"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, quant_type="MXFP4", mx_quantised_epilogue=True, mx_repacked_decode=True)
    for fn in (e2e.bench_decode, e2e.bench_protocol):
        assert inspect.signature(fn).parameters["mx_repacked_only"].default is False
    assert inspect.signature(e2e.DecoderModel.__init__).parameters["mx_repacked_only"].default is False
    assert inspect.signature(e2e.QLinear.mx_repack).parameters["release_reference"].default is False
