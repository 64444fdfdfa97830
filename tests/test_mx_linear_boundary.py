"""CPU checks of the boundary of the MXFP4 fused decode linears (include/arcq.h "MXFP4 fused decode linear"): the three entry points answer
every violation with its documented status and text before any HIP call (on a machine without a GPU a call that got as far as HIP
would return ARCQ_ERR_LAUNCH instead), in the documented order; arcq_mx_linear_fused_supported from both sides of each limit, the LDS
formula's edge included; the Python wrappers raise from CPU tensors naming the broken argument and refuse the unbroken CPU set last for
living on the CPU; and the DecoderModel keyword follows its rules."""
import pytest
import torch

from arcquant_amd import _lib, agemm, mx

SHAPE, UNSUPPORTED, NULL = -1, -2, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or has no rows)
BF16, U8, I16 = torch.bfloat16, torch.uint8, torch.int16
RMS, PLAIN = mx.SRC_RMSNORM, mx.SRC_PLAIN


def L():
    return _lib.lib()


def _rms(X=P, Wn=P, idx=P, W=P, SW=P, D=P, M=4, N=4608, KQ=3584, KE=64, bias=None, residual=None, out_dtype=0):
    return L().arcq_mx_linear_rmsnorm_repacked(X, Wn, 1e-6, idx, W, SW, D, M, N, KQ, KE, 1.0, None, bias, residual, out_dtype, None)


def _silu(X=P, Wn=P, idx=P, W=P, SW=P, D=P, M=4, N=4608, KQ=3584, KE=64, bias=None, residual=None, out_dtype=0):
    assert residual is None and out_dtype == 0
    return L().arcq_mx_linear_rmsnorm_silu_repacked(X, Wn, 1e-6, idx, W, SW, D, M, N, KQ, KE, 1.0, None, bias, None)


def _plain(X=P, Wn=P, idx=P, W=P, SW=P, D=P, M=4, N=4608, KQ=3584, KE=64, bias=None, residual=None, out_dtype=0):
    return L().arcq_mx_linear_quantize_repacked(X, idx, W, SW, D, M, N, KQ, KE, 1.0, None, bias, residual, out_dtype, None)


ENTRIES = [(_rms, "arcq_mx_linear_rmsnorm_repacked", "D", True), (_silu, "arcq_mx_linear_rmsnorm_silu_repacked", "ACT", True),
           (_plain, "arcq_mx_linear_quantize_repacked", "D", False)]


def _says(call, status, text, **kw):
    assert call(**kw) == status, kw
    assert L().arcq_last_error().decode() == text, kw


@pytest.mark.parametrize("call,who,d,rms", ENTRIES)
def test_rejections_with_status_and_text(call, who, d, rms):
    rng = ", 2048<=KQ<=8192" if rms else "<=32767"
    q = who + ": need KQ%64==0, KE%64==0, 0<=KE<=KQ" + rng + " (rows={M} KQ={KQ} KE={KE})"
    _says(call, SHAPE, q.format(M=4, KQ=3600, KE=64), KQ=3600)
    _says(call, SHAPE, q.format(M=4, KQ=3584, KE=32), KE=32)
    _says(call, SHAPE, q.format(M=4, KQ=3584, KE=3648), KE=3648)
    _says(call, SHAPE, q.format(M=4, KQ=3584, KE=-64), KE=-64)
    _says(call, SHAPE, q.format(M=4, KQ=0, KE=0), KQ=0, KE=0)
    _says(call, SHAPE, q.format(M=-1, KQ=3584, KE=64), M=-1)
    _says(call, SHAPE, q.format(M=4, KQ=32768, KE=64), KQ=32768)
    if rms:
        _says(call, SHAPE, q.format(M=4, KQ=2048 - 64, KE=64), KQ=2048 - 64)
        _says(call, SHAPE, q.format(M=4, KQ=8192 + 64, KE=64), KQ=8192 + 64)
    g = who + ": need M,N >= 0, K % 128 == 0 and N % 16 == 0 (M={M} N={N} K=3712)"
    _says(call, SHAPE, g.format(M=4, N=4600), N=4600)
    _says(call, SHAPE, g.format(M=4, N=-16), N=-16)
    _says(call, SHAPE, g.format(M=0, N=4600), M=0, N=4600)            # an empty call still has to name a valid weight
    for kw in ("X", "idx", "W", "SW", "D") + (("Wn",) if rms else ()):
        _says(call, NULL, who + ": NULL pointer", **{kw: None})
    _says(call, UNSUPPORTED, f"{who}: no fused kernel for this shape: need 1 <= M <= 16 and {mx.linear_fused_lds_bytes(RMS if rms else PLAIN, 3584, 64)} <= "
          "81920 bytes of LDS (M=17 N=4608 KQ=3584 KE=64)", M=17)
    x_text = who + (": X, the norm weight and reorder_index must be 16-byte aligned" if rms else ": X and reorder_index must be 16-byte aligned")
    for kw in ("X", "idx") + (("Wn",) if rms else ()):
        _says(call, SHAPE, x_text, **{kw: P + 8})
    for kw in ("W", "D"):
        _says(call, SHAPE, f"{who}: MRW and {d} must be 16-byte aligned", **{kw: P + 8})
    _says(call, SHAPE, who + ": MRSF must be 4-byte aligned", SW=P + 2)
    _says(call, SHAPE, who + ": bias and residual must be 2-byte aligned", bias=P + 1)
    assert call(M=0) == 0 and call(N=0) == 0
    assert call(M=0, X=None, Wn=None, idx=None, W=None, SW=None, D=None) == 0
    for M in (1, 16):                                        # the ends of the M range pass the shape rules (NULL is what is left to find)
        assert call(M=M, X=None) == NULL


def test_out_dtype_and_residual():
    for call, who in ((_rms, "arcq_mx_linear_rmsnorm_repacked"), (_plain, "arcq_mx_linear_quantize_repacked")):
        _says(call, SHAPE, who + ": bad out_dtype 2", out_dtype=2)
        _says(call, SHAPE, who + ": bias and residual must be 2-byte aligned", residual=P + 1)
        assert call(out_dtype=1, X=None) == NULL


@pytest.mark.parametrize("call,who,d,rms", ENTRIES)
def test_rejection_order(call, who, d, rms):
    """arcq.h: the quantiser's shape rules, the GEMM's, out_dtype, the empty shape, NULL (the quantiser's operands, then the GEMM's),
    unsupported, alignment (the quantiser's operands, the GEMM's 16-byte, 4-byte, bias / residual)."""
    everything = dict(KQ=3600, N=4600, M=17, X=None, W=None, idx=P + 8, D=P + 8, SW=P + 2, bias=P + 1)
    assert call(**everything) == SHAPE and b"KQ%64" in L().arcq_last_error()
    del everything["KQ"]
    assert call(**everything) == SHAPE and b"N % 16" in L().arcq_last_error()
    del everything["N"]
    if call is not _silu:
        assert call(out_dtype=7, **everything) == SHAPE and b"out_dtype" in L().arcq_last_error()
        assert call(out_dtype=7, M=0) == SHAPE                 # out_dtype ahead of the empty shape
    assert call(**{**everything, "M": 0}) == 0                 # the empty shape ahead of every pointer rule
    assert call(**everything) == NULL                          # a NULL X ahead of M = 17
    del everything["X"]
    assert call(**everything) == NULL                          # ... and a NULL MRW too
    del everything["W"]
    assert call(**everything) == UNSUPPORTED and b"M=17" in L().arcq_last_error()      # ahead of every alignment rule
    del everything["M"]
    assert call(**everything) == SHAPE and b"reorder_index must be 16-byte" in L().arcq_last_error()
    del everything["idx"]
    assert call(**everything) == SHAPE and f"MRW and {d} must be 16-byte".encode() in L().arcq_last_error()
    del everything["D"]
    assert call(**everything) == SHAPE and b"4-byte" in L().arcq_last_error()
    del everything["SW"]
    assert call(**everything) == SHAPE and b"bias" in L().arcq_last_error()


def _lds(kind, KQ, KE, rows):
    """The budget formula of include/arcq.h, restated."""
    steps, row = -(-(KQ + KE) // 128), KQ * 9 // 4
    return steps * 1088 + 32 + max(16384, (rows + (kind == RMS)) * row)


def test_supported_from_both_sides_of_each_limit():
    sup = L().arcq_mx_linear_fused_supported
    for kind in (RMS, PLAIN):
        assert sup(kind, 1, 16, 2048, 0) == 1 and sup(kind, 16, 16, 2048, 0) == 1
        assert sup(kind, 0, 16, 2048, 0) == 0 and sup(kind, 17, 16, 2048, 0) == 0
        assert sup(kind, 4, 24, 2048, 0) == 0 and sup(kind, 4, 0, 2048, 0) == 0          # N % 16, N > 0
        assert sup(kind, 4, 16, 2048, 32) == 0 and sup(kind, 4, 16, 2080, 0) == 0 and sup(kind, 4, 16, 2048, 2112) == 0
    assert sup(RMS, 4, 16, 2048 - 64, 0) == 0 and sup(PLAIN, 4, 16, 2048 - 64, 0) == 1
    assert sup(RMS, 4, 16, 8192 + 64, 0) == 0
    assert sup(2, 4, 16, 2048, 0) == 0 and sup(0, 4, 16, 2048, 0) == 0                   # ARCQ_SRC_DYNAMIC has no MXFP4 meaning
    assert mx.linear_fused_supported is agemm.mx_linear_fused_supported
    # the LDS formula: the reported bytes are the formula's at the largest R of 8, 4, 2, 1 that fits, and the edge is where R = 1 stops fitting
    for kind in (RMS, PLAIN):
        edge = None
        for KQ in range(2048, 32768, 64):
            fits = [r for r in (8, 4, 2, 1) if _lds(kind, KQ, 64, r) <= 81920]
            assert bool(sup(kind, 4, 16, KQ, 64)) == (bool(fits) and (kind == PLAIN or KQ <= 8192)), (kind, KQ)
            assert mx.linear_fused_lds_bytes(kind, KQ, 64) == _lds(kind, KQ, 64, fits[0] if fits else 1), (kind, KQ)
            if not fits and edge is None:
                edge = KQ
        assert edge is not None and 4096 < edge <= 8192 + 4096, edge
        assert sup(kind, 4, 16, edge - 64, 64) == 1 and sup(kind, 4, 16, edge, 64) == 0
    assert mx.linear_fused_lds_bytes(RMS, 3584, 64) == _lds(RMS, 3584, 64, 4) == 71904      # the model's shape stages four rows a pass
    # the grid helper: one workgroup per row block up to the resident set
    wg = L().arcq_mx_linear_fused_workgroups
    assert wg(RMS, 16, 3584, 64) == 1 and wg(RMS, 4608, 3584, 64) == 288 and wg(RMS, 37888, 3584, 64) == 512 and wg(PLAIN, 16 * 513, 64, 0) == 512
    assert wg(RMS, 24, 3584, 64) == 0 and wg(RMS, 16, 1024, 0) == 0


# ---- the Python wrappers --------------------------------------------------------------------------------------------------------------
def _raises(pattern, fn, *a, **kw):
    with pytest.raises(RuntimeError, match=pattern):
        fn(*a, **kw)


def _broken(t):
    """dtype, contiguity and rank faults of one tensor."""
    yield t.to(torch.float64)
    yield torch.stack([t, t], dim=-1)[..., 0]
    yield t.unsqueeze(0)


def _cpu_set(M=4, N=32, KQ=2048, KE=64):
    K = mx.mx_k_padded(KQ + KE)
    MRW, MRSF = agemm.mx_repack_w(torch.zeros(N, K // 2, dtype=U8), torch.zeros(N, K // 32, dtype=U8))
    return dict(X=torch.zeros(M, KQ, dtype=BF16), W=torch.ones(KQ, dtype=BF16), reorder_index=torch.arange(KQ, dtype=I16), MRW=MRW, MRSF=MRSF)


def _call(fn, ops, KE=64, N=32, **kw):
    if fn is mx.linear_quantize_repacked:
        return fn(ops["X"], ops["reorder_index"], KE, ops["MRW"], ops["MRSF"], 1.0, N, **kw)
    return fn(ops["X"], ops["W"], 1e-6, ops["reorder_index"], KE, ops["MRW"], ops["MRSF"], 1.0, N, **kw)


@pytest.mark.parametrize("fn", [mx.linear_rmsnorm_repacked, mx.linear_rmsnorm_silu_repacked, mx.linear_quantize_repacked], ids=["rms", "silu", "plain"])
def test_wrappers_name_the_broken_argument(fn):
    ok = _cpu_set()
    names = [n for n in ok if not (n == "W" and fn is mx.linear_quantize_repacked)]
    for name in names:
        for bad in _broken(ok[name]):
            _raises(name, _call, fn, {**ok, name: bad})
    _raises("entries", _call, fn, {**ok, "reorder_index": ok["reorder_index"][:1024].contiguous()})
    if fn is not mx.linear_quantize_repacked:
        _raises("entries", _call, fn, {**ok, "W": ok["W"][:1024].contiguous()})
        small = _cpu_set(KQ=1024)
        _raises("2048 <= KQ", _call, fn, small)
    _raises("KE=32", _call, fn, ok, KE=32)
    _raises("KE=4096", _call, fn, ok, KE=4096)
    _raises("multiple of 16", _call, fn, ok, N=24)
    _raises("multiple of 16", _call, fn, ok, N=0)
    _raises("do not belong", _call, fn, ok, N=48)
    _raises("do not belong", _call, fn, ok, KE=192)                             # (KE = 128 pads to the same Kp as KE = 64)
    _raises("do not belong", _call, fn, {**ok, "MRSF": torch.cat([ok["MRSF"], ok["MRSF"]])})
    _raises("M=17", _call, fn, _cpu_set(M=17))
    _raises("M=0", _call, fn, {**ok, "X": ok["X"][:0]})
    bias = torch.zeros(32, dtype=BF16)
    for bad in list(_broken(bias)) + [bias[:16]]:
        _raises("bias", _call, fn, ok, bias=bad)
    out = torch.zeros(4, 16 if fn is mx.linear_rmsnorm_silu_repacked else 32, dtype=BF16)
    for bad in list(_broken(out)) + [torch.zeros(4, 8, dtype=BF16)]:
        _raises("out", _call, fn, ok, out=bad)
    _raises("GPU", _call, fn, ok, bias=bias, out=out)                           # the device check comes last


@pytest.mark.parametrize("fn", [mx.linear_rmsnorm_repacked, mx.linear_quantize_repacked], ids=["rms", "plain"])
def test_wrapper_out_dtype_and_residual(fn):
    ok = _cpu_set()
    _raises("out_dtype", _call, fn, ok, out_dtype=torch.float16)
    res = torch.zeros(4, 32, dtype=BF16)
    for bad in list(_broken(res)) + [res[:2]]:
        _raises("residual", _call, fn, ok, residual=bad)
    _raises("GPU", _call, fn, ok, residual=res, out_dtype=torch.float32)


# ---- the harness keyword --------------------------------------------------------------------------------------------------------------
def test_decoder_model_keyword_rules():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    cpu = torch.device("cpu")
    mxkw = dict(fused=True, quant_type="MXFP4")
    with pytest.raises(ValueError, match="mx_fused_linears needs mx_repacked_decode or mx_repacked_only"):
        e2e.DecoderModel(cfg, 1, 8, cpu, mx_fused_linears="qkv", **mxkw)
    with pytest.raises(ValueError, match="mx_fused_linears needs"):
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=True, mx_fused_linears="qkv")                                    # NVFP4
    with pytest.raises(ValueError, match="mx_fused_linears needs"):
        e2e.DecoderModel(cfg, 1, 8, cpu, mx_repacked_decode=False, mx_fused_linears="o,gateup", **mxkw)
    with pytest.raises(ValueError, match="subset of 'qkv,o,gateup'"):
        e2e.DecoderModel(cfg, 1, 8, cpu, mx_repacked_only=True, mx_fused_linears="qkv,down", **mxkw)
    with pytest.raises(ValueError, match="no form of the quantising epilogue"):
        e2e.DecoderModel(cfg, 1, 8, cpu, mx_repacked_only=True, mx_quantised_epilogue=True, mx_fused_linears="qkv,gateup", **mxkw)
    with pytest.raises(ValueError, match="mx_repacked_only needs"):                                             # the neighbours' rules still come first
        e2e.DecoderModel(cfg, 1, 8, cpu, fused=False, quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears="qkv")
    assert set(filter(None, e2e.MX_FUSED_LINEARS_DEFAULT.split(","))) <= {"qkv", "o", "gateup"}
    import inspect
    for fn in (e2e.bench_decode, e2e.bench_protocol, e2e.DecoderModel.__init__):
        assert inspect.signature(fn).parameters["mx_fused_linears"].default is None


def test_fused_gateup_refuses_the_quantiser_route():
    """The fused gate|up linear is the "epilogue" decode route's; under the other route forward() raises before any operator runs."""
    from arcquant_amd import e2e
    m = object.__new__(e2e.DecoderModel)
    m.cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=64)
    m.mx_fuse, m.mx_decode_route = frozenset(("gateup",)), "quantiser"
    with pytest.raises(ValueError, match="mx_decode_route='quantiser'"):
        m._forward_mx(torch.zeros((1, 1), dtype=torch.int64), 0)
