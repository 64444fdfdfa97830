"""The MXFP4 decoder-layer operators on the MI355X (arcquant_amd/mx.py): the fused RMSNorm quantiser byte for byte
against tests/mx_fused_reference.py, the SiLU*up quantiser byte for byte against the torch pipeline it replaces, the SiLU*up GEMM
epilogue bit for bit against mx_matmul + torch's silu and mul, one concatenated weight against several, one decoder layer of the
harness stage by stage, and the harness plumbing of quant_type="MXFP4"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from arcquant_amd import _lib, agemm, mx
from tests import mx_fused_reference as FR
from tests import mx_reference as R
from tests.test_mx_gpu import _check, deq_torch
from tests.util import bits, from_bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6


def _f32(x_bf16: torch.Tensor) -> np.ndarray:
    return R.bf16_bits_to_f32(bits(x_bf16))


def _norm_weight(KQ, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(KQ, generator=g) * 1.5 + 0.25).to(torch.bfloat16)


def _poisoned(call, rows, KQ, KE, poison):
    """Runs a C-ABI quantiser into outputs pre-filled with `poison` -> (Q, SF) as numpy."""
    Kp = R.k_padded(KQ + KE)
    Q = torch.full((rows, Kp // 2), poison, dtype=torch.uint8, device=DEV)
    SF = torch.full((rows, Kp // 32), poison, dtype=torch.uint8, device=DEV)
    _lib.check(call(Q.data_ptr(), SF.data_ptr()), "fused mx quantiser")
    torch.cuda.synchronize()
    return Q.cpu().numpy(), SF.cpu().numpy()


# -------------------------------------------------------------------------------------------------------------- RMSNorm quantiser
@pytest.mark.parametrize("M", [1, 3, 130, 4096])
@pytest.mark.parametrize("KQ,KE", [(2048, 0), (3584, 64), (3584, 256), (4096, 64), (8192, 64)])
@pytest.mark.parametrize("perm", ["identity", "random"])
def test_rmsnorm_quantiser_bytes_equal_reference(M, KQ, KE, perm):
    X = outlier_activations(M, KQ, 2000 + M + KQ + KE)
    W = _norm_weight(KQ, KQ + KE)
    idx = torch.arange(KQ, dtype=torch.int16) if perm == "identity" else random_perm(KQ, KQ + 7)
    Xd, Wd, idxd = X.to(DEV), W.to(DEV), idx.to(DEV)
    fn = _lib.lib().arcq_mx_rmsnorm_quantize_x

    def call(q, sf):
        return fn(Xd.data_ptr(), Wd.data_ptr(), EPS, idxd.data_ptr(), q, sf, M, KQ, KE, None)

    Q0, S0 = _poisoned(call, M, KQ, KE, 0x00)
    Q1, S1 = _poisoned(call, M, KQ, KE, 0xFF)
    assert np.array_equal(Q0, Q1) and np.array_equal(S0, S1), "some output byte is not written"
    rows = np.arange(M) if M * KQ <= 4096 * 4096 else np.unique(np.r_[np.arange(0, M, 61), M - 1])
    wq, ws = FR.rmsnorm_quantize_x(bits(X)[rows], bits(W), EPS, idx.numpy().astype(np.int64), KE)
    assert np.array_equal(S0[rows], ws), "scale bytes differ"
    assert np.array_equal(Q0[rows], wq), "codes differ"
    Qm, Sm = mx.rmsnorm_quantize_x(Xd, Wd, EPS, idxd, KE)                  # the module allocates and returns the same bytes
    assert np.array_equal(Qm.cpu().numpy(), Q0) and np.array_equal(Sm.cpu().numpy(), S0)
    from arcquant_amd.qlinear import MXFP4_rmsnorm_quantize_x
    qx, sx, one = MXFP4_rmsnorm_quantize_x(Xd, Wd, EPS, idxd, KE)
    assert torch.equal(qx, Qm) and torch.equal(sx, Sm) and one.dim() == 0 and one.item() == 1.0


def test_rmsnorm_quantiser_zero_and_subnormal_rows():
    """An all-zero row (sum of squares 0, rstd = 1 / sqrt(eps): every block zero, scale byte 127) and a row of bf16 subnormals (their
    squares underflow to 0 in fp32 as well; x * w is an fp32 subnormal that rstd lifts into the normal range) among ordinary rows,
    byte for byte against tests/mx_fused_reference.py + R.quantize_x."""
    M, KQ, KE = 6, 2048, 64
    Xb = bits(outlier_activations(M, KQ, 31))
    rng = np.random.default_rng(5)
    Xb[1] = 0
    Xb[4] = rng.integers(1, 0x80, KQ).astype(np.uint16) | (rng.integers(0, 2, KQ).astype(np.uint16) << 15)
    W = _norm_weight(KQ, 9)
    idx = random_perm(KQ, 13)
    rows = FR.normalised_rows(Xb, bits(W), EPS, idx.numpy().astype(np.int64))
    assert np.all(rows[1] == 0) and np.all(np.abs(rows[4]) >= 2.0 ** -126) and len(np.unique(rows[4])) > 100
    wq, ws = FR.rmsnorm_quantize_x(Xb, bits(W), EPS, idx.numpy().astype(np.int64), KE)
    assert np.all(ws[1] == 127) and np.all(wq[1] == 0) and wq[4, KQ // 2:(KQ + KE) // 2].any()
    Xd, Wd, idxd = from_bits(Xb).to(DEV), W.to(DEV), idx.to(DEV)
    fn = _lib.lib().arcq_mx_rmsnorm_quantize_x
    for poison in (0x00, 0xFF):
        Q, S = _poisoned(lambda q, sf: fn(Xd.data_ptr(), Wd.data_ptr(), EPS, idxd.data_ptr(), q, sf, M, KQ, KE, None), M, KQ, KE, poison)
        for r in range(M):
            assert np.array_equal(S[r], ws[r]), f"row {r}: scale bytes differ (poison {poison:#x})"
            assert np.array_equal(Q[r], wq[r]), f"row {r}: codes differ (poison {poison:#x})"


# -------------------------------------------------------------------------------------------------------------- SiLU*up quantiser
@pytest.mark.parametrize("M,KQ,KE", [(4, 18944, 64), (1, 18944, 64), (1, 3584, 64), (8, 512, 64), (300, 2048, 128), (300, 18944, 64)])
def test_silu_mul_quantiser_equals_torch_pipeline(M, KQ, KE):
    """Both layouts against mx_reorder_quantize_x(F.silu(gate) * up): decode-sized M (rows split over blockIdx.y: every element
    gathered from global memory and activated once) and M = 300 (rows staged in LDS); the special values at the ends of exp."""
    g = torch.Generator().manual_seed(7 * M + KQ)
    gu = (torch.randn(M, 2 * KQ, generator=g) * 3).to(torch.bfloat16)
    gu[0, :4] = torch.tensor([0.0, -0.0, 60.0, -60.0]).to(torch.bfloat16)
    gu[0, 4:8] = torch.tensor([-100.0, 100.0, 1e-3, -1e-3]).to(torch.bfloat16)
    gu = gu.to(DEV)
    idx = random_perm(KQ, 43).to(DEV)
    act = (F.silu(gu[:, :KQ]) * gu[:, KQ:]).contiguous()
    want_q, want_sf = agemm.mx_reorder_quantize_x(act, idx, KE)
    pairs = torch.stack((gu[:, :KQ], gu[:, KQ:]), dim=2).reshape(M, 2 * KQ).contiguous()          # g0, u0, g1, u1, ...
    fn = _lib.lib().arcq_mx_silu_mul_quantize_x
    for src, layout in ((gu, agemm.GU_HALVES), (pairs, agemm.GU_PAIRS)):
        got_q, got_sf = mx.silu_mul_quantize_x(src, idx, KE, layout=layout)
        assert torch.equal(got_sf, want_sf), f"scale bytes differ (layout {layout})"
        assert torch.equal(got_q, want_q), f"codes differ (layout {layout})"
        for poison in (0x00, 0xFF):                                         # every byte is written
            Q, S = _poisoned(lambda q, sf: fn(src.data_ptr(), idx.data_ptr(), q, sf, M, KQ, KE, layout, None), M, KQ, KE, poison)
            assert np.array_equal(Q, want_q.cpu().numpy()) and np.array_equal(S, want_sf.cpu().numpy()), (layout, poison)
    # and the reference restatement agrees with the torch pipeline's own bytes
    rq, rs = R.quantize_x(_f32(act), idx.cpu().numpy().astype(np.int64), KE)
    assert np.array_equal(rq, want_q.cpu().numpy()) and np.array_equal(rs, want_sf.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- SiLU*up GEMM epilogue
@pytest.mark.parametrize("M,N,KQ,KE", [(4, 5120, 4096, 64), (17, 176, 3584, 256), (64, 2048, 4096, 64), (65, 2048, 4096, 64),
                                       (129, 37888, 3584, 64), (4096, 37888, 3584, 64)])
def test_silu_mul_gemm_equals_the_unfused_steps(M, N, KQ, KE):
    """mx.matmul_silu_mul == F.silu(y[:, 0::2]) * y[:, 1::2] of y = mx_matmul(...), bit for bit: with and without bias, host and
    device alpha, both kernels (M <= 64 / above) and ragged tiles.  The down projection's quantiser then gives identical bytes from ACT
    and from the torch tensor (where N/2 is a legal KQ of the quantiser, a multiple of 64: every shape here but N = 176)."""
    g = torch.Generator().manual_seed(N + KQ + M)
    w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 3).to(DEV)
    QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE)
    del w
    x = outlier_activations(M, KQ, M + 5).to(DEV)
    QX, SX = agemm.mx_reorder_quantize_x(x, idx, KE)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    idx2 = random_perm(N // 2, 5).to(DEV) if (N // 2) % 64 == 0 else None
    for kw in (dict(scale=0.75), dict(scale=0.75, bias=bias), dict(scale=alpha, scale_host=1.5), dict(scale=alpha, scale_host=1.5, bias=bias)):
        y = agemm.mx_matmul(QX, QW, SX, SW, **kw)
        want = F.silu(y[:, 0::2]) * y[:, 1::2]
        del y
        got = mx.matmul_silu_mul(QX, QW, SX, SW, **kw)
        assert got.shape == (M, N // 2) and got.dtype == torch.bfloat16
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), kw.keys()
        if idx2 is not None:
            (q0, s0), (q1, s1) = agemm.mx_reorder_quantize_x(got, idx2, 64), agemm.mx_reorder_quantize_x(want.contiguous(), idx2, 64)
            assert torch.equal(q0, q1) and torch.equal(s0, s1)
        del want
    out = torch.full((M, N // 2), 7.0, dtype=torch.bfloat16, device=DEV)    # the caller's buffer, every element written
    assert mx.matmul_silu_mul(QX, QW, SX, SW, 0.75, bias=bias, out=out) is out
    ref = mx.matmul_silu_mul(QX, QW, SX, SW, 0.75, bias=bias)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


# -------------------------------------------------------------------------------------------------------------- one weight or several
@pytest.mark.parametrize("M", [4, 300])
def test_concatenated_weight_equals_separate_gemms(M):
    """mx_matmul on the q|k|v weight equals the three separate GEMMs column for column, bit for bit: both kernels accumulate per
    16-column slice / per tile independently of N, which makes the harness's two call structures comparable."""
    KQ, KE, N = 3584, 64, 3584
    g = torch.Generator().manual_seed(M)
    idx = random_perm(KQ, 9).to(DEV)
    ws = [(torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV) for _ in range(3)]
    bs = [(torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(3)]
    x = outlier_activations(M, KQ, 17).to(DEV)
    QX, SX = agemm.mx_reorder_quantize_x(x, idx, KE)
    QW, SW = agemm.mx_reorder_quantize_w(torch.cat(ws), idx, KE)
    for kw, parts in ((dict(), [dict()] * 3), (dict(bias=torch.cat(bs)), [dict(bias=b) for b in bs])):
        for dt in (torch.bfloat16, torch.float32):
            whole = agemm.mx_matmul(QX, QW, SX, SW, 1.0, out_dtype=dt, **kw)
            for i, (w, pk) in enumerate(zip(ws, parts)):
                qw, sw = agemm.mx_reorder_quantize_w(w, idx, KE)
                part = agemm.mx_matmul(QX, qw, SX, sw, 1.0, out_dtype=dt, **pk)
                assert torch.equal(whole[:, i * N:(i + 1) * N], part), (i, dt)


# -------------------------------------------------------------------------------------------------------------- decoder layer
def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("route", ["epilogue", "quantiser"])
def test_mx_decoder_layer_stage_by_stage(route):
    """One decoder layer of DecoderModel(quant_type="MXFP4", fused=True), every arcq stage of _forward_mx re-run by hand on the stage's
    own input and compared bit for bit with its reference (tests/test_e2e_gpu.py says why a chained tolerance is not used):
    the two RMSNorm quantisers against tests/mx_fused_reference.py, the other two against tests/mx_reference.py, each GEMM's fp32
    output within the project's MXFP4 bound of the fp64 dequantised product and its bf16 epilogue bit-exact from that fp32 output.
    The hand chain reproduces forward()'s logits exactly.  Attention is torch's, compared with fp32 math on the CPU within 1e-2.
    Both routes of a decode-sized step's gate|up stage (DecoderModel.mx_decode_route) are walked."""
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy1mx", num_layers=1, num_heads=16, hidden_size=2048, intermediate_size=5632, vocab_size=256,
                          attention_bias=True, mlp_bias=True)
    dev = torch.device(DEV)
    bsz, q_len = 2, 3
    tok = torch.randint(0, cfg.vocab_size, (bsz, q_len), device=dev)
    with torch.no_grad():
        model = e2e.DecoderModel(cfg, bsz, 8, dev, fused=True, quant_type="MXFP4")
        model.mx_decode_route = route
        L = model.layers[0]
        L["ln1"].copy_(_norm_weight(cfg.hidden_size, 1).to(dev))
        L["ln2"].copy_(_norm_weight(cfg.hidden_size, 2).to(dev))
        logits = model.forward(tok, 0)
    h, it, ke, nh = cfg.hidden_size, cfg.intermediate_size, cfg.select_num, cfg.num_heads
    hd, T = h // nh, bsz * q_len
    idx_h, idx_i = model.idx_h.cpu().numpy().astype(np.int64), model.idx_i.cpu().numpy().astype(np.int64)

    def same_bytes(got, want):
        return np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])

    def gemm_stage(qa, sfa, lin, residual=None):
        """-> (fp32 accumulator checked against fp64, the bf16 value the plain epilogue stores, rebuilt from that accumulator)."""
        acc = agemm.mx_matmul(qa, lin.W, sfa, lin.SFW, 1.0, out_dtype=torch.float32)
        _check(acc, deq_torch(qa, sfa) @ deq_torch(lin.W, lin.SFW).T, False)
        y = _bf(_bf(acc) + lin.bias.float())
        if residual is not None:
            y = _bf(y + residual.float())
        return acc, y.to(torch.bfloat16)

    with torch.no_grad():
        hcur = model.embed[tok].reshape(T, h)
        A = mx.rmsnorm_quantize_x(hcur, L["ln1"], cfg.eps, model.idx_h, ke)
        assert same_bytes(A, FR.rmsnorm_quantize_x(bits(hcur), bits(L["ln1"]), cfg.eps, idx_h, ke))
        _, want = gemm_stage(*A, L["qkv"])
        qkv = agemm.mx_matmul(*A[:1], L["qkv"].W, A[1], L["qkv"].SFW, 1.0, bias=L["qkv"].bias)
        assert torch.equal(qkv, want)
        att = model._attention_torch(L, qkv[:, :h], qkv[:, h:2 * h], qkv[:, 2 * h:], qkv, 0, bsz, q_len)
        q, k, v = (qkv[:, i * h:(i + 1) * h].reshape(bsz, q_len, nh, hd).transpose(1, 2).float().cpu() for i in range(3))
        att_cpu = F.scaled_dot_product_attention(q, k, v, is_causal=True).to(torch.bfloat16).transpose(1, 2).reshape(T, h)
        assert float((att.cpu().float() - att_cpu.float()).norm() / att_cpu.float().norm()) < 1e-2
        qa = agemm.mx_reorder_quantize_x(att, model.idx_h, ke)
        assert same_bytes(qa, R.quantize_x(_f32(att), idx_h, ke))
        _, want = gemm_stage(*qa, L["o"], residual=hcur)
        h2 = agemm.mx_matmul(qa[0], L["o"].W, qa[1], L["o"].SFW, 1.0, bias=L["o"].bias, residual=hcur)
        assert torch.equal(h2, want)
        A = mx.rmsnorm_quantize_x(h2, L["ln2"], cfg.eps, model.idx_h, ke)
        assert same_bytes(A, FR.rmsnorm_quantize_x(bits(h2), bits(L["ln2"]), cfg.eps, idx_h, ke))
        Gt = L["gateup"]
        _, gu = gemm_stage(*A, Gt)                                          # interleaved (g0, u0, g1, u1, ...)
        act_want = (F.silu(gu[:, 0::2]) * gu[:, 1::2]).contiguous()
        if route == "epilogue":
            act = mx.matmul_silu_mul(A[0], Gt.W, A[1], Gt.SFW, 1.0, bias=Gt.bias)
            assert torch.equal(act.view(torch.int16), act_want.view(torch.int16))
            qa = agemm.mx_reorder_quantize_x(act, model.idx_i, ke)
        else:
            y = agemm.mx_matmul(A[0], Gt.W, A[1], Gt.SFW, 1.0, bias=Gt.bias)
            assert torch.equal(y, gu)
            qa = mx.silu_mul_quantize_x(y, model.idx_i, ke, layout=agemm.GU_PAIRS)
        assert same_bytes(qa, R.quantize_x(_f32(act_want), idx_i, ke))
        _, want = gemm_stage(*qa, L["down"], residual=h2)
        h3 = agemm.mx_matmul(qa[0], L["down"].W, qa[1], L["down"].SFW, 1.0, bias=L["down"].bias, residual=h2)
        assert torch.equal(h3, want)
        assert torch.equal(model._logits(h3, bsz, q_len), logits)           # the chain above IS what forward() runs


# -------------------------------------------------------------------------------------------------------------- harness plumbing
def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toy", num_layers=2, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=512)


@pytest.mark.parametrize("fused", [True, False])
def test_bench_decode_runs_mxfp4(fused):
    e2e, cfg = _toy()
    e2e.MODEL_CFGS["toy"] = cfg
    try:
        out = e2e.bench_decode("toy", batch=2, prefill=16, steps=2, repeats=1, fused=fused, quant_type="MXFP4")
    finally:
        del e2e.MODEL_CFGS["toy"]
    assert out["quant_type"] == "MXFP4" and out["layers"] == 2
    assert out["decode_tok_per_s"] > 0 and out["decode_ms_per_step_graph"] > 0 and out["prefill_tok_per_s"] > 0
    h, it, ke = cfg.hidden_size, cfg.intermediate_size, cfg.select_num
    per_row = lambda k: R.k_padded(k + ke) // 2 + R.k_padded(k + ke) // 32            # noqa: E731
    want = cfg.num_layers * ((4 * h + 2 * it) * per_row(h) + h * per_row(it)) + cfg.vocab_size * h * 2
    assert out["weight_bytes"] == want


def test_decoder_model_quant_type_plumbing():
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 2, 16, dev, fused=True, repacked_only=True, quant_type="MXFP4")
    tok = torch.randint(0, cfg.vocab_size, (2, 8), generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        for fused in (True, False):
            a = e2e.DecoderModel(cfg, 2, 16, dev, fused=fused).forward(tok, 0)
            b = e2e.DecoderModel(cfg, 2, 16, dev, fused=fused, quant_type="NVFP4").forward(tok, 0)
            assert torch.equal(a, b)
            m = e2e.DecoderModel(cfg, 2, 16, dev, fused=fused, quant_type="MXFP4").forward(tok, 0)
            assert m.shape == a.shape and torch.isfinite(m.float()).all() and not torch.equal(m, a)
