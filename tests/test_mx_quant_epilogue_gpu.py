"""The MXFP4 gate|up GEMM that writes the down projection's quantised input (mx.matmul_silu_mul_quantize) on the MI355X:
byte for byte against the two launches it replaces (mx.matmul_silu_mul + mx_reorder_quantize_x with the identity gather), the deployment-time
row order of mx.gate_up_rows against the quantiser's own gather, and the harness flag DecoderModel(mx_quantised_epilogue=True)."""
import numpy as np
import pytest
import torch

from arcquant_amd import _lib, agemm, mx
from tests import mx_reference as R
from tests.util import outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _operands(M, N, KQ, KE_in, seed):
    """Quantised activation and gate|up weight (rows g0, u0, g1, u1, ...) of one shape, and a bias."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 3).to(DEV)
    QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE_in)
    QX, SX = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, M + 5).to(DEV), idx, KE_in)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    return QX, QW, SX, SW, bias


def _variants(bias):
    alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    return (dict(scale=0.75), dict(scale=0.75, bias=bias), dict(scale=alpha, scale_host=1.5), dict(scale=alpha, scale_host=1.5, bias=bias))


def _cabi(QX, QW, SX, SW, KE, poison, scale, scale_host=1.0, bias=None):
    """arcq_gemm_mxfp4_silu_mul_quantize into outputs pre-filled with `poison` -> (codes, scale bytes) as numpy."""
    M, N, K = QX.shape[0], QW.shape[0], QX.shape[1] * 2
    Kp2 = R.k_padded(N // 2 + KE)
    Q = torch.full((M, Kp2 // 2), poison, dtype=torch.uint8, device=DEV)
    SF = torch.full((M, Kp2 // 32), poison, dtype=torch.uint8, device=DEV)
    dev_alpha = isinstance(scale, torch.Tensor)
    st = _lib.lib().arcq_gemm_mxfp4_silu_mul_quantize(QX.data_ptr(), QW.data_ptr(), SX.data_ptr(), SW.data_ptr(), Q.data_ptr(), SF.data_ptr(), M, N, K,
                                                      float(scale_host) * (1.0 if dev_alpha else float(scale)), scale.data_ptr() if dev_alpha else None,
                                                      None if bias is None else bias.data_ptr(), KE, None)
    _lib.check(st, "arcq_gemm_mxfp4_silu_mul_quantize")
    torch.cuda.synchronize()
    return Q.cpu().numpy(), SF.cpu().numpy()


# M, N, KQ, KE_in (the input side's select_num), KE (the operator's argument)
SHAPES = [
    (1, 128, 64, 64, 64),          # one K step: seven idle waves; the whole row is tail; no padding
    (5, 256, 1088, 64, 64),        # Kp = 1152: nine steps over eight waves; K2 = 192 -> Kp2 = 256: two padding blocks
    (16, 640, 4096, 64, 0),        # no tail; Kp2 = 384
    (17, 384, 3584, 256, 128),     # second row-block of the small-M kernel; the tail spans two column slices
    (64, 2176, 4096, 64, 256),     # the last M of the small-M kernel
    (65, 2176, 4096, 64, 256),     # the first M of the tile kernel, ragged rows
    (130, 384, 3584, 256, 128),    # two row tiles; the tail spans two column tiles; padding written by the last tile
    (200, 128, 64, 64, 64),        # tile kernel, one K step, everything tail
]
# seed of the weight and the bias: N + KQ + M, except where that data fails the condition on the reference chain below (the one-row shape
# has four scale bytes in all, and with seed 193 its two blocks share an exponent)
SEEDS = {(1, 128, 64, 64, 64): 206}


@pytest.mark.parametrize("M,N,KQ,KE_in,KE", SHAPES)
def test_bytes_equal_the_two_launch_chain(M, N, KQ, KE_in, KE):
    """(QACT, SFACT) == mx_reorder_quantize_x(mx.matmul_silu_mul(...), arange(N/2), KE) byte for byte, codes and scale bytes compared
    separately, for host / device alpha with and without bias; through the C-ABI into outputs poisoned with 0x00 and with 0xFF (every
    byte is written, padding included) and through the module."""
    QX, QW, SX, SW, bias = _operands(M, N, KQ, KE_in, SEEDS.get((M, N, KQ, KE_in, KE), N + KQ + M))
    KQ2 = N // 2
    ident = torch.arange(KQ2, dtype=torch.int16, device=DEV)
    assert QX.shape[1] * 2 == R.k_padded(KQ + KE_in)
    for kw in _variants(bias):
        want_q, want_s = agemm.mx_reorder_quantize_x(mx.matmul_silu_mul(QX, QW, SX, SW, **kw), ident, KE)
        wq, ws = want_q.cpu().numpy(), want_s.cpu().numpy()
        assert wq.shape == (M, R.k_padded(KQ2 + KE) // 2) and ws.shape == (M, R.k_padded(KQ2 + KE) // 32)
        # the reference chain alone: the comparison below is not vacuous
        assert len(np.unique(ws)) >= 4, f"reference scale bytes take {len(np.unique(ws))} values"
        if KE > 0:
            assert wq[:, KQ2 // 2:(KQ2 + KE) // 2].any(), "the reference's residual codes are all zero"
        q0, s0 = _cabi(QX, QW, SX, SW, KE, 0x00, **kw)
        q1, s1 = _cabi(QX, QW, SX, SW, KE, 0xFF, **kw)
        assert np.array_equal(s0, s1) and np.array_equal(q0, q1), f"some output byte is not written ({sorted(kw)})"
        assert np.array_equal(s0, ws), f"scale bytes differ ({sorted(kw)})"
        assert np.array_equal(q0, wq), f"codes differ ({sorted(kw)})"
        mq, ms = mx.matmul_silu_mul_quantize(QX, QW, SX, SW, kw["scale"], KE, scale_host=kw.get("scale_host", 1.0), bias=kw.get("bias"))
        assert mq.dtype == torch.uint8 and ms.dtype == torch.uint8
        assert torch.equal(ms, want_s) and torch.equal(mq, want_q), f"the module returns other bytes ({sorted(kw)})"


@pytest.mark.parametrize("M,N,KQ,KE_in,KE", [(5, 256, 1088, 64, 64), (65, 2176, 4096, 64, 256)])
def test_bytes_equal_the_two_launch_chain_zero_and_negative_alpha(M, N, KQ, KE_in, KE):
    """alpha = 0 (host and device): every y is +-0, so every activation is +-0 -- scale byte 127 in every block, residual and padding
    included, and the codes carry nothing but the sign of zero; the precondition on distinct scale bytes is replaced by exactly that.
    A negative alpha (host and device, with and without bias) under the usual preconditions.  Chain and fused kernel byte for byte."""
    QX, QW, SX, SW, bias = _operands(M, N, KQ, KE_in, N + KQ + M)
    KQ2 = N // 2
    ident = torch.arange(KQ2, dtype=torch.int16, device=DEV)
    dev = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)       # noqa: E731
    cases = [(True, dict(scale=0.0)), (True, dict(scale=dev(0.0), scale_host=1.5)), (False, dict(scale=-0.75)),
             (False, dict(scale=dev(-0.5), scale_host=1.5, bias=bias)), (False, dict(scale=-0.75, bias=bias))]
    for zero, kw in cases:
        want_q, want_s = agemm.mx_reorder_quantize_x(mx.matmul_silu_mul(QX, QW, SX, SW, **kw), ident, KE)
        wq, ws = want_q.cpu().numpy(), want_s.cpu().numpy()
        if zero:
            assert np.all(ws == 127), "a zero activation has scale byte 127"
            nib = R.unpack(wq[:, :KQ2 // 2])
            assert set(np.unique(nib)) == {0, 8}, "both signs of zero among the reference's codes"
            assert not wq[:, KQ2 // 2:].any(), "the residual of a zero and the padding are +0"
        else:
            assert len(np.unique(ws)) >= 4, f"reference scale bytes take {len(np.unique(ws))} values"
            assert wq[:, KQ2 // 2:(KQ2 + KE) // 2].any(), "the reference's residual codes are all zero"
        q0, s0 = _cabi(QX, QW, SX, SW, KE, 0x00, **kw)
        q1, s1 = _cabi(QX, QW, SX, SW, KE, 0xFF, **kw)
        assert np.array_equal(s0, s1) and np.array_equal(q0, q1), f"some output byte is not written ({sorted(kw)})"
        assert np.array_equal(s0, ws), f"scale bytes differ ({sorted(kw)})"
        assert np.array_equal(q0, wq), f"codes differ ({sorted(kw)})"


@pytest.mark.parametrize("M", [4, 130])
def test_deployment_row_order_equals_the_quantisers_gather(M):
    """The operator on the weight of mx.gate_up_rows(gate, up, reorder_index, ...) == mx_reorder_quantize_x(act, reorder_index, KE) of the
    activation in natural channel order: storing the row pairs in the consumer's order at deployment time replaces its gather exactly."""
    KQ2, KQ, KE_in, KE = 192, 256, 64, 64
    g = torch.Generator().manual_seed(100 + M)
    gate, up = ((torch.randn(KQ2, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV) for _ in range(2))
    gb, ub = ((torch.randn(KQ2, generator=g) * 0.5).to(torch.bfloat16).to(DEV) for _ in range(2))
    reorder = random_perm(KQ2, 11).to(DEV)
    idx = random_perm(KQ, 3).to(DEV)
    QX, SX = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, M + 5).to(DEV), idx, KE_in)
    w_nat, b_nat = mx.gate_up_rows(gate, up, None, gb, ub)
    assert torch.equal(w_nat[0::2], gate) and torch.equal(w_nat[1::2], up) and torch.equal(b_nat[0::2], gb) and torch.equal(b_nat[1::2], ub)
    w_dep, b_dep = mx.gate_up_rows(gate, up, reorder, gb, ub)
    assert torch.equal(w_dep[0::2], gate[reorder.long()]) and torch.equal(b_dep[1::2], ub[reorder.long()])
    assert torch.equal(mx.gate_up_rows(gate, up, reorder), w_dep)
    for with_bias in (False, True):
        QWn, SWn = agemm.mx_reorder_quantize_w(w_nat, idx, KE_in)
        act = mx.matmul_silu_mul(QX, QWn, SX, SWn, 0.75, bias=b_nat if with_bias else None)
        want_q, want_s = agemm.mx_reorder_quantize_x(act, reorder, KE)
        QWd, SWd = agemm.mx_reorder_quantize_w(w_dep, idx, KE_in)
        got_q, got_s = mx.matmul_silu_mul_quantize(QX, QWd, SX, SWd, 0.75, KE, bias=b_dep if with_bias else None)
        assert torch.equal(got_s, want_s), "scale bytes differ"
        assert torch.equal(got_q, want_q), "codes differ"


def _toy():
    """2 layers, intermediate 320, select_num 64, with bias, the existing MXFP4 toy's heads (tests/test_mx_fused_gpu.py).  hidden_size is
    2048, the smallest the harness can run with MXFP4: every layer starts with mx.rmsnorm_quantize_x, whose KQ range is [2048, 8192]."""
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toyq", num_layers=2, num_heads=4, hidden_size=2048, intermediate_size=320, vocab_size=512, select_num=64,
                                attention_bias=True, mlp_bias=True)


def test_harness_flag_gives_the_same_logits():
    """DecoderModel(fused=True, quant_type="MXFP4") with and without mx_quantised_epilogue: equal logits for a prefill of 2 x 40 = 80
    tokens (the tile kernel) and for the decode step that follows it (2 tokens, the small-M kernel)."""
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, cfg.vocab_size, (2, 40), generator=g).to(dev)
    nxt = torch.randint(0, cfg.vocab_size, (2, 1), generator=g).to(dev)
    with torch.no_grad():
        off = e2e.DecoderModel(cfg, 2, 48, dev, fused=True, quant_type="MXFP4")
        on = e2e.DecoderModel(cfg, 2, 48, dev, fused=True, quant_type="MXFP4", mx_quantised_epilogue=True)
        assert not off.mx_quantised_epilogue and on.mx_quantised_epilogue
        for t, pos in ((tok, 0), (nxt, 40)):
            a, b = off.forward(t, pos), on.forward(t, pos)
            assert torch.isfinite(a.float()).all() and torch.equal(a, b), pos


def test_bench_decode_runs_with_the_flag():
    e2e, cfg = _toy()
    e2e.MODEL_CFGS["toyq"] = cfg
    try:
        out = e2e.bench_decode("toyq", batch=2, prefill=16, steps=2, repeats=1, fused=True, quant_type="MXFP4", mx_quantised_epilogue=True)
    finally:
        del e2e.MODEL_CFGS["toyq"]
    assert out["quant_type"] == "MXFP4" and out["mx_quantised_epilogue"] is True and out["layers"] == 2
    assert out["decode_tok_per_s"] > 0 and out["decode_ms_per_step_graph"] > 0 and out["prefill_tok_per_s"] > 0
