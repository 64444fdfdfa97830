"""The MXFP4 decode GEMMs over the repacked weight (gemm_mx_rw.hip) on the MI355X: exact sums against fp64 that do not go
through mx_matmul, bit-equality with the reference-layout GEMMs on the quantisers' output over every epilogue, the lane map over long K,
the independence of MRSF's padding bytes, and the layer / harness plumbing of the opt-in keywords."""
import math

import numpy as np
import pytest
import torch

from arcquant_amd import agemm, mx
from arcquant_amd.qlinear import QLinearLayer, reorder_quantize_x
from tests import mx_reference as R
from tests.util import outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the data rule of tests/test_mx_gemm_exact_gpu.py::test_long_k_exact: codes of 0, 0.5, 1, -0.5, -1, -0 and exponents 0..2, so a product is
# a multiple of 2^-2 of magnitude <= 16 and the sum over Kp = 8192 stays under 2^17 granules; the budget is 2^20
ALPHABET = np.array([0, 1, 2, 9, 10, 8], dtype=np.uint8)
EXACT_GRANULES = 2.0 ** 20

EXACT = [
    (1, 16, 128),        # one step: seven idle waves
    (16, 16, 1152),      # nine steps: wave 0 takes two
    (17, 48, 4096),      # 32 steps: every unroll slot full; second A fragment with 15 clamped rows; odd row-block count
    (33, 48, 4224),      # 33 steps: a partial second round
    (49, 144, 5120),     # 40 steps: every wave runs slot 0 only in the second round; four fragments, the last with one row
    (64, 32, 8192),      # two full rounds, four full A fragments
]


def _report(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {got.size} differ; first: " + ", ".join(f"D{tuple(b)} got {got[tuple(b)]!r} want {want[tuple(b)]!r}" for b in bad[:6])


def _repacked_f32(QA, QB, sa, sb, pad=None):
    """fp32 output of mx_matmul_repacked on numpy operands in the reference layout (repacked on the CPU), alpha = 1."""
    A, SFA = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (QA, sa))
    MRW, MRSF = agemm.mx_repack_w(torch.from_numpy(np.ascontiguousarray(QB)), torch.from_numpy(np.ascontiguousarray(sb)))
    if pad is not None:
        MRSF = _with_padding(MRSF, QB.shape[0], QB.shape[1] * 2, pad)
    D = agemm.mx_matmul_repacked(A, MRW.to(DEV), SFA, MRSF.to(DEV), 1.0, QB.shape[0], out_dtype=torch.float32)
    torch.cuda.synchronize()
    return D.cpu().numpy().astype(np.float64)


def _padding_mask(N, K):
    """True at the MRSF bytes of steps that do not exist (include/arcq.h), from the index formula."""
    T, R_ = K // 128, -(-(K // 128) // 32)
    m = torch.ones((N // 16, R_, 8, 64, 4), dtype=torch.bool)
    t = torch.arange(T)
    m[:, t // 32, t % 8, :, (t // 8) % 4] = False
    return m.reshape(-1)


def _with_padding(MRSF, N, K, value):
    out = MRSF.clone()
    out[_padding_mask(N, K).to(out.device)] = value
    return out


@pytest.mark.parametrize("M,N,Kp", EXACT)
def test_exact_sums(M, N, Kp):
    """Random codes of {0, +-0.5, +-1}, exponents 0..2 per (row, block), fp32 output, alpha = 1: bit-equal to the fp64 sum, with no
    reference-layout GEMM in between."""
    rng = np.random.default_rng(11 * M + 3 * N + Kp)
    QA = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (M, Kp))])
    QB = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (N, Kp))])
    sa = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (M, Kp // 32))
    sb = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (N, Kp // 32))
    want = R.gemm(QA, QB, sa, sb)
    granules = R.abs_gemm(QA, QB, sa, sb).max() / 0.25
    assert granules <= EXACT_GRANULES, f"sum |a||b| reaches 2^{math.log2(granules):.1f} granules"
    assert np.array_equal(np.rint(want / 0.25) * 0.25, want)
    assert len(np.unique(QB, axis=0)) == N and len(np.unique(want)) >= min(want.size, 512) // 4
    got = _repacked_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


def test_lane_map_exact_over_long_k():
    """tests/test_mx_gemm_exact_gpu.py::test_lane_map_exact_over_long_k's construction at (16, 32, 4224): one nonzero code per A row, so
    each output is ONE exact product -- a swapped row, a mis-ordered K element or a scale byte taken from another step, wave slot or lane
    of MRSF is an exactly wrong value.  The passes together put a nonzero into every one of the 33 steps."""
    M, N, Kp = 16, 32, 4224
    rng = np.random.default_rng(M * 131 + N * 7 + Kp)
    steps, passes = Kp // 128, -(-Kp // (37 * M))
    cb = ((np.arange(N)[:, None] * 5 + np.arange(Kp)[None, :] * 3 + (np.arange(N)[:, None] * np.arange(Kp)[None, :]) % 7) % 16).astype(np.uint8)
    sa = (127 + (np.arange(M)[:, None] + 3 * np.arange(Kp // 32)[None, :]) % 7 - 3).astype(np.uint8)
    sb = (127 + (2 * np.arange(N)[:, None] + np.arange(Kp // 32)[None, :]) % 5 - 2).astype(np.uint8)
    QB = R.pack(cb)
    kpos = [(np.arange(M) * 37 + 5 + 37 * M * p) % Kp for p in range(passes)]
    assert set(np.concatenate(kpos) // 128) == set(range(steps)), "some K step holds no row's nonzero"
    for kp in kpos:
        ca = np.zeros((M, Kp), dtype=np.uint8)
        ca[np.arange(M), kp] = rng.integers(1, 16, M).astype(np.uint8) | 1
        QA = R.pack(ca)
        want = R.gemm(QA, QB, sa, sb)
        assert np.count_nonzero(want) > want.size // 2
        got = _repacked_f32(QA, QB, sa, sb)
        assert np.array_equal(got, want), _report(got, want)


def test_padding_bytes_do_not_matter():
    """(33, 48, 4224): 33 steps, so 31 of the second round's 32 step slots are padding.  0x00 (2^-127) and 0xFE (2^127) in them: equal
    outputs, and equal to the fp64 sum."""
    M, N, Kp = 33, 48, 4224
    assert int(_padding_mask(N, Kp).sum()) == (N // 16) * 31 * 64
    rng = np.random.default_rng(5)
    QA = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (M, Kp))])
    QB = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (N, Kp))])
    sa = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (M, Kp // 32))
    sb = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (N, Kp // 32))
    lo, hi = _repacked_f32(QA, QB, sa, sb, pad=0x00), _repacked_f32(QA, QB, sa, sb, pad=0xFE)
    assert np.array_equal(lo, hi), _report(lo, hi)
    want = R.gemm(QA, QB, sa, sb)
    assert np.array_equal(lo, want), _report(lo, want)


# ---------------------------------------------------------------------------------------------------- bit-equal to the reference layout
MS = (1, 4, 16, 17, 48, 64)
KQ_KE = {128: (64, 64), 1152: (1088, 64), 3840: (3584, 256), 4224: (4096, 64)}
ALPHA = 0.75
_acts = {}


def _activations(M, Kp, idx):
    """Quantised outlier activations of M rows over this Kp, built once per (M, Kp) and left unchanged (idx = random_perm(KQ, 3) depends on
    Kp alone)."""
    if (M, Kp) not in _acts:
        KQ, KE = KQ_KE[Kp]
        _acts[(M, Kp)] = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, 100 + M).to(DEV), idx, KE)
    return _acts[(M, Kp)]


def _weights(N, Kp):
    KQ, KE = KQ_KE[Kp]
    g = torch.Generator().manual_seed(N + Kp)
    w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 3).to(DEV)
    QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE)
    assert QW.shape == (N, Kp // 2)
    MRW, MRSF = agemm.mx_repack_w(QW, SW)
    return idx, QW, SW, MRW, MRSF


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    ai, bi = (t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) for t in (a, b))
    assert torch.equal(ai, bi), f"{what}: {int((ai != bi).sum())} of {ai.numel()} elements differ"


@pytest.mark.parametrize("Kp", sorted(KQ_KE))
@pytest.mark.parametrize("N", [16, 144, 1024])
def test_bit_equal_to_mx_matmul(N, Kp):
    """mx_matmul_repacked against mx_matmul on the same quantised operands (outlier activations, a random permutation): bf16 and fp32
    output, alpha = 0.75 from the host and from the device, bias / residual / both / residual aliasing the output.  torch.equal on the bit
    patterns, every element."""
    idx, QW, SW, MRW, MRSF = _weights(N, Kp)
    g = torch.Generator().manual_seed(N * 3 + Kp)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    dev_alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    for M in MS:
        QX, SX = _activations(M, Kp, idx)
        res = (torch.randn(M, N, generator=g) * 4).to(torch.bfloat16).to(DEV)
        variants = [
            dict(scale=ALPHA),
            dict(scale=ALPHA, out_dtype=torch.float32),
            dict(scale=dev_alpha, scale_host=1.5),
            dict(scale=dev_alpha, scale_host=1.5, out_dtype=torch.float32, bias=bias, residual=res),
            dict(scale=ALPHA, bias=bias),
            dict(scale=ALPHA, residual=res),
            dict(scale=ALPHA, bias=bias, residual=res),
        ]
        for kw in variants:
            want = agemm.mx_matmul(QX, QW, SX, SW, **kw)
            got = agemm.mx_matmul_repacked(QX, MRW, SX, MRSF, N=N, **kw)
            _same_bits(got, want, f"M={M} {sorted(k for k in kw if k != 'scale')}")
        # residual aliasing the output
        want = res.clone()
        agemm.mx_matmul(QX, QW, SX, SW, ALPHA, bias=bias, residual=want, out=want)
        got = res.clone()
        r = agemm.mx_matmul_repacked(QX, MRW, SX, MRSF, ALPHA, N, bias=bias, residual=got, out=got)
        assert r.data_ptr() == got.data_ptr()
        _same_bits(got, want, f"M={M} residual aliasing out")
        assert not torch.equal(got, res)


@pytest.mark.parametrize("Kp", sorted(KQ_KE))
@pytest.mark.parametrize("N", [16, 144])
def test_silu_mul_bit_equal(N, Kp):
    """mx.matmul_silu_mul_repacked against mx.matmul_silu_mul, with and without bias, every M."""
    idx, QW, SW, MRW, MRSF = _weights(N, Kp)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N + 1)).to(torch.bfloat16).to(DEV)
    for M in MS:
        QX, SX = _activations(M, Kp, idx)
        for kw in (dict(), dict(bias=bias), dict(bias=bias, scale_host=1.5)):
            want = mx.matmul_silu_mul(QX, QW, SX, SW, ALPHA, **kw)
            got = mx.matmul_silu_mul_repacked(QX, MRW, SX, MRSF, ALPHA, N, **kw)
            assert got.shape == (M, N // 2)
            _same_bits(got, want, f"M={M} {sorted(kw)}")
        out = torch.full((M, N // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
        assert mx.matmul_silu_mul_repacked(QX, MRW, SX, MRSF, ALPHA, N, out=out).data_ptr() == out.data_ptr()
        _same_bits(out, mx.matmul_silu_mul(QX, QW, SX, SW, ALPHA), f"M={M} out=")


# ---------------------------------------------------------------------------------------------------- layer and harness
def test_qlinear_layer_repacked_equals_plain():
    KQ, N, KE = 1088, 144, 64
    torch.manual_seed(KQ + KE)
    lin = torch.nn.Linear(KQ, N, bias=True).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 5).to(DEV)
    plain = QLinearLayer(lin, KE, idx, quant_type="MXFP4")
    layer = QLinearLayer(lin, KE, idx, quant_type="MXFP4", mx_repack_for_decode=True)
    assert plain.MRW is None and layer.MRW.numel() == layer.W.numel() and torch.equal(layer.W, plain.W)
    for T in (4, agemm.MX_REPACKED_MAX_M + 1):                  # the repacked kernel, then mx_matmul
        x = outlier_activations(T, KQ, 6 + T).to(DEV)
        qx, sx, scale = reorder_quantize_x(x, idx, KE, quant_type="MXFP4")
        _same_bits(layer((qx, sx, scale, 1, T)), plain((qx, sx, scale, 1, T)), f"T={T}")
    # the 4-token call really took the repacked weight: with another weight's MRW the result changes, at 65 tokens it does not
    layer.MRW = torch.zeros_like(layer.MRW)
    x = outlier_activations(4, KQ, 10).to(DEV)
    qx, sx, scale = reorder_quantize_x(x, idx, KE, quant_type="MXFP4")
    assert not torch.equal(layer((qx, sx, scale, 1, 4)), plain((qx, sx, scale, 1, 4)))
    x = outlier_activations(65, KQ, 71).to(DEV)
    qx, sx, scale = reorder_quantize_x(x, idx, KE, quant_type="MXFP4")
    _same_bits(layer((qx, sx, scale, 1, 65)), plain((qx, sx, scale, 1, 65)), "T=65 after zeroing MRW")


def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toy", num_layers=2, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=512)


@pytest.mark.parametrize("route", ["epilogue", "quantiser"])
def test_decoder_model_flag_gives_equal_logits(route):
    """DecoderModel(quant_type="MXFP4", fused=True) with and without mx_repacked_decode: a 2 x 8 prefill (16 tokens, over the repacked weight
    too), an eager decode step and the same step replayed from a HIP graph -- torch.equal logits each time, on both decode routes."""
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, cfg.vocab_size, (2, 8), generator=g).to(dev)
    nxt = torch.randint(0, cfg.vocab_size, (2, 1), generator=g).to(dev)
    with torch.no_grad():
        off = e2e.DecoderModel(cfg, 2, 16, dev, fused=True, quant_type="MXFP4")
        on = e2e.DecoderModel(cfg, 2, 16, dev, fused=True, quant_type="MXFP4", mx_repacked_decode=True)
        off.mx_decode_route = on.mx_decode_route = route
        assert on.layers[0]["qkv"].MRW is not None and off.layers[0]["qkv"].MRW is None
        assert on.weight_bytes() == off.weight_bytes()
        assert torch.equal(on.forward(tok, 0), off.forward(tok, 0))
        want = off.forward(nxt, 8)
        assert torch.equal(on.forward(nxt, 8), want)
        on.forward(nxt, 8)
        torch.cuda.synchronize()
        graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                logits = on.forward(nxt, 8)
        torch.cuda.synchronize()
        logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, want)
        # the flag-on step really ran over the repacked weight
        on.layers[0]["down"].MRW.zero_()
        assert not torch.equal(on.forward(nxt, 8), want)


def test_bench_decode_reports_the_flag():
    e2e, cfg = _toy()
    e2e.MODEL_CFGS["toy"] = cfg
    try:
        out = e2e.bench_decode("toy", batch=2, prefill=16, steps=2, repeats=1, fused=True, quant_type="MXFP4", mx_repacked_decode=True)
    finally:
        del e2e.MODEL_CFGS["toy"]
    assert out["mx_repacked_decode"] is True and out["quant_type"] == "MXFP4" and out["decode_tok_per_s"] > 0
