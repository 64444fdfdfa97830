"""The MXFP4 GEMMs that serve every batch size from the repacked weight (gemm_mx_tile_rw.hip, gemm_mx_slice_rw.hip) on the
MI355X: exact sums of the tile kernel against fp64 that do not go through mx_matmul, the lane map over long K, the independence of MRSF's
padding bytes, bit-equality with the reference-layout GEMMs on the quantisers' output over every epilogue and across the M = 64 / 65
kernel boundary, the quantising epilogue byte for byte, and the layer / harness plumbing of mx_repacked_only."""
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

# the data rule of tests/test_mx_repacked_gpu.py::test_exact_sums: codes of 0, 0.5, 1, -0.5, -1, -0 and exponents 0..2, so a product is a
# multiple of 2^-2 of magnitude <= 16 and the sum over Kp = 8192 stays under 2^17 granules; the budget is 2^20
ALPHABET = np.array([0, 1, 2, 9, 10, 8], dtype=np.uint8)
EXACT_GRANULES = 2.0 ** 20

EXACT = [
    (65, 16, 128),       # one step, 63 clamped A rows, seven clamped row blocks
    (128, 144, 1152),    # nine steps, a second column tile with one live row block
    (65, 128, 4224),     # 33 steps: crosses an MRSF round into a partial one, every byte index (t / 8) % 4
    (129, 272, 8192),    # two full rounds, a 3 x 3 grid
]


def _report(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {got.size} differ; first: " + ", ".join(f"D{tuple(b)} got {got[tuple(b)]!r} want {want[tuple(b)]!r}" for b in bad[:6])


def _padding_mask(N, K):
    """True at the MRSF bytes of steps that do not exist (include/arcq.h), from the index formula."""
    T, R_ = K // 128, -(-(K // 128) // 32)
    m = torch.ones((N // 16, R_, 8, 64, 4), dtype=torch.bool)
    t = torch.arange(T)
    m[:, t // 32, t % 8, :, (t // 8) % 4] = False
    return m.reshape(-1)


def _rw_f32(QA, QB, sa, sb, pad=None):
    """fp32 output of mx_matmul_rw on numpy operands in the reference layout (repacked on the CPU), alpha = 1."""
    A, SFA = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in (QA, sa))
    N, K = QB.shape[0], QB.shape[1] * 2
    MRW, MRSF = agemm.mx_repack_w(torch.from_numpy(np.ascontiguousarray(QB)), torch.from_numpy(np.ascontiguousarray(sb)))
    if pad is not None:
        MRSF = MRSF.clone()
        MRSF[_padding_mask(N, K)] = pad
    assert agemm.mx_rw_route(QA.shape[0], N, K) == 2, "these tests are about the tile kernel"
    D = agemm.mx_matmul_rw(A, MRW.to(DEV), SFA, MRSF.to(DEV), 1.0, N, out_dtype=torch.float32)
    torch.cuda.synchronize()
    return D.cpu().numpy().astype(np.float64)


def _exact_operands(M, N, Kp, seed):
    rng = np.random.default_rng(seed)
    QA = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (M, Kp))])
    QB = R.pack(ALPHABET[rng.integers(0, len(ALPHABET), (N, Kp))])
    sa = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (M, Kp // 32))
    sb = rng.choice(np.array([127, 128, 129], dtype=np.uint8), (N, Kp // 32))
    return QA, QB, sa, sb


@pytest.mark.parametrize("M,N,Kp", EXACT)
def test_exact_sums(M, N, Kp):
    """Random codes of {0, +-0.5, +-1}, exponents 0..2 per (row, block), fp32 output, alpha = 1: bit-equal to the fp64 sum, with no
    reference-layout GEMM in between."""
    QA, QB, sa, sb = _exact_operands(M, N, Kp, 11 * M + 3 * N + Kp)
    want = R.gemm(QA, QB, sa, sb)
    granules = R.abs_gemm(QA, QB, sa, sb).max() / 0.25
    assert granules <= EXACT_GRANULES, f"sum |a||b| reaches 2^{math.log2(granules):.1f} granules"
    assert np.array_equal(np.rint(want / 0.25) * 0.25, want)
    assert len(np.unique(QB, axis=0)) == N and len(np.unique(want)) >= min(want.size, 512) // 4
    got = _rw_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


def test_lane_map_exact_over_long_k():
    """tests/test_mx_repacked_gpu.py::test_lane_map_exact_over_long_k's construction at (80, 32, 4224): one nonzero code per A row, so each
    output is ONE exact product -- a chunk stored to another row or chunk of the LDS image, a mis-ordered K element, or a scale byte taken
    from another step, dword or byte of MRSF is an exactly wrong value.  The nonzeros are spread over all 33 steps."""
    M, N, Kp = 80, 32, 4224
    rng = np.random.default_rng(M * 131 + N * 7 + Kp)
    steps = Kp // 128
    cb = ((np.arange(N)[:, None] * 5 + np.arange(Kp)[None, :] * 3 + (np.arange(N)[:, None] * np.arange(Kp)[None, :]) % 7) % 16).astype(np.uint8)
    sa = (127 + (np.arange(M)[:, None] + 3 * np.arange(Kp // 32)[None, :]) % 7 - 3).astype(np.uint8)
    sb = (127 + (2 * np.arange(N)[:, None] + np.arange(Kp // 32)[None, :]) % 5 - 2).astype(np.uint8)
    QB = R.pack(cb)
    kpos = (np.arange(M) * 53 + 5) % Kp
    assert set(kpos // 128) == set(range(steps)), "some K step holds no row's nonzero"
    assert len(set((kpos % 128) // 32)) == 4, "some 32-block of a step holds no row's nonzero"
    ca = np.zeros((M, Kp), dtype=np.uint8)
    ca[np.arange(M), kpos] = rng.integers(1, 16, M).astype(np.uint8) | 1
    QA = R.pack(ca)
    want = R.gemm(QA, QB, sa, sb)
    assert np.count_nonzero(want) > want.size // 2
    got = _rw_f32(QA, QB, sa, sb)
    assert np.array_equal(got, want), _report(got, want)


def test_padding_bytes_do_not_matter():
    """(65, 48, 4224): 33 steps, so 31 of the second round's 32 step slots are padding, and the tile kernel fetches dwords that hold them.
    0x00 (2^-127) and 0xFE (2^127) in them: equal outputs, and equal to the fp64 sum."""
    M, N, Kp = 65, 48, 4224
    assert int(_padding_mask(N, Kp).sum()) == (N // 16) * 31 * 64
    QA, QB, sa, sb = _exact_operands(M, N, Kp, 5)
    lo, hi = _rw_f32(QA, QB, sa, sb, pad=0x00), _rw_f32(QA, QB, sa, sb, pad=0xFE)
    assert np.array_equal(lo, hi), _report(lo, hi)
    want = R.gemm(QA, QB, sa, sb)
    assert np.array_equal(lo, want), _report(lo, want)


# ---------------------------------------------------------------------------------------------------- bit-equal to the reference layout
MS = (1, 64, 65, 129, 300)
KQ_KE = {128: (64, 64), 1152: (1088, 64), 3840: (3584, 256), 4224: (4096, 64)}
ALPHA = 0.75
_acts, _wts = {}, {}


def _activations(M, Kp, idx):
    """Quantised outlier activations of M rows over this Kp, built once per (M, Kp) and left unchanged (idx = random_perm(KQ, 3) depends on
    Kp alone)."""
    if (M, Kp) not in _acts:
        KQ, KE = KQ_KE[Kp]
        _acts[(M, Kp)] = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, 100 + M).to(DEV), idx, KE)
    return _acts[(M, Kp)]


def _weights(N, Kp):
    if (N, Kp) not in _wts:
        KQ, KE = KQ_KE[Kp]
        g = torch.Generator().manual_seed(N + Kp)
        w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
        idx = random_perm(KQ, 3).to(DEV)
        QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE)
        assert QW.shape == (N, Kp // 2)
        MRW, MRSF = agemm.mx_repack_w(QW, SW)
        _wts[(N, Kp)] = (idx, QW, SW, MRW, MRSF)
    return _wts[(N, Kp)]


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    ai, bi = (t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype)) for t in (a, b))
    assert torch.equal(ai, bi), f"{what}: {int((ai != bi).sum())} of {ai.numel()} elements differ"


@pytest.mark.parametrize("Kp", sorted(KQ_KE))
@pytest.mark.parametrize("N", [16, 144, 1024])
def test_bit_equal_to_mx_matmul(N, Kp):
    """mx_matmul_rw against mx_matmul on the same quantised operands (outlier activations, a random permutation), on both sides of the
    kernel boundary: bf16 and fp32 output, alpha = 0.75 from the host and from the device, bias / residual / both / residual aliasing the
    output.  torch.equal on the bit patterns, every element."""
    idx, QW, SW, MRW, MRSF = _weights(N, Kp)
    g = torch.Generator().manual_seed(N * 3 + Kp)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(DEV)
    dev_alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    for M in MS:
        assert agemm.mx_rw_route(M, N, Kp) == (1 if M <= 64 else 2)
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
            got = agemm.mx_matmul_rw(QX, MRW, SX, MRSF, N=N, **kw)
            _same_bits(got, want, f"M={M} {sorted(k for k in kw if k != 'scale')}")
        # residual aliasing the output
        want = res.clone()
        agemm.mx_matmul(QX, QW, SX, SW, ALPHA, bias=bias, residual=want, out=want)
        got = res.clone()
        r = agemm.mx_matmul_rw(QX, MRW, SX, MRSF, ALPHA, N, bias=bias, residual=got, out=got)
        assert r.data_ptr() == got.data_ptr()
        _same_bits(got, want, f"M={M} residual aliasing out")
        assert not torch.equal(got, res)


@pytest.mark.parametrize("Kp", sorted(KQ_KE))
@pytest.mark.parametrize("N", [16, 144, 1024])
def test_silu_mul_bit_equal(N, Kp):
    """mx.matmul_silu_mul_rw against mx.matmul_silu_mul, with and without bias, every M."""
    idx, QW, SW, MRW, MRSF = _weights(N, Kp)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N + 1)).to(torch.bfloat16).to(DEV)
    for M in MS:
        QX, SX = _activations(M, Kp, idx)
        for kw in (dict(), dict(bias=bias), dict(bias=bias, scale_host=1.5)):
            want = mx.matmul_silu_mul(QX, QW, SX, SW, ALPHA, **kw)
            got = mx.matmul_silu_mul_rw(QX, MRW, SX, MRSF, ALPHA, N, **kw)
            assert got.shape == (M, N // 2)
            _same_bits(got, want, f"M={M} {sorted(kw)}")
        out = torch.full((M, N // 2), float("nan"), dtype=torch.bfloat16, device=DEV)
        assert mx.matmul_silu_mul_rw(QX, MRW, SX, MRSF, ALPHA, N, out=out).data_ptr() == out.data_ptr()
        _same_bits(out, mx.matmul_silu_mul(QX, QW, SX, SW, ALPHA), f"M={M} out=")


# ---------------------------------------------------------------------------------------------------- the quantising epilogue
# M, N, Kp, KE (the operator's argument): the decode kernel with one step / 33 steps and two A fragments / two full rounds and four
# fragments; the tile kernel with one step and with a second row tile of one row, three column tiles, the tail spanning two of them
QUANT = [(1, 128, 128, 0), (17, 256, 4224, 64), (64, 128, 8192, 64), (65, 128, 128, 64), (129, 384, 4224, 128)]
QUANT_KQ_KE = {**KQ_KE, 8192: (8128, 64)}


@pytest.mark.parametrize("M,N,Kp,KE", QUANT)
def test_quantising_epilogue_bytes_equal(M, N, Kp, KE):
    """mx.matmul_silu_mul_quantize_rw against mx.matmul_silu_mul_quantize on the un-repacked weight: codes and scale bytes with torch.equal,
    for a positive, a zero and a negative alpha, host and device, with and without bias."""
    KQ, KE_in = QUANT_KQ_KE[Kp]
    g = torch.Generator().manual_seed(M + N + Kp)
    w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 3).to(DEV)
    QW, SW = agemm.mx_reorder_quantize_w(w, idx, KE_in)
    assert QW.shape == (N, Kp // 2)
    MRW, MRSF = agemm.mx_repack_w(QW, SW)
    QX, SX = agemm.mx_reorder_quantize_x(outlier_activations(M, KQ, M + 5).to(DEV), idx, KE_in)
    bias = (torch.randn(N, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    dev_alpha = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    live = 0
    for kw in (dict(scale=ALPHA), dict(scale=ALPHA, bias=bias), dict(scale=dev_alpha, scale_host=1.5, bias=bias), dict(scale=0.0),
               dict(scale=0.0, bias=bias), dict(scale=-ALPHA), dict(scale=dev_alpha, scale_host=-1.5, bias=bias)):
        want_q, want_s = mx.matmul_silu_mul_quantize(QX, QW, SX, SW, KE=KE, **kw)
        got_q, got_s = mx.matmul_silu_mul_quantize_rw(QX, MRW, SX, MRSF, N=N, KE=KE, **kw)
        what = f"{sorted(k for k in kw if k != 'scale')} scale={kw['scale'] if not isinstance(kw['scale'], torch.Tensor) else 'dev'}"
        _same_bits(got_q, want_q, "codes " + what)
        _same_bits(got_s, want_s, "scale bytes " + what)
        live += int(want_q.any())
    assert live >= 5, "the reference's codes are all zero: the comparison is vacuous"


# ---------------------------------------------------------------------------------------------------- layer and harness
def test_qlinear_layer_repacked_only_equals_plain():
    KQ, N, KE = 1088, 144, 64
    torch.manual_seed(KQ + KE)
    lin = torch.nn.Linear(KQ, N, bias=True).to(torch.bfloat16).to(DEV)
    idx = random_perm(KQ, 5).to(DEV)
    plain = QLinearLayer(lin, KE, idx, quant_type="MXFP4")
    layer = QLinearLayer(lin, KE, idx, quant_type="MXFP4", mx_repacked_only=True)
    assert layer.W is None and layer.scale_w is None and layer.RW is None
    held = sum(b.numel() * b.element_size() for n, b in layer.named_buffers() if n not in ("bias", "scale"))
    assert held == layer.MRW.numel() + layer.MRSF.numel()
    QW, SW = agemm.mx_unrepack_w(layer.MRW, layer.MRSF, N, plain.W.shape[1] * 2)           # the reference pair can be rebuilt
    assert torch.equal(QW, plain.W) and torch.equal(SW, plain.scale_w)
    calls = {}
    for T in (4, 65):                                           # the decode kernel, then the tile kernel
        x = outlier_activations(T, KQ, 6 + T).to(DEV)
        calls[T] = reorder_quantize_x(x, idx, KE, quant_type="MXFP4") + (1, T)
        _same_bits(layer(calls[T]), plain(calls[T]), f"T={T}")
    # both calls really took the one copy: with another weight's MRW both results change
    layer.MRW = torch.zeros_like(layer.MRW)
    for T in (4, 65):
        assert not torch.equal(layer(calls[T]), plain(calls[T])), f"T={T}"


def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toy", num_layers=2, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=512)


_reference_logits = {}


def _reference(e2e, cfg, dev, qe, tok, nxt):
    """Logits of the two-copy-free, flag-off model for the prefill and the decode step, computed once per mx_quantised_epilogue."""
    if qe not in _reference_logits:
        off = e2e.DecoderModel(cfg, 2, 48, dev, fused=True, quant_type="MXFP4", mx_quantised_epilogue=qe)
        _reference_logits[qe] = (off.forward(tok, 0).clone(), off.forward(nxt, 40).clone(), off.weight_bytes())
    return _reference_logits[qe]


@pytest.mark.parametrize("qe", [False, True], ids=["two_launches", "quantised_epilogue"])
def test_decoder_model_flag_gives_equal_logits(qe):
    """DecoderModel(quant_type="MXFP4", fused=True) with and without mx_repacked_only, each with and without mx_quantised_epilogue: a 2 x 40
    prefill (80 tokens: the tile kernel over the repacked weight), an eager decode step and the same step replayed from a HIP graph --
    torch.equal logits each time."""
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, cfg.vocab_size, (2, 40), generator=g).to(dev)
    nxt = torch.randint(0, cfg.vocab_size, (2, 1), generator=g).to(dev)
    with torch.no_grad():
        want_prefill, want, off_bytes = _reference(e2e, cfg, dev, qe, tok, nxt)
        on = e2e.DecoderModel(cfg, 2, 48, dev, fused=True, quant_type="MXFP4", mx_quantised_epilogue=qe, mx_repacked_only=True)
        linears = [v for L in on.layers for v in L.values() if isinstance(v, e2e.QLinear)]
        assert len(linears) == 8 and all(v.W is None and v.SFW is None and v.MRW is not None for v in linears)
        assert on.weight_bytes() == sum(v.MRW.numel() + v.MRSF.numel() for v in linears) + on.lm_head.numel() * 2
        assert on.weight_bytes() >= off_bytes                   # (MRSF is padded to whole rounds of 32 steps)
        assert torch.equal(on.forward(tok, 0), want_prefill)
        assert torch.equal(on.forward(nxt, 40), want)
        on.forward(nxt, 40)
        torch.cuda.synchronize()
        graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                logits = on.forward(nxt, 40)
        torch.cuda.synchronize()
        logits.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(logits, want)
        # the gate|up call really ran over the repacked weight, at both token counts
        on.layers[0]["gateup"].MRW.zero_()
        assert not torch.equal(on.forward(nxt, 40), want)
        assert not torch.equal(on.forward(tok, 0), want_prefill)


def test_bench_decode_reports_the_flag():
    e2e, cfg = _toy()
    e2e.MODEL_CFGS["toy"] = cfg
    try:
        out = e2e.bench_decode("toy", batch=2, prefill=40, steps=2, repeats=1, fused=True, quant_type="MXFP4", mx_repacked_only=True)
    finally:
        del e2e.MODEL_CFGS["toy"]
    assert out["mx_repacked_only"] is True and out["quant_type"] == "MXFP4" and out["decode_tok_per_s"] > 0
    assert out["model_resident_bytes"] > 0 and "mx_repacked_decode" not in out
