"""The MXFP4 fused decode linears (gemm_mx_linear_rw.hip; include/arcq.h "MXFP4 fused decode linear") on the MI355X: each
of the three entry points against the two-launch chain it replaces, in the same process -- mx.rmsnorm_quantize_x or
agemm.mx_reorder_quantize_x, then mx_matmul_repacked / mx.matmul_silu_mul_repacked -- bit for bit (the outputs are compared as bit
patterns, which is torch.equal and also tells -0 from 0 and one NaN from another).  No tolerance is involved."""
import functools

import pytest
import torch

from arcquant_amd import agemm, mx
from tests.util import outlier_activations, random_perm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
MS = (1, 4, 5, 16)

# (KQ, KE): Kp, steps, what it exercises
RMS_SHAPES = [
    (2048, 0),       # 2048, 16 steps (two per wave): no tail
    (2048, 64),      # 2176, 17: two padding blocks, a residual tail
    (2048, 128),     # 2176, 17: no padding
    (3584, 64),      # 3712, 29: the model's shape; a partial MRSF round
    (4096, 128),     # 4224, 33: a second round
]
PLAIN_SHAPES = RMS_SHAPES + [(64, 0), (64, 64)]      # one step, seven idle waves
KINDS = ("rms", "silu", "plain")


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(got, want, what):
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = _bits(got), _bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        first = ", ".join(f"{tuple(i.tolist())}: got {got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}" for i in bad[:5])
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} outputs differ; first {first}")
    assert torch.equal(got, want) or bool(torch.isnan(want).any())


@functools.lru_cache(maxsize=None)
def _weight(N, Kp, seed=0):
    """(MRW, MRSF) of a random MXFP4 weight [N, Kp]: every code, scale bytes 2^-6 .. 2^1."""
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + N + Kp)
    QW = torch.randint(0, 256, (N, Kp // 2), generator=g, device=DEV, dtype=torch.uint8)
    SFW = torch.randint(121, 129, (N, Kp // 32), generator=g, device=DEV, dtype=torch.uint8)
    return agemm.mx_repack_w(QW, SFW)


@functools.lru_cache(maxsize=None)
def _index(KQ, which):
    if which == "reversed":                  # sends every block's gather across the whole row
        return torch.arange(KQ - 1, -1, -1, dtype=torch.int16).to(DEV)
    return random_perm(KQ, 17 + KQ).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(M, KQ, seed=0):
    """X bf16 [M, KQ] with structured outliers and the norm weight, on the GPU; shared and never written."""
    g = torch.Generator().manual_seed(31 * M + KQ + seed)
    x = outlier_activations(M, KQ, 7 * M + KQ + seed) * (torch.randint(0, 2, (M, KQ), generator=g).to(torch.bfloat16) * 2 - 1)
    wn = (1.0 + 0.25 * torch.randn(KQ, generator=g)).to(torch.bfloat16)
    return x.to(DEV), wn.to(DEV)


@functools.lru_cache(maxsize=None)
def _bias(N):
    return (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.5).to(torch.bfloat16).to(DEV)


def _chain(kind, X, Wn, idx, KE, MRW, MRSF, N, scale, **kw):
    """The two launches a fused call replaces (parent-commit operators)."""
    if kind == "plain":
        A, SFA = agemm.mx_reorder_quantize_x(X, idx, KE)
    else:
        A, SFA = mx.rmsnorm_quantize_x(X, Wn, EPS, idx, KE)
    if kind == "silu":
        return mx.matmul_silu_mul_repacked(A, MRW, SFA, MRSF, scale, N, **kw)
    return mx.mx_matmul_repacked(A, MRW, SFA, MRSF, scale, N, **kw)


def _fused(kind, X, Wn, idx, KE, MRW, MRSF, N, scale, **kw):
    if kind == "plain":
        return mx.linear_quantize_repacked(X, idx, KE, MRW, MRSF, scale, N, **kw)
    if kind == "silu":
        return mx.linear_rmsnorm_silu_repacked(X, Wn, EPS, idx, KE, MRW, MRSF, scale, N, **kw)
    return mx.linear_rmsnorm_repacked(X, Wn, EPS, idx, KE, MRW, MRSF, scale, N, **kw)


def _both(kind, M, N, KQ, KE, order="perm", scale=0.5, X=None, **kw):
    Xs, Wn = _inputs(M, KQ)
    X = Xs if X is None else X
    MRW, MRSF = _weight(N, mx.mx_k_padded(KQ + KE))
    idx = _index(KQ, order)
    want = _chain(kind, X, Wn, idx, KE, MRW, MRSF, N, scale, **kw)
    got = _fused(kind, X, Wn, idx, KE, MRW, MRSF, N, scale, **kw)
    _same(got, want, f"{kind} M={M} N={N} KQ={KQ} KE={KE} {order} {sorted(kw)}")


@pytest.mark.parametrize("kind,KQ,KE", [(kind, KQ, KE) for kind in KINDS for KQ, KE in (PLAIN_SHAPES if kind == "plain" else RMS_SHAPES)])
def test_every_shape_and_row_count(kind, KQ, KE):
    """Each K shape of the table at M = 1, 4, 5, 16 and N = 16 (one workgroup), 144 (nine), with a seeded permutation."""
    for M in MS:
        assert mx.linear_fused_supported(mx.SRC_PLAIN if kind == "plain" else mx.SRC_RMSNORM, M, 144, KQ, KE)
        for N in (16, 144):
            _both(kind, M, N, KQ, KE)


@pytest.mark.parametrize("kind", KINDS)
def test_reversed_index(kind):
    """reorder_index = the reversal: every block's gather runs across the whole row; the residual tail is the row's head."""
    for M, (KQ, KE) in ((4, (3584, 64)), (5, (2048, 128))):
        _both(kind, M, 144, KQ, KE, order="reversed")


@pytest.mark.parametrize("kind", KINDS)
def test_more_row_blocks_than_workgroups(kind):
    """A weight whose row-block count exceeds the launch's workgroup count and is no multiple of it: workgroups walk two row blocks, some
    one (the count is the library's own host helper; KQ = 2048 keeps the weight near 10 MB)."""
    KQ, KE = 2048, 0
    k = mx.SRC_PLAIN if kind == "plain" else mx.SRC_RMSNORM
    wgs = mx.linear_fused_workgroups(k, 1 << 20, KQ, KE)            # the resident set: what a launch of many row blocks gets
    assert wgs >= 16
    N = 16 * (wgs + wgs // 4 + 3)
    assert mx.linear_fused_workgroups(k, N, KQ, KE) == wgs and (N // 16) % wgs and N // 16 > wgs
    assert mx.linear_fused_workgroups(k, 144, KQ, KE) == 9
    for M in (4, 16):
        _both(kind, M, N, KQ, KE, bias=_bias(N))


@pytest.mark.parametrize("kind", ("rms", "plain"))
def test_outputs(kind):
    """bf16 and fp32, alpha as host float and as device scalar, bias, residual, residual aliasing D."""
    M, N, KQ, KE = 5, 144, 3584, 64
    alpha = torch.tensor([0.37], dtype=torch.float32, device=DEV)
    res = (torch.randn(M, N, generator=torch.Generator().manual_seed(3)) * 2).to(torch.bfloat16).to(DEV)
    for out_dtype in (torch.bfloat16, torch.float32):
        for scale in (0.5, alpha):
            _both(kind, M, N, KQ, KE, scale=scale, out_dtype=out_dtype)
            _both(kind, M, N, KQ, KE, scale=scale, out_dtype=out_dtype, bias=_bias(N))
            _both(kind, M, N, KQ, KE, scale=scale, out_dtype=out_dtype, bias=_bias(N), residual=res)
    # residual aliasing D (bf16: the residual's dtype): each call adds into its own copy
    X, Wn = _inputs(M, KQ)
    MRW, MRSF = _weight(N, mx.mx_k_padded(KQ + KE))
    idx = _index(KQ, "perm")
    d_want, d_got = res.clone(), res.clone()
    _chain(kind, X, Wn, idx, KE, MRW, MRSF, N, alpha, bias=_bias(N), residual=d_want, out=d_want)
    out = _fused(kind, X, Wn, idx, KE, MRW, MRSF, N, alpha, bias=_bias(N), residual=d_got, out=d_got)
    assert out.data_ptr() == d_got.data_ptr()
    _same(d_got, d_want, f"{kind}: residual aliasing D")
    assert not torch.equal(d_got, res)


def test_silu_outputs():
    """The SiLU form: with and without bias, alpha as host float and as device scalar, into the caller's tensor."""
    M, N, KQ, KE = 5, 144, 3584, 64
    alpha = torch.tensor([0.37], dtype=torch.float32, device=DEV)
    for scale in (0.5, alpha):
        _both("silu", M, N, KQ, KE, scale=scale)
        _both("silu", M, N, KQ, KE, scale=scale, bias=_bias(N))
    X, Wn = _inputs(M, KQ)
    MRW, MRSF = _weight(N, mx.mx_k_padded(KQ + KE))
    out = torch.empty((M, N // 2), dtype=torch.bfloat16, device=DEV)
    got = _fused("silu", X, Wn, _index(KQ, "perm"), KE, MRW, MRSF, N, 0.5, bias=_bias(N), out=out)
    assert got.data_ptr() == out.data_ptr()
    _same(out, _chain("silu", X, Wn, _index(KQ, "perm"), KE, MRW, MRSF, N, 0.5, bias=_bias(N)), "silu: out=")


@pytest.mark.parametrize("kind", KINDS)
def test_edge_values_through_the_image(kind):
    """An all-zero block (scale byte of amax = 0), a row that is one large outlier (the exponent clamp for the plain source; a row the
    norm flattens for the RMSNorm source), tiny values and -0.0 (the sign of zero), in primary and residual blocks."""
    M, N, KQ, KE = 4, 144, 2048, 128
    X = _inputs(M, KQ)[0].clone()
    idx = _index(KQ, "perm").long()
    X[:, idx[32:64]] = 0.0                                   # block 1 of every reordered row
    X[:, idx[KQ - 32:]] = 0.0                                # the last block of the outlier tail: its residual block is zero too
    X[1] = 0.0
    X[1, int(idx[KQ - 70])] = 3.0e38 if kind == "plain" else 6.0e4      # in the tail: the residual of a clamped exponent
    X[2, idx[64:96]] = -0.0
    X[2, int(idx[70])] = 1.0e-38                             # a block whose amax is (nearly) subnormal
    X[3, idx[96:128]] = torch.tensor(-0.0, dtype=torch.bfloat16)
    X[3, int(idx[100])] = -1.5
    assert bool((X.view(torch.int16) == -32768).any())
    _both(kind, M, N, KQ, KE, X=X, **({} if kind == "silu" else {"out_dtype": torch.float32}))
    _both(kind, M, N, KQ, KE, X=X, bias=_bias(N))


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_follows_x(kind):
    """Captured once, replayed with X rewritten in between: each replay is the chain's result on the X of that moment."""
    M, N, KQ, KE = 4, 144, 3584, 64
    Xa, Wn = _inputs(M, KQ)
    Xb = _inputs(M, KQ, seed=5)[0]
    MRW, MRSF = _weight(N, mx.mx_k_padded(KQ + KE))
    idx = _index(KQ, "perm")
    X, bias = Xa.clone(), _bias(N)
    out = torch.empty((M, N // 2 if kind == "silu" else N), dtype=torch.bfloat16, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fused(kind, X, Wn, idx, KE, MRW, MRSF, N, 0.5, bias=bias, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        _fused(kind, X, Wn, idx, KE, MRW, MRSF, N, 0.5, bias=bias, out=out)
    for src in (Xb, Xa, Xb):
        X.copy_(src)
        out.zero_()
        graph.replay()
        _same(out, _chain(kind, src, Wn, idx, KE, MRW, MRSF, N, 0.5, bias=bias), f"{kind}: replay")
    assert not torch.equal(_chain(kind, Xa, Wn, idx, KE, MRW, MRSF, N, 0.5), _chain(kind, Xb, Wn, idx, KE, MRW, MRSF, N, 0.5))


@pytest.mark.parametrize("kind", KINDS)
def test_rows_beyond_m_do_not_matter(kind):
    """M = 5: X is the head of a 16-row buffer; what follows its last row (rows 5 .. 15 of the image's fragment) changes nothing."""
    M, N, KQ, KE = 5, 144, 2048, 64
    buf = torch.empty((16, KQ), dtype=torch.bfloat16, device=DEV)
    buf[:M] = _inputs(M, KQ)[0]
    Wn = _inputs(M, KQ)[1]
    MRW, MRSF = _weight(N, mx.mx_k_padded(KQ + KE))
    idx = _index(KQ, "perm")
    outs = []
    for fill in (0.0, float("nan"), 3.0e38):
        buf[M:] = fill
        outs.append(_fused(kind, buf[:M], Wn, idx, KE, MRW, MRSF, N, 0.5).clone())
    _same(outs[1], outs[0], f"{kind}: NaN behind X")
    _same(outs[2], outs[0], f"{kind}: 3e38 behind X")
    _same(outs[0], _chain(kind, buf[:M], Wn, idx, KE, MRW, MRSF, N, 0.5), f"{kind}: M = 5")
