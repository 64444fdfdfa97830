"""GPU tests of the FP8 paged KV cache (arcquant_amd/kvfp8.py; kv_write8.hip, kv_decode_gqa8.hip).  Writers: byte for byte the torch
formula ``quantize_fp8`` on CPU rows, nothing else touched.  Decode: element-wise against the fp64 attention over the dequantised pages
(tests/kv_reference.py) with the analytic bound of an MFMA attention whose weights are rounded once to 16 bits
(kv_prefill_reference.prefill_bound) -- it applies unchanged because the codes convert exactly and the only further roundings are fp32
multiplies by the row scales.  Every row the tables do not own holds the NaN code 0x7F and NaN parameters.
Measured on MI355X: max err / bound 0.25 - 0.35 in fp16 and 0.42 - 0.55 in bf16 on randn; 0.93 - 0.95 and 0.88 - 0.98 against the
uniform profile's far tighter bound (the result's own rounding); 0.23 / 0.33 in the heads test (DESIGN.md 11 "FP8 cache")."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, FP8, U8 = torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.uint8
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
L, LAYER, N = 2, 1, 2
#   test_kv_gqa_f16_gpu.py's geometries
CASES = {"short": dict(P=16, lens=(0, 1, 33), split=False), "long": dict(P=16, lens=(1500, 2, 700), split=True),
         "p5": dict(P=5, lens=(143, 6, 0), split=False)}


def _starts(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@pytest.mark.parametrize("P,lens", [(16, (0, 1, 33)), (5, (143, 6, 1))], ids=["p16", "p5"])
@DTYPES
def test_writers_are_the_torch_formula_byte_for_byte(P, lens, dtype):
    """init of every sequence's first T - 1 positions, then one append, into a cache of 0xA5 bytes and NaN parameters: the whole cache
    equals the CPU formula's rows written by kv_reference.write_rows into the same bytes -- owned rows and everything around them."""
    from arcquant_amd import kvcache
    pages, indptr, indices, last = R.make_tables(lens, P, seed=P)
    st = _starts(lens)
    gen = torch.Generator().manual_seed(P)
    k, v = ((torch.randn(sum(lens), N, 128, generator=gen) * 3).to(dtype) for _ in range(2))
    k[-1, 0], k[-2, 1, 7], v[-1, 1, 3], v[-3, 0, 0:4] = 0.0, torch.finfo(dtype).max, -0.0, 2.0 ** -20     # zero row, dtype max, -0.0, tiny
    data = np.full((pages, L, 2, N, P, 128), 0xA5, dtype=np.uint8)
    param = np.full((pages, L, 2, N, P, 2), np.nan, dtype=np.float16)
    dev = [torch.from_numpy(data).to(DEV).view(FP8), torch.from_numpy(param).to(DEV)]
    # the tables of the sequences one position shorter: the same pages, a last page fewer where T - 1 is a multiple of P
    cnt0 = [(max(T - 1, 0) + P - 1) // P for T in lens]
    indices0 = np.concatenate([indices[indptr[b]:indptr[b] + c] for b, c in enumerate(cnt0)] + [np.zeros(0, np.int32)]).astype(np.int32)
    last0 = np.array([T - 1 - (c - 1) * P if c else 0 for T, c in zip(lens, cnt0)], dtype=np.int32)
    first = torch.tensor([t for b, T in enumerate(lens) for t in range(st[b], st[b] + T - 1)], dtype=torch.long)
    final = torch.tensor([st[b + 1] - 1 if T else 0 for b, T in enumerate(lens)], dtype=torch.long)       # (no position: the token is not written)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                                      # noqa: E731
    kvcache.init_kv_quantize_fp8(*dev, to(_starts(cnt0)), to(indices0), to(last0), k[first].to(DEV), v[first].to(DEV),
                                 to(_starts([max(T - 1, 0) for T in lens])), LAYER)
    kvcache.append_kv_quantize_fp8(*dev, to(indptr), to(indices), to(last), k[final].to(DEV), v[final].to(DEV), LAYER)
    (kc, ks), (vc, vs) = kvcache.quantize_fp8(k), kvcache.quantize_fp8(v)
    pair = [torch.cat([s, torch.zeros_like(s)], -1).numpy() for s in (ks, vs)]
    R.write_rows(data, param, indptr, indices, last, kc.view(U8).numpy(), vc.view(U8).numpy(), pair[0], pair[1], st, LAYER)
    assert torch.equal(dev[0].view(U8).cpu(), torch.from_numpy(data))
    assert torch.equal(dev[1].view(torch.int16).cpu(), torch.from_numpy(param.view(np.int16)))


@functools.lru_cache(maxsize=None)
def _pages(case, dtype, lens=None):
    """Layer 1 of 2 of a cache behind shuffled tables whose unowned rows are NaN codes and NaN parameters, and the same pages dequantised
    to float64 (NaN elsewhere).  randn * 3 rows of ``dtype`` through quantize_fp8; "pow2": those codes under scales 1/32 or 1/16, so every
    value is exact in float16 and bfloat16; "uniform" (``lens`` given): integer codes -15 .. 15, scales in {1/8, 1/4, 1/2}, written
    directly.  Built once and shared; nothing modifies it."""
    from arcquant_amd import kvcache
    spec = CASES.get(case) or (dict(CASES["long"]) if case == "pow2" else dict(P=16, lens=lens))
    P, lens = spec["P"], spec["lens"]
    pages, indptr, indices, last = R.make_tables(lens, P, seed=len(case) + P)
    gen = torch.Generator().manual_seed(P + sum(lens))
    shape = (sum(lens), N, 128)
    if case == "uniform":
        code = [torch.randint(-15, 16, shape, generator=gen).float().to(FP8) for _ in range(2)]
        scale = [(2.0 ** -torch.randint(1, 4, shape[:2] + (1,), generator=gen).float()).to(F16) for _ in range(2)]
    else:
        code, scale = zip(*(kvcache.quantize_fp8((torch.randn(shape, generator=gen) * 3).to(dtype)) for _ in range(2)))
        if case == "pow2":
            scale = [(2.0 ** -torch.randint(4, 6, shape[:2] + (1,), generator=gen).float()).to(F16) for _ in range(2)]
    value = [(c.double() * s.double()).numpy() for c, s in zip(code, scale)]
    pair = [torch.cat([s, torch.zeros_like(s)], -1).numpy() for s in scale]
    ones = np.ones(shape[:2] + (2,), dtype=np.float16)
    data64, raw = np.full((pages, L, 2, N, P, 128), np.nan), np.full((pages, L, 2, N, P, 128), 0x7F, dtype=np.uint8)
    param = np.full((pages, L, 2, N, P, 2), np.nan, dtype=np.float16)
    R.write_rows(data64, np.zeros_like(param), indptr, indices, last, value[0], value[1], ones, ones, _starts(lens), LAYER)
    R.write_rows(raw, param, indptr, indices, last, code[0].view(U8).numpy(), code[1].view(U8).numpy(), pair[0], pair[1], _starts(lens), LAYER)
    dev = [torch.from_numpy(raw).to(DEV).view(FP8)] + [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (param, indptr, indices, last)]
    return dict(P=P, lens=lens, tables=(indptr, indices, last), data=data64, param=param, gen_state=gen.get_state(), dev=dev)


@functools.lru_cache(maxsize=None)
def _case(case, dtype, g, lens=None):
    """The pages + q (randn; zeros for "uniform") and the fp64 reference over the dequantised pages with its bound terms."""
    c = _pages(case, dtype, lens)
    gen = torch.Generator()
    gen.set_state(c["gen_state"])
    q = torch.randn(len(c["lens"]), g * N, 128, generator=gen).to(dtype)
    if case == "uniform":
        q.zero_()
    ref, (spa, qa) = R.paged_attention_f64(q.double().numpy(), c["data"], c["param"], *c["tables"], LAYER, i4=False)
    T_rows = np.array(c["lens"], dtype=np.float64).reshape(-1, 1, 1)
    return dict(c, q=q.to(DEV), ref=ref, spa=spa, qa=qa, bound=PR.prefill_bound(ref, spa, qa, U[dtype], T_rows))


def _run(c, fn=None, dev=None):
    """o is rows 1 .. B of a NaN-filled tensor: the rows around it must stay NaN."""
    from arcquant_amd import kvcache
    B = c["q"].shape[0]
    big = torch.full((B + 2,) + tuple(c["q"].shape[1:]), float("nan"), dtype=c["q"].dtype, device=DEV)
    (fn or kvcache.batch_decode_gqa_fp8)(big[1:B + 1], c["q"], *(dev or c["dev"]), LAYER)
    assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all(), "the rows around o were written"
    return big[1:B + 1]


def _check(c, o, what, bound=None):
    bound = c["bound"] if bound is None else bound
    got = o.double().cpu().numpy()
    err = np.abs(got - c["ref"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())
    print(f"{what}: max err / bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"max err / bound = {worst}"
    for b, T in enumerate(c["lens"]):
        if T == 0:                                             # a sequence without positions: zero bits
            assert not o[b].cpu().view(torch.int16).any(), b
    return got


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("g", [1, 3, 7, 8, 16])
@DTYPES
def test_randn_decode_within_the_bound(case, g, dtype):
    from arcquant_amd import _lib
    c = _case(case, dtype, g)
    ws = _lib.lib().arcq_kv_decode_gqa_workspace_bytes(len(c["lens"]), g * N, N, len(c["tables"][1]), c["P"])
    assert (ws > 0) == CASES[case]["split"], "the slice count of this case changed"
    _check(c, _run(c), f"{case} g={g} {dtype}")


#   one either side of: a score tile inside a block (16), the kernel's 32-position block, the wave ranges of one slice (32, 64, 96 for
#   T <= 128) and the end of its fourth wave (128); and a split batch (S = 4) whose wave ranges are 64 (T = 1000, 671) and 32 (T = 97)
UNIFORM_LENS = [(15, 16, 17), (31, 32, 33), (63, 64, 65), (95, 96, 97), (127, 128, 129), (1000, 97, 671)]


@pytest.mark.parametrize("lens", UNIFORM_LENS, ids=lambda t: "-".join(map(str, t)))
@DTYPES
def test_uniform_weights_count_every_position_once(lens, dtype):
    """q = 0: every score is exactly 0, every scaled weight a power of two, every product a multiple of 1/8 below 8 and T <= 1000: the sums
    are exact in fp32 in any order, so a position dropped, doubled or read from beyond the range is an error of order 1 / T against
    uniform_bound.  g = 7.  The plain fp32 attention over the same values is inside that bound on its own."""
    c = _case("uniform", dtype, 7, lens)
    assert not c["qa"].any() and max(lens) <= 1000
    bound = PR.uniform_bound(c["ref"], U[dtype])
    f32 = R.paged_attention_f32(c["q"].double().cpu().numpy(), c["data"], c["param"], *c["tables"], LAYER, i4=False)
    assert (np.abs(torch.from_numpy(f32).to(dtype).double().numpy() - c["ref"]) <= bound).all()
    _check(c, _run(c), f"uniform {lens} {dtype}", bound)


@DTYPES
def test_heads_map_as_the_16_bit_kernel_maps_them(dtype):
    """g = 7, N = 2, split, scales that are powers of two: the pages dequantise EXACTLY to q's dtype (4 significant bits, |value| in
    2^-14 .. 28), so batch_decode_gqa_f16 over them computes the same attention and the two results differ by at most the two bounds."""
    from arcquant_amd import kvcache
    c = _case("pow2", dtype, 7)
    pages16 = torch.from_numpy(c["data"]).to(dtype)
    own = ~np.isnan(c["data"])
    assert np.array_equal(pages16.double().numpy()[own], c["data"][own])
    got = _check(c, _run(c), f"heads {dtype}")
    other = _run(c, kvcache.batch_decode_gqa_f16, [pages16.to(DEV)] + c["dev"][1:]).double().cpu().numpy()
    assert (np.abs(got - other) <= 2 * c["bound"]).all()


def test_graph_replay_is_the_eager_result():
    from arcquant_amd import kvcache
    c = _case("long", BF16, 7)
    eager = _run(c).clone()
    o = torch.empty_like(eager)
    torch.cuda.synchronize()
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        kvcache.batch_decode_gqa_fp8(o, c["q"], *c["dev"], LAYER)
    torch.cuda.synchronize()
    for _ in range(2):
        o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), eager.view(torch.int16))
