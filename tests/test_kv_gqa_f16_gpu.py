"""GPU tests of kvcache.batch_decode_gqa_f16 (arcq_kv_batch_decode_gqa_16bit, kv_decode_gqa16.hip): the g <= 16 query heads of a kv head
in one pass on MFMA over 16-bit pages, element-wise against the fp64 attention over the same pages (tests/kv_reference.py) with the
analytic bound of an MFMA attention whose weights are rounded once to 16 bits (kv_prefill_reference.prefill_bound, T_rows = the sequences'
lengths, a_td = |k_td| / |v_td|).  Every row the tables do not own -- unowned pages, rows past T in a last page, the other layer --
holds NaN, so a kernel that reads one shows it.
Measured on MI355X: max err / bound 0.24 - 0.37 in fp16 and 0.27 - 0.48 in bf16 on randn, 0.09 - 0.19 and 0.10 - 0.24 on the uniform
profile (DESIGN.md 11 "GQA decode over a 16-bit cache")."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
L, LAYER = 2, 1
#   the geometries of test_kv_gqa_gpu.py.  short: one slice, a sequence without positions, T = 1, one position into a second block;
#   long: the kernel's rule splits, an idle-but-for-one-wave sequence among deep loops;  p5: blocks that span 6-7 pages
CASES = {"short": dict(P=16, lens=(0, 1, 33), split=False), "long": dict(P=16, lens=(1500, 2, 700), split=True),
         "p5": dict(P=5, lens=(143, 6, 0), split=False)}
N = 2


@functools.lru_cache(maxsize=None)
def _pages(case, dtype, lens=None):
    """Layer 1 of 2 of a NaN-filled cache behind shuffled tables, as float64 values exact in ``dtype``: randn * 3 rows, or (``lens``
    given) the uniform profile's.  Built once and shared; nothing modifies it."""
    spec = CASES.get(case) or dict(P=16, lens=lens)
    P, lens = spec["P"], spec["lens"]
    pages, indptr, indices, last = R.make_tables(lens, P, seed=len(case) + P)
    gen = torch.Generator().manual_seed(P + sum(lens))
    if case == "uniform":
        data, param = R.rows_to_cache(pages, L, P, (indptr, indices, last), lens, LAYER, *R.profile_rows("uniform", lens, N, seed=sum(lens)), False, dtype)
    else:
        k, v = ((torch.randn(sum(lens), N, 128, generator=gen) * 3).to(dtype).double().numpy() for _ in range(2))
        data, param = np.full((pages, L, 2, N, P, 128), np.nan), np.zeros((pages, L, 2, N, P, 2), dtype=np.float16)
        ones = np.ones((sum(lens), N, 2), dtype=np.float16)
        R.write_rows(data, param, indptr, indices, last, k, v, ones, ones, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), LAYER)
    dev = [torch.from_numpy(data).to(dtype).to(DEV)] + [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (param, indptr, indices, last)]
    return dict(P=P, lens=lens, tables=(indptr, indices, last), data=data, param=param, gen_state=gen.get_state(), dev=dev)


@functools.lru_cache(maxsize=None)
def _case(case, dtype, g, lens=None):
    """The pages + q (randn; zeros for the uniform profile) and the fp64 reference with its bound for g query heads per kv head."""
    c = _pages(case, dtype, lens)
    gen = torch.Generator()
    gen.set_state(c["gen_state"])
    q = torch.randn(len(c["lens"]), g * N, 128, generator=gen).to(dtype)
    if case == "uniform":
        q.zero_()
    ref, (spa, qa) = R.paged_attention_f64(q.double().numpy(), c["data"], c["param"], *c["tables"], LAYER, i4=False)
    T_rows = np.array(c["lens"], dtype=np.float64).reshape(-1, 1, 1)
    return dict(c, q=q.to(DEV), ref=ref, spa=spa, qa=qa, bound=PR.prefill_bound(ref, spa, qa, U[dtype], T_rows))


def _run(c, fn=None):
    """o is rows 1 .. B of a NaN-filled tensor: the rows around it must stay NaN."""
    from arcquant_amd import kvcache
    B = c["q"].shape[0]
    big = torch.full((B + 2,) + tuple(c["q"].shape[1:]), float("nan"), dtype=c["q"].dtype, device=DEV)
    (fn or kvcache.batch_decode_gqa_f16)(big[1:B + 1], c["q"], *c["dev"], LAYER)
    assert torch.isnan(big[0]).all() and torch.isnan(big[-1]).all(), "the rows around o were written"
    return big[1:B + 1]


def _check(c, o, what):
    got = o.double().cpu().numpy()
    err = np.abs(got - c["ref"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.where(c["bound"] > 0, err / c["bound"], np.where(err > 0, np.inf, 0.0)).max())
    print(f"{what}: max err / bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= c["bound"]).all(), f"max err / bound = {worst}"
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


#   test_kv_gqa_gpu.py's: the edges of a 32-position block and of the wave ranges of one slice (32, 64, 96 for T <= 128), one either side,
#   and a split batch whose wave ranges are 96 (T = 1500, S = 5) and 32 (T = 97) positions
UNIFORM_LENS = [(15, 16, 17), (31, 32, 33), (63, 64, 65), (95, 96, 97), (127, 128, 129), (1500, 97, 671)]


@pytest.mark.parametrize("lens", UNIFORM_LENS, ids=lambda t: "-".join(map(str, t)))
@DTYPES
def test_uniform_weights_count_every_position_once(lens, dtype):
    """q = 0: every unrounded weight is exactly 1 and every position weighs 1 / T, so a position dropped, doubled or read from beyond the
    range is an error of order 1 / T.  g = 7."""
    c = _case("uniform", dtype, 7, lens)
    assert not c["qa"].any()
    _check(c, _run(c), f"uniform {lens} {dtype}")


@DTYPES
def test_heads_map_as_batch_decode_maps_them(dtype):
    """g = 7, N = 2, split: besides the bound against fp64, the result agrees with batch_decode_f16's within the sum of the two kernels'
    bounds -- a head or group permutation that a mistake shared with the reference's helpers would hide is O(1) here."""
    from arcquant_amd import kvcache
    c = _case("long", dtype, 7)
    got = _check(c, _run(c), f"heads {dtype}")
    other = _run(c, kvcache.batch_decode_f16).double().cpu().numpy()
    both = c["bound"] + R.decode_bound(c["ref"], c["spa"], c["qa"], U[dtype])
    assert (np.abs(got - other) <= both).all()


def test_graph_replay_is_the_eager_result():
    from arcquant_amd import kvcache
    c = _case("long", BF16, 7)
    eager = _run(c).clone()
    o = torch.empty_like(eager)
    torch.cuda.synchronize()
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        kvcache.batch_decode_gqa_f16(o, c["q"], *c["dev"], LAYER)
    torch.cuda.synchronize()
    for _ in range(2):
        o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), eager.view(torch.int16))
