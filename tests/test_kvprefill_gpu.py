"""GPU tests of kvcache.batch_prefill_i4 (include/arcq_kv.h arcq_kv_batch_prefill): causal attention of several query tokens per
sequence over the int4 pages, element-wise against the fp64 attention over the same pages (tests/kv_prefill_reference.py) with the bound

    |got - ref| <= decode_bound(ref, spa, qa, U[dtype], n = T_b) + 2 U[dtype] spa

decode_bound is the decode tests' (tests/kv_reference.py) with n = T_b, the any-order worst case of an fp32 sum of T_b terms, so nothing
here knows the kernel's partition; 2 U spa covers one rounding of each weight p s to the 16-bit type, on the numerator and on a row sum
taken from the rounded or the unrounded weights.

Measured on MI355X, max err / bound over the cases and g in {1, 2, 4, 7}: 0.056 - 0.122 in fp16, 0.124 - 0.252 in bf16; spikes 0 (diagonal)
and 0.05 - 0.21 (first masked position) (DESIGN.md 11 "Prefill").

The cases are (T, n) pairs chosen so that n and T - n straddle multiples of 16 / 32 / 64 / 128 (tests/test_kv_prefill_reference.py);
inputs with controlled scores (the spike profile) turn one position too many -- the first masked one -- or too few -- the query's own --
into an O(1) error.

What reaches below the diagonal and into the wide groups (the teeth of each are measured on the CPU against a numpy
restatement of the algorithm, tests/test_kv_prefill_reference.py):
  uniform   q = 0: exact fp32 sums, held to (U + 2^-21) |ref| + 2^-25 with no room for a position dropped or doubled anywhere.
            Measured max err / bound 0.977 - 0.991 in fp16, 0.978 - 0.996 in bf16: the rounding of the result alone.
  probes    a spike at every block edge at or below every query's own position, another target for every head: the V row, error 0 on
            all 16 runs; "group" takes them through g = 8 .. 130 (16, 8, 4, 2, 1 tokens per tile; two chunks).
  randn     "group" at the same g: 0.114 - 0.137 in fp16, 0.227 - 0.269 in bf16.
  ramps     the running maximum rises in every block (up: 0.017 - 0.115 fp16, 0.094 - 0.182 bf16) or settles in block 0 while the fp16
            weights go subnormal (down: 0.010 - 0.068, 0.057 - 0.149), under the bound above unchanged."""
import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
GS = [1, 2, 4, 7]
SENTINEL = 0xA5


def _kv():
    from arcquant_amd import kvcache
    return kvcache


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _upload(c):
    indptr, indices, last = c["tables"]
    return dict(kv_data=_dev(c["data"]), kv_param=_dev(c["param"]), kv_indptr=_dev(indptr), kv_indices=_dev(indices), last_page_offset=_dev(last))


def _sentinel_like(q):
    return torch.full(q.shape, SENTINEL, dtype=torch.uint8, device=DEV).repeat_interleave(2, dim=-1).view(q.dtype)


def _prefill(c):
    """-> o (sentinel-filled before the call)."""
    q = c["q"].to(DEV)
    o = _sentinel_like(q)
    assert o.shape == q.shape
    out = _kv().batch_prefill_i4(o, q, _dev(c["qo"]), **_upload(c), layer_idx=PR.LAYER)
    assert out is o
    return o


def _check(c, o, dtype, what):
    """Rows of a sequence: inside the bound.  Every other row of o: the sentinel, untouched."""
    got = o.double().cpu().numpy()
    n_rows = int(c["qo"][-1])
    sent = torch.full((1,), SENTINEL, dtype=torch.uint8).repeat(2).view(torch.int16).item()
    assert (o[n_rows:].cpu().view(torch.int16) == sent).all(), "rows at or beyond qo_indptr[B] were written"
    if n_rows == 0:
        return 0.0
    ref, bound = c["ref"][:n_rows], PR.prefill_bound(c["ref"], c["spa"], c["qa"], U[dtype], c["T_rows"])[:n_rows]
    err = np.abs(got[:n_rows] - ref)
    assert np.isfinite(got[:n_rows]).all()
    worst = float((err / bound).max())
    print(f"{what}: max err/bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert (err <= bound).all(), f"{what}: max err / bound = {worst}"
    return worst


@pytest.mark.parametrize("case", list(PR.PREFILL_CASES))
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_within_the_bound(case, g, dtype):
    c = PR.case_inputs(case, dtype, g)
    o = _prefill(c)
    _check(c, o, dtype, f"{case} {dtype} g={g}")


@pytest.mark.parametrize("case", ["chunk", "tiles"])
@pytest.mark.parametrize("mode", ["diagonal", "masked"])
@pytest.mark.parametrize("g", [1, 7])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_controlled_scores(case, mode, g, dtype):
    """Spikes (kv_reference.profile_rows("spike"), q = 8 K_t).  diagonal: every query points at its own position, the last one it may
    attend to: the output is V there.  masked: every query but a sequence's last points at the position after its own, which exists and
    is masked: the output is the fp64 reference's mix of the allowed rows, and a leak would return V at own + 1."""
    c = PR.spike_case(case, dtype, g, mode)
    assert c["gap"] > 60.0, "the target's score must lead by more than 60 for the case to test what it claims"
    assert torch.equal(c["q"].double().to(dtype).double(), c["q"].double())
    o = _prefill(c)
    _check(c, o, dtype, f"spike {mode} {case} {dtype} g={g}")
    if mode == "diagonal":
        got = o.double().cpu().numpy()
        for b, (T, n) in enumerate(zip(c["lens"], c["new"])):
            for i in PR.edge_queries(T, n) if n else ():
                r = c["qo"][b] + i
                for h in range(g * c["N"]):
                    want = torch.from_numpy(c["V"][c["start"][b] + c["own"][r], h // g]).to(dtype).double().numpy()
                    assert np.abs(got[r, h] - want).max() <= 2 * U[dtype] * np.abs(want).max() + 1e-6, (b, i, h)


@pytest.mark.parametrize("case,g", PR.UNIFORM_RUNS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_uniform_exact_sums(case, g, dtype):
    """q = 0: every allowed score is exactly 0 and every weight 1, so the numerator, the zero sum and the row sum are sums of multiples
    of 1/8, 1/16 and 1 below 2^24 units -- exact in fp32 in ANY order (premises asserted on the pages) -- and what is left is 1 / l, one
    product and the store:  |got - ref| <= (U + 2^-21) |ref| + 2^-25  (kv_prefill_reference.uniform_bound), no spa term and no n term.
    One position dropped, doubled, let through or masked early, or V codes in the unswapped position order, overshoots it by
    5e5 - 4e7 (tests/test_kv_prefill_reference.py)."""
    c = PR.profile_case(case, "uniform", dtype, g)
    PR.uniform_premises(c)
    o = _prefill(c)
    _check(c, o, dtype, f"uniform {case} {dtype} g={g} (any-order bound)")
    n_rows = int(c["qo"][-1])
    got, ref = o.double().cpu().numpy()[:n_rows], c["ref"][:n_rows]
    err, bound = np.abs(got - ref), PR.uniform_bound(ref, U[dtype])
    worst = float((err / bound).max())
    print(f"uniform {case} {dtype} g={g}: max err/exact-sum bound = {worst:.3f}")
    assert (err <= bound).all(), f"uniform {case} {dtype} g={g}: max err / bound = {worst}"


@pytest.mark.parametrize("case,g", PR.PROBE_RUNS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_interior_probes(case, g, dtype):
    """A spike at every block edge below the diagonal (kv_prefill_reference.probe_case): head h of query row i points at another of
    0, the multiples of 32, the position before each, own - 1 and own, so neighbouring heads (and mostly neighbouring tokens) expect different V rows.  Every
    (row, head) is its target's V row."""
    c = PR.probe_case(case, dtype, g)
    assert c["gap"] > 60.0, "the target's score must lead by more than 60 for the case to test what it claims"
    assert torch.equal(c["q"].double().to(dtype).double(), c["q"].double())
    o = _prefill(c)
    _check(c, o, dtype, f"probes {case} {dtype} g={g}")
    ok = PR.probe_rows_ok(o.double().cpu().numpy(), c, dtype, U[dtype])
    assert ok.all(), f"{int((~ok).sum())} of {ok.size} (row, head) pairs are not their target's V row, first {np.argwhere(~ok)[:4].tolist()}"


@pytest.mark.parametrize("g", PR.WIDE_GS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_wide_groups_within_the_bound(g, dtype):
    """randn rows under the wide groups: 16, 8, 4, 2 and 1 tokens per tile, and at g = 130 two chunks, the second with 2 live heads."""
    c = PR.case_inputs("group", dtype, g)
    _check(c, _prefill(c), dtype, f"group {dtype} g={g}")


@pytest.mark.parametrize("case,profile,g", PR.RAMP_RUNS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_batch_prefill_ramps(case, profile, g, dtype):
    """ramp_up: a query's running maximum rises in every block, so l, the zero sum and the 64 accumulators rescale on each trip.
    ramp_down: it settles in block 0, the rescale is skipped for the rest of the loop and the fp16 weights pass through the subnormal
    range.  Under prefill_bound as it is."""
    c = PR.profile_case(case, profile, dtype, g)
    _check(c, _prefill(c), dtype, f"{profile} {case} {dtype} g={g}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_one_query_token_per_sequence_agrees_with_decode(dtype):
    """n_b = 1 everywhere is batch_decode_i4's contract: both are within their bounds of the same reference (not bitwise equal: the
    prefill rounds its weights to the 16-bit type)."""
    kv = _kv()
    g = 2
    c = R.profile_case("ragged", "uniform", True, dtype, g)
    spec = R.CASES["ragged"]
    gen = torch.Generator().manual_seed(7)
    B = len(spec["lens"])
    q = torch.randn(B, g * spec["N"], 128, generator=gen).to(dtype)
    indptr, indices, last = c["tables"]
    ref, (spa, qa) = R.paged_attention_f64(q.double().numpy(), c["data"], c["param"], indptr, indices, last, c["layer"])
    tabs = dict(kv_data=_dev(c["data"]), kv_param=_dev(c["param"]), kv_indptr=_dev(indptr), kv_indices=_dev(indices), last_page_offset=_dev(last))
    od, op = torch.empty_like(q, device=DEV), torch.empty_like(q, device=DEV)
    kv.batch_decode_i4(od, q.to(DEV), **tabs, layer_idx=c["layer"])
    kv.batch_prefill_i4(op, q.to(DEV), torch.arange(B + 1, dtype=torch.int32, device=DEV), **tabs, layer_idx=c["layer"])
    T_rows = np.array(spec["lens"], dtype=np.float64).reshape(-1, 1, 1)
    bd = R.decode_bound(ref, spa, qa, U[dtype])
    bp = PR.prefill_bound(ref, spa, qa, U[dtype], T_rows)
    ed, ep = np.abs(od.double().cpu().numpy() - ref), np.abs(op.double().cpu().numpy() - ref)
    print(f"decode agreement {dtype}: decode err/bound = {(ed / bd).max():.3f}, prefill err/bound = {(ep / bp).max():.3f}")
    assert (ed <= bd).all() and (ep <= bp).all()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_unwritten_rows_and_graph_replay(dtype):
    """Rows of o at or beyond qo_indptr[B] keep their sentinel; a sequence without query tokens between two that have some leaves its
    neighbours' rows alone (every row of o belongs to exactly one sequence, so a row written twice or by the wrong sequence misses the
    bound); the call replays from a graph capture three times with identical output."""
    g = 4
    c = PR.case_inputs("chunk", dtype, g)
    assert c["new"][3] == 0 and c["new"][4] == 0 and c["ntok"] == int(c["qo"][-1]) + PR.PAD_ROWS
    eager = _prefill(c)
    _check(c, eager, dtype, f"eager chunk {dtype}")
    # a batch with the empty-handed sequence in the middle: (100, 37) (40, 0) (65, 33)
    lens, new = [100, 40, 65], [37, 0, 33]
    pages, indptr, indices, last = R.make_tables(lens, 16, seed=3)
    gen = torch.Generator().manual_seed(11)
    sl = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k, v = (torch.randn(sum(lens), 2, 128, generator=gen) * 3).to(dtype), (torch.randn(sum(lens), 2, 128, generator=gen) * 3).to(dtype)
    (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
    data = np.full((pages, 2, 2, 2, 16, 64), SENTINEL, dtype=np.uint8)
    param = np.zeros((pages, 2, 2, 2, 16, 2), dtype=np.float16)
    param.view(np.uint8)[...] = SENTINEL
    R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), sl, 1)
    qo = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    q = torch.randn(int(qo[-1]) + 2, 2 * g, 128, generator=gen).to(dtype)
    ref, (spa, qa) = PR.paged_prefill_f64(q.double().numpy(), qo, data, param, indptr, indices, last, 1)
    T_rows = np.zeros((q.shape[0], 1, 1))
    for b, T in enumerate(lens):
        T_rows[qo[b]:qo[b + 1]] = T
    mid = dict(qo=qo, q=q, tables=(indptr, indices, last), data=data, param=param, ref=ref, spa=spa, qa=qa, T_rows=T_rows)
    _check(mid, _prefill(mid), dtype, f"middle sequence without query tokens {dtype}")

    # graph capture: no workspace, no state, no host read of a table
    kv = _kv()
    qd, qo_d, tabs = c["q"].to(DEV), _dev(c["qo"]), _upload(c)
    o = _sentinel_like(qd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kv.batch_prefill_i4(o, qd, qo_d, **tabs, layer_idx=PR.LAYER)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            kv.batch_prefill_i4(o, qd, qo_d, **tabs, layer_idx=PR.LAYER)
    torch.cuda.synchronize()
    for _ in range(3):
        o.copy_(_sentinel_like(qd))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), eager.view(torch.int16))
