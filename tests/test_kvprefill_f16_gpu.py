"""GPU tests of kvcache.batch_prefill_f16 (arcq_kv_batch_prefill_16bit, kv_prefill16.hip) against fp64 attention over the cache's values,
each query row over the positions it may attend to.  Tables: kv_prefill_reference.case_geometry; every row they do not own (unowned
pages, rows past T in a last page, the other layer) holds NaN, so a kernel that reads one shows it.
Measured on MI355X: max err / bound 0.23 - 0.44 in fp16, 0.37 - 0.50 in bf16; probes max |err| = 0 on all eight runs (DESIGN.md 11 "Prefill
over a 16-bit cache")."""
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
SENTINEL = -1024.0                     # (exact in fp16 and bf16, and no result: |V| stays below 128)


def _attention_f64(q, qo, data, tables, N):
    """fp64 causal attention over the float64 cache ``data`` -> (out, spa, qa) of kv_prefill_reference.prefill_bound with
    a_td = |k_td| / |v_td| (kv_reference.decode_bound); rows of no sequence stay zero."""
    g, param = q.shape[1] // N, np.zeros(data.shape[:-1] + (2,), dtype=np.float16)
    lens = R.seq_lens(tables[0], tables[2], data.shape[4])
    out, spa, qa = np.zeros(q.shape), np.zeros(q.shape), np.zeros(q.shape[:2])
    for b, T in enumerate(lens):
        for n in range(N if qo[b + 1] > qo[b] else 0):
            K, V = (R.gather_rows(data, param, *tables, PR.LAYER, b, n, which)[0] for which in (0, 1))
            for r in range(qo[b], qo[b + 1]):
                end, hs = T - (qo[b + 1] - r) + 1, slice(n * g, (n + 1) * g)           # positions 0 .. end - 1
                sc = (q[r, hs] @ K[:end].T) * R.SM_SCALE
                p = np.exp(sc - sc.max(-1, keepdims=True))
                p /= p.sum(-1, keepdims=True)
                out[r, hs], spa[r, hs] = p @ V[:end], p @ np.abs(V[:end])
                qa[r, hs] = R.SM_SCALE * (np.abs(q[r, hs]) @ np.abs(K[:end]).T).max(-1)
    return out, spa, qa


def _cache(case, k, v):
    """float64 pages [pages, L, 2, N, P, 128] of a case: rows k, v [sum lens, N, 128] in layer 1, NaN everywhere else."""
    spec, lens, _, _, pages, tables = PR.case_geometry(case)
    data = np.full((pages, PR.L, 2, spec["N"], spec["P"], 128), np.nan)
    ones = np.ones(k.shape[:2] + (2,), dtype=np.float16)
    R.write_rows(data, np.zeros(data.shape[:-1] + (2,), dtype=np.float16), *tables, k, v, ones, ones, np.concatenate([[0], np.cumsum(lens)]), PR.LAYER)
    return data


@functools.lru_cache(maxsize=None)
def _randn_case(case, dtype, g):
    spec, lens, _, qo, _, tables = PR.case_geometry(case)
    gen = torch.Generator().manual_seed(spec["P"] + sum(lens) + len(case))
    k, v = ((torch.randn(sum(lens), spec["N"], 128, generator=gen) * 3).to(dtype).double().numpy() for _ in range(2))
    q = torch.randn(int(qo[-1]) + PR.PAD_ROWS, g * spec["N"], 128, generator=gen).to(dtype)
    data = _cache(case, k, v)
    ref, spa, qa = _attention_f64(q.double().numpy(), qo, data, tables, spec["N"])
    T_rows = np.zeros((q.shape[0], 1, 1))
    for b, T in enumerate(lens):
        T_rows[qo[b]:qo[b + 1]] = T
    return dict(q=q, qo=qo, data=data, tables=tables, bound=PR.prefill_bound(ref, spa, qa, U[dtype], T_rows), ref=ref)


def _args(c, dtype):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    data = torch.from_numpy(c["data"]).to(dtype).to(DEV)
    return dict(q=c["q"].to(DEV), qo_indptr=dev(c["qo"]), kv_data=data, kv_param=torch.zeros(data.shape[:-1] + (2,), dtype=F16, device=DEV),
                kv_indptr=dev(c["tables"][0]), kv_indices=dev(c["tables"][1]), last_page_offset=dev(c["tables"][2]), layer_idx=PR.LAYER)


def _run(c, dtype):
    """-> (o as float64 numpy, rows of a sequence); the rows of no sequence must keep the sentinel written beforehand."""
    from arcquant_amd import kvcache
    args = _args(c, dtype)
    o = torch.full_like(args["q"], SENTINEL)
    assert kvcache.batch_prefill_f16(o, **args) is o
    got, n_rows = o.double().cpu().numpy(), int(c["qo"][-1])
    assert (got[n_rows:] == SENTINEL).all(), "rows at or beyond qo_indptr[B] were written"
    return got, n_rows


BOUND_RUNS = [(case, g, dtype) for case in ("tiny", "chunk", "chunk1", "tiles", "group") for g in (1, 4, 7) for dtype in (F16, BF16)]
BOUND_RUNS += [("deep", 1, F16), ("group", 130, F16)]               # the long loop; two chunks of heads per kv head


@pytest.mark.parametrize("case,g,dtype", BOUND_RUNS, ids=[f"{c}-g{g}-{str(d)[6:]}" for c, g, d in BOUND_RUNS])
def test_within_the_bound(case, g, dtype):
    c = _randn_case(case, dtype, g)
    got, n = _run(c, dtype)
    err, bound = np.abs(got[:n] - c["ref"][:n]), c["bound"][:n]
    print(f"{case} g={g} {dtype}: max err/bound = {(err / bound).max():.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got[:n]).all() and (err <= bound).all(), f"max err / bound = {(err / bound).max()}"


@functools.lru_cache(maxsize=None)
def _probe_case(case, g):
    """One-hot queries and K rows that put ~90 nats between one target position and every other permitted one, a decoy twice as high on the
    first masked position; V[t, d] = ((7 t + d) mod 256) - 128 is exact in both types, so the output IS the target's V row."""
    spec, lens, new, qo, _, tables = PR.case_geometry(case)
    N, start = spec["N"], np.concatenate([[0], np.cumsum(lens)])
    k, v = np.zeros((sum(lens), N, 128)), np.zeros((sum(lens), N, 128))
    q, want, rows = np.zeros((int(qo[-1]) + PR.PAD_ROWS, g * N, 128)), np.zeros((int(qo[-1]) + PR.PAD_ROWS, g * N, 128)), []
    for b, (T, n) in enumerate(zip(lens, new)):
        v[start[b]:start[b] + T] = (((7 * np.arange(T)[:, None] + np.arange(128)[None, :]) % 256) - 128)[:, None, :]
        for i in range(min(n, 128)):
            limit = T - n + i
            cands = sorted({t for t in (0, 31, 32, 63, 64, limit - 1, limit) if 0 <= t <= limit})
            target = cands[i % len(cands)]
            k[start[b] + target, :, i] = 16.0
            if limit + 1 < T:
                k[start[b] + limit + 1, :, i] = 32.0                                    # the decoy
            q[qo[b] + i, :, i] = 64.0
            want[qo[b] + i] = v[start[b] + target, 0]
            rows.append(qo[b] + i)
    data = _cache(case, k, v)
    assert np.abs(_attention_f64(q, qo, data, tables, N)[0][rows] - want[rows]).max() <= 1e-30, "the fp64 reference is the target's V row"
    return dict(q64=q, qo=qo, data=data, tables=tables, want=want[rows], rows=np.array(rows))


@pytest.mark.parametrize("case", ["chunk", "tiles"])
@pytest.mark.parametrize("g", [1, 4])
@DTYPES
def test_probes(case, g, dtype):
    c = _probe_case(case, g)
    got, _ = _run(dict(c, q=torch.from_numpy(c["q64"]).to(dtype)), dtype)
    err = np.abs(got[c["rows"]] - c["want"])
    print(f"{case} g={g} {dtype}: probes max |err| = {err.max():.3e}")
    assert (err <= 2 * U[dtype] * np.abs(c["want"]).max(-1, keepdims=True) + 1e-6).all(), f"row {c['rows'][err.max((1, 2)).argmax()]}: {err.max()}"


@DTYPES
def test_unwritten_rows_and_graph_replay(dtype):
    from arcquant_amd import kvcache
    c = _randn_case("chunk", dtype, 4)                  # sequences (40, 0) and (0, 0) have n_b = 0; PAD_ROWS rows follow qo_indptr[B]
    args, n_rows = _args(c, dtype), int(c["qo"][-1])
    eager = torch.full_like(args["q"], SENTINEL)
    kvcache.batch_prefill_f16(eager, **args)
    assert (eager[n_rows:] == SENTINEL).all() and torch.isfinite(eager[:n_rows]).all()
    o = torch.full_like(eager, SENTINEL)
    torch.cuda.synchronize()
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        kvcache.batch_prefill_f16(o, **args)
    torch.cuda.synchronize()
    for _ in range(3):
        o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), eager.view(torch.int16))
