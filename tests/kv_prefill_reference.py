"""The causal prefill attention of include/arcq_kv.h (arcq_kv_batch_prefill) in fp64 on the CPU, on top of tests/kv_reference.py: the
query tokens of sequence b are its last n_b positions, query i attends over positions 0 .. T_b - n_b + i.  It also holds the cases the
GPU tests of the prefill share (``PREFILL_CASES``) and builds their inputs once.  Test infrastructure: slow, plain and independent of
the library."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import kv_reference as R


def paged_prefill_f64(q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer):
    """q float64 [ntok, Nq, 128], qo_indptr int [B + 1] -> (out [ntok, Nq, 128], (spa [ntok, Nq, 128], qa [ntok, Nq])): the bound terms
    of ``kv_reference.paged_attention_f64`` (``sum_t p_t a_td`` per output element, ``sm_scale * max_t sum_d |q_d| a_td`` per row), each
    query row over the positions it may attend to only.  Rows of no sequence (at or beyond qo_indptr[B]) stay zero, bound terms
    included; a sequence with n_b = 0 or T_b = 0 contributes no rows."""
    ntok, Nq, _ = q.shape
    N = kv_data.shape[3]
    g = Nq // N
    P = kv_data.shape[4]
    lens = R.seq_lens(kv_indptr, last_page_offset, P)
    out, spa, qa = np.zeros((ntok, Nq, R.D)), np.zeros((ntok, Nq, R.D)), np.zeros((ntok, Nq))
    for b in range(len(lens)):
        q0, nb, T = int(qo_indptr[b]), int(qo_indptr[b + 1] - qo_indptr[b]), int(lens[b])
        if nb == 0 or T == 0:
            continue
        assert nb <= T, "the contract: the query tokens are positions of the sequence"
        for n in range(N):
            kr, kp = R.gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 0)
            vr, vp = R.gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 1)
            K, V = R.dequantize_f32(kr, kp).astype(np.float64), R.dequantize_f32(vr, vp).astype(np.float64)
            ck, cv = R.unpack_codes(kr).astype(np.float64), R.unpack_codes(vr).astype(np.float64)
            aK = ck * kp[:, 0:1].astype(np.float64) + np.abs(kp[:, 1:2].astype(np.float64))
            aV = cv * vp[:, 0:1].astype(np.float64) + np.abs(vp[:, 1:2].astype(np.float64))
            for i in range(nb):
                end = T - nb + i + 1                                  # positions 0 .. end - 1
                for h in range(n * g, (n + 1) * g):
                    sc = (K[:end] @ q[q0 + i, h]) * R.SM_SCALE
                    p = np.exp(sc - sc.max())
                    p /= p.sum()
                    out[q0 + i, h] = p @ V[:end]
                    spa[q0 + i, h] = p @ aV[:end]
                    qa[q0 + i, h] = R.SM_SCALE * (aK[:end] @ np.abs(q[q0 + i, h])).max()
    return out, (spa, qa)


def prefill_bound(ref, spa, qa, u, T_rows):
    """|got - ref| <= decode_bound(ref, spa, qa, u, n = T_b) + 2 u spa, element-wise; T_rows [ntok, 1, 1] = T_b of each row's sequence.
    n = T_b is the any-order worst case of the fp32 sums; the extra term is one rounding of each weight p s to the 16-bit type, on the
    numerator and on a row sum taken from either the rounded or the unrounded weights."""
    return R.decode_bound(ref, spa, qa, u, T_rows) + 2.0 * u * spa


# ---- the cases of the GPU tests, as (T, n) per sequence: n and T - n straddle multiples of 16 / 32 / 64 / 128
PREFILL_CASES = {
    "tiny": dict(P=16, N=1, seqs=((1, 1), (2, 2), (3, 1), (17, 16))),
    "chunk": dict(P=16, N=2, seqs=((100, 37), (64, 64), (65, 33), (40, 0), (0, 0)), empty_pages=0),
    "chunk1": dict(P=16, N=2, seqs=((100, 37), (64, 64), (65, 33), (40, 0), (0, 0)), empty_pages=1),
    "tiles": dict(P=5, N=1, seqs=((300, 130), (129, 129), (257, 1))),
    "deep": dict(P=16, N=1, seqs=((1000, 96), (1, 1))),
}
L, LAYER, SENTINEL, PAD_ROWS = 2, 1, 0xA5, 3


def case_geometry(case):
    spec = PREFILL_CASES[case]
    lens, new = [T for T, _ in spec["seqs"]], [n for _, n in spec["seqs"]]
    qo = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    pages, indptr, indices, last = R.make_tables(lens, spec["P"], seed=len(case) + spec["P"], empty_pages=spec.get("empty_pages", 0))
    return spec, lens, new, qo, pages, (indptr, indices, last)


@functools.lru_cache(maxsize=None)
def case_pages(case, dtype):
    """The pages of a case: randn * 3 rows of ``dtype`` through ``kv_reference.quantize_i4`` in layer 1, sentinel bytes elsewhere.  Built
    once and shared; nothing may modify it."""
    spec, lens, new, qo, pages, tables = case_geometry(case)
    P, N = spec["P"], spec["N"]
    gen = torch.Generator().manual_seed(P + sum(lens) + len(case))
    ntok_kv = sum(lens)
    sl = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k, v = (torch.randn(ntok_kv, N, 128, generator=gen) * 3).to(dtype), (torch.randn(ntok_kv, N, 128, generator=gen) * 3).to(dtype)
    (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
    data = np.full((pages, L, 2, N, P, 64), SENTINEL, dtype=np.uint8)
    param = np.zeros((pages, L, 2, N, P, 2), dtype=np.float16)
    param.view(np.uint8)[...] = SENTINEL
    R.write_rows(data, param, *tables, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), sl, LAYER)
    return dict(P=P, N=N, lens=lens, new=new, qo=qo, pages=pages, tables=tables, data=data, param=param, gen_state=gen.get_state())


@functools.lru_cache(maxsize=None)
def case_inputs(case, dtype, g):
    """case_pages + randn queries of ``dtype`` for g heads per kv head (PAD_ROWS rows beyond qo_indptr[B] that belong to no sequence) and
    the fp64 reference with its bound terms.  T_rows [ntok, 1, 1]: T_b of each row's sequence (0 for the rows of none)."""
    c = case_pages(case, dtype)
    gen = torch.Generator()
    gen.set_state(c["gen_state"])
    ntok = int(c["qo"][-1]) + PAD_ROWS
    q = torch.randn(ntok, g * c["N"], 128, generator=gen).to(dtype)
    ref, (spa, qa) = paged_prefill_f64(q.double().numpy(), c["qo"], c["data"], c["param"], *c["tables"], LAYER)
    T_rows = np.zeros((ntok, 1, 1))
    for b, T in enumerate(c["lens"]):
        T_rows[c["qo"][b]:c["qo"][b + 1]] = T
    return dict(c, q=q, ntok=ntok, ref=ref, spa=spa, qa=qa, T_rows=T_rows)


# ---- controlled scores: the spike profile of kv_reference, one target position per query row
def edge_queries(T, n):
    """Query indices i of a sequence whose own position T - n + i is a multiple of 16, 32, 64 or 128, or one below one, plus the first and
    the last query."""
    own = [T - n + i for i in range(n)]
    return [i for i, t in enumerate(own) if t % 16 == 0 or t % 16 == 15 or i in (0, n - 1)]


@functools.lru_cache(maxsize=None)
def spike_case(case, dtype, g, mode):
    """The pages of ``case`` written from ``profile_rows("spike", ...)``; every query row is q = 8 K_t = 2 c_t - 15 for a target t:
    mode "diagonal": its own position, the last one it may attend to, so the output is V there up to e^-30 of anything else;
    mode "masked": own + 1 (the sequence's last query: own), a row that exists and is masked, so the output is the fp64 reference's
    mix of the allowed rows and a leak returns V at own + 1.  -> case_inputs' dict + targets [ntok], own [ntok], gap (the smallest lead
    of a target's score over every OTHER position of its sequence, allowed or not; for "masked" that is what a leak would win by)."""
    spec, lens, new, qo, pages, tables = case_geometry(case)
    P, N = spec["P"], spec["N"]
    rows = R.profile_rows("spike", lens, N, seed=P + sum(lens) + len(mode))
    data, param = R.rows_to_cache(pages, L, P, tables, lens, LAYER, *rows, True, dtype, fill=SENTINEL)
    k_codes = rows[0]
    start = np.concatenate([[0], np.cumsum(lens)])
    ntok = int(qo[-1]) + PAD_ROWS
    q = np.zeros((ntok, g * N, 128))
    targets, own = np.full(ntok, -1), np.full(ntok, -1)
    gap = np.inf
    for b, (T, n) in enumerate(zip(lens, new)):
        for i in range(n):
            r = qo[b] + i
            own[r] = T - n + i
            targets[r] = own[r] if mode == "diagonal" or i == n - 1 else own[r] + 1
            for h in range(g * N):
                q[r, h] = 2.0 * k_codes[start[b] + targets[r], h // g].astype(np.float64) - 15.0
                K = 0.25 * k_codes[start[b]:start[b] + T, h // g].astype(np.float64) - 1.875
                sc = (K @ q[r, h]) * R.SM_SCALE
                gap = min(gap, sc[targets[r]] - np.delete(sc, targets[r]).max())
    ref, (spa, qa) = paged_prefill_f64(q, qo, data, param, *tables, LAYER)
    T_rows = np.zeros((ntok, 1, 1))
    for b, T in enumerate(lens):
        T_rows[qo[b]:qo[b + 1]] = T
    v_codes, v_param = rows[2], rows[3]
    V = v_codes.astype(np.float64) * v_param[..., 0:1].astype(np.float64) - v_param[..., 1:2].astype(np.float64)      # [sum lens, N, 128]
    return dict(P=P, N=N, lens=lens, new=new, qo=qo, pages=pages, tables=tables, data=data, param=param, q=torch.from_numpy(q).to(dtype),
                ntok=ntok, ref=ref, spa=spa, qa=qa, T_rows=T_rows, targets=targets, own=own, gap=float(gap), V=V, start=start)
