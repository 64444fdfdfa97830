"""The causal prefill attention of include/arcq_kv.h (arcq_kv_batch_prefill) in fp64 on the CPU, on top of tests/kv_reference.py: the
query tokens of sequence b are its last n_b positions, query i attends over positions 0 .. T_b - n_b + i.  It also holds the cases the
GPU tests of the prefill share (``PREFILL_CASES``) and builds their inputs once: randn rows (``case_inputs``), spikes at the diagonal
(``spike_case``), the uniform and ramp profiles (``profile_case``) and spikes at every block edge below the diagonal (``probe_case``).
``prefill_f32_emulated`` restates the algorithm in numpy fp32, with one deliberate mistake on request: what the CPU tests measure the
inputs' teeth with.  Test infrastructure: slow, plain and independent of the library."""
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
    "group": dict(P=16, N=2, seqs=((70, 40), (33, 33), (1, 1))),      # the wide groups: g = 8 .. 130 (tile_geometry)
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


# ---- the launcher's tiling, restated (kv_prefill.hip: kv_prefill, the first lines of kv_prefill_kernel).  Used ONLY to assert that a
#      case reaches the geometry it claims, never to compute an expected value.
TILE_ROWS, BLOCK = 128, 32
WIDE_GS = (8, 16, 32, 64, 128, 130)


# what the GPU tests run (tests/test_kvprefill_gpu.py) and the CPU tests hold the unmutated emulation to (tests/test_kv_prefill_reference.py)
UNIFORM_RUNS = [(case, g) for case in ("chunk", "tiles", "deep", "group") for g in (1, 7, 8, 32)]
RAMP_RUNS = [(case, profile, g) for case in ("tiles", "deep") for profile in ("ramp_up", "ramp_down") for g in (2, 7)]
PROBE_RUNS = [("tiles", 7), ("deep", 7)] + [("group", g) for g in WIDE_GS]


def tile_geometry(g):
    """-> (hc heads per chunk, tpt tokens per tile, chunks per kv head)."""
    hc = min(g, TILE_ROWS)
    return hc, TILE_ROWS // hc, (g + hc - 1) // hc


def wave_lasts(T, n, g):
    """[tiles of the sequence][4]: the last kv position each wave of a tile attends to, -1 for a wave none of whose 32 slots holds a
    token of the sequence (the kernel's ``wave_last``; a wave visits block tb iff tb <= wave_last)."""
    hc, tpt, _ = tile_geometry(g)
    out = []
    for tok0 in range(0, n, tpt):
        row = []
        for w in range(4):
            t0, t1 = (w * 32) // hc, min((w * 32 + 31) // hc, tpt - 1)
            row.append(T - n + min(tok0 + t1, n - 1) if t0 < tpt and tok0 + t0 < n else -1)
        out.append(row)
    return out


def _t_rows(ntok, qo, lens):
    T_rows = np.zeros((ntok, 1, 1))
    for b, T in enumerate(lens):
        T_rows[qo[b]:qo[b + 1]] = T
    return T_rows


# ---- profiles with controlled scores for the prefill: kv_reference.profile_rows written through rows_to_cache
def uniform_bound(ref, u):
    """|got - ref| <= (u + 2^-21) |ref| + 2^-25 for the uniform profile.  With q = 0 every allowed score is exactly 0 and every weight 1,
    the rounded weight p s is the V scale (1/8, 1/4 or 1/2), every product s c is a multiple of 1/8 below 8, every p z a multiple of 1/16
    below 4 and l a count: for T <= 1000 every partial sum is an integer below 2^24 in its unit, so the three sums are exact in fp32 in
    ANY order.  What is left: the reciprocal and the product in fp32 (2^-21 |ref| has a factor 4 of room for a reciprocal that is 1 ulp
    accurate), the rounding of the result (u |ref|) and, below 2^-14, fp16's subnormal grid (2^-25).  No spa term, no n term."""
    return (u + 2.0 ** -21) * np.abs(ref) + 2.0 ** -25


def uniform_premises(c):
    """What makes the three sums of the uniform profile exact in fp32 in any order, asserted on the operands themselves: q = 0, V scales
    in {1/8, 1/4, 1/2} with zero = 7.5 scale, and per sequence and kv head  sum_t s c  below 2^24 units of 1/8,  sum_t z  below 2^24
    units of 1/16, T below 2^24.  -> the largest of the three sums in its unit."""
    assert not c["q"].double().any()
    worst = 0.0
    for b, T in enumerate(c["lens"]):
        for n in range(c["N"] if T else 0):
            vr, vp = R.gather_rows(c["data"], c["param"], *c["tables"], LAYER, b, n, 1)          # the pages themselves
            s, z = vp[:, 0].astype(np.float64), vp[:, 1].astype(np.float64)
            assert len(s) == T and set(np.unique(s)) <= {0.125, 0.25, 0.5} and np.array_equal(z, 7.5 * s)
            sc = (s[:, None] * R.unpack_codes(vr).astype(np.float64)).sum(0) * 8.0
            worst = max(worst, float(sc.max()), float(z.sum()) * 16.0, float(T))
    assert worst < 2.0 ** 24
    return worst


@functools.lru_cache(maxsize=None)
def _profile_core(case, profile, g):
    spec, lens, new, qo, pages, tables = case_geometry(case)
    P, N = spec["P"], spec["N"]
    rows = R.profile_rows(profile, lens, N, seed=P + sum(lens) + len(profile))
    data, param = R.rows_to_cache(pages, L, P, tables, lens, LAYER, *rows, True, torch.float16, fill=SENTINEL)
    ntok = int(qo[-1]) + PAD_ROWS
    q = np.zeros((ntok, g * N, 128))
    if profile != "uniform":
        q[:int(qo[-1])] = R.profile_q(profile, (1,), N, g, rows[0])[0]          # beta[h % 2] w, the same for every query token
        ref, (spa, qa) = paged_prefill_f64(q, qo, data, param, *tables, LAYER)
    elif g == 1:
        ref, (spa, qa) = paged_prefill_f64(q, qo, data, param, *tables, LAYER)
    else:        # q = 0: the heads of a group agree, so the reference is computed once per (token, kv head) and repeated
        one = _profile_core(case, profile, 1)
        ref, spa, qa = (np.repeat(one[k], g, axis=1) for k in ("ref", "spa", "qa"))
    return dict(P=P, N=N, lens=lens, new=new, qo=qo, pages=pages, tables=tables, data=data, param=param, q64=q, ntok=ntok, ref=ref,
                spa=spa, qa=qa, T_rows=_t_rows(ntok, qo, lens))


def profile_case(case, profile, dtype, g):
    """The pages of ``case`` written from ``kv_reference.profile_rows(profile, ...)``; uniform: q = 0 for every row; ramp_up / ramp_down:
    q = RAMP_BETA[h % 2] w (``kv_reference.profile_q``) for every query token, so that a query's running maximum rises in every block up
    to its own position (up) or settles in block 0 while the later weights fall below fp16's normal range (down).  -> case_inputs' dict
    (q exact in ``dtype``).  Shared; nothing may modify it."""
    c = _profile_core(case, profile, g)
    q = torch.from_numpy(c["q64"]).to(dtype)
    assert torch.equal(q.double(), torch.from_numpy(c["q64"]))
    return dict(c, q=q)


@functools.lru_cache(maxsize=None)
def _probe_core(case, g):
    spec, lens, new, qo, pages, tables = case_geometry(case)
    P, N = spec["P"], spec["N"]
    gN = g * N
    rows = R.profile_rows("spike", lens, N, seed=P + sum(lens) + 5)
    data, param = R.rows_to_cache(pages, L, P, tables, lens, LAYER, *rows, True, torch.float16, fill=SENTINEL)
    k_codes, v_codes, v_param = rows[0], rows[2], rows[3]
    start = np.concatenate([[0], np.cumsum(lens)])
    ntok = int(qo[-1]) + PAD_ROWS
    q = np.zeros((ntok, gN, 128))
    targets, own = np.full((ntok, gN), -1), np.full(ntok, -1)
    heads_kv = np.arange(gN) // g
    gap = np.inf
    for b, (T, n) in enumerate(zip(lens, new)):
        K = (0.25 * k_codes[start[b]:start[b] + T].astype(np.float64) - 1.875)[:, heads_kv]           # [T, gN, 128]
        for i in range(n):
            r = qo[b] + i
            own[r] = T - n + i
            pos = [t for t in R.probe_positions(own[r] + 1, BLOCK) if t >= 0]           # (own = 0: own - 1 does not exist)
            targets[r] = [pos[(i * gN + h) % len(pos)] for h in range(gN)]
            q[r] = 2.0 * k_codes[start[b] + targets[r], heads_kv].astype(np.float64) - 15.0
            sc = np.einsum("thd,hd->th", K, q[r]) * R.SM_SCALE                          # over ALL positions of the sequence
            for h in range(gN):
                t = targets[r, h]
                if T > 1:
                    gap = min(gap, sc[t, h] - np.delete(sc[:, h], t).max())
    ref, (spa, qa) = paged_prefill_f64(q, qo, data, param, *tables, LAYER)
    V = v_codes.astype(np.float64) * v_param[..., 0:1].astype(np.float64) - v_param[..., 1:2].astype(np.float64)      # [sum lens, N, 128]
    want = np.zeros((ntok, gN, 128))
    for b in range(len(lens)):
        for r in range(qo[b], qo[b + 1]):
            want[r] = V[start[b] + targets[r], heads_kv]
    return dict(P=P, N=N, lens=lens, new=new, qo=qo, pages=pages, tables=tables, data=data, param=param, q64=q, ntok=ntok, ref=ref, spa=spa,
                qa=qa, T_rows=_t_rows(ntok, qo, lens), targets=targets, own=own, gap=float(gap), want=want, V=V, start=start)


def probe_case(case, dtype, g):
    """Interior probes: the pages of ``case`` from the spike profile; head h of query row i of a sequence (own position ``own``) is a
    spike, q = 8 K_t = 2 c_t - 15, at t = pos[(i gN + h) % len(pos)] with pos = kv_reference.probe_positions(own + 1, 32): every multiple
    of the block at or below own, the position before each, 0, own - 1 and own.  Neighbouring heads always point at different rows and
    neighbouring tokens mostly, so a head stored to the wrong row of o shows, and so does a block edge below the diagonal that is skipped
    or misaddressed.  -> case_inputs' dict + targets [ntok, gN], own [ntok], gap (the smallest lead of a target's score over every OTHER
    position of its sequence, masked ones included), want [ntok, gN, 128] (the targets' V rows, fp64).  Shared; nothing may modify it."""
    c = _probe_core(case, g)
    return dict(c, q=torch.from_numpy(c["q64"]).to(dtype))


def probe_rows_ok(got, c, dtype, u):
    """bool [rows of a sequence, gN]: |got - V_target| <= 2 u max|V_target| + 1e-6 over the 128 elements (the diagonal spikes' assertion),
    V_target rounded to ``dtype``."""
    n_rows = int(c["qo"][-1])
    want = torch.from_numpy(c["want"][:n_rows]).to(dtype).double().numpy()
    return np.abs(got[:n_rows] - want).max(-1) <= 2 * u * np.abs(want).max(-1) + 1e-6


# ---- what any fp32 implementation of the header's algorithm owes the bounds, and the same with one deliberate mistake
IDLE = np.float32(-3.0e38)
MUTATIONS = ("drop", "double", "mask_late", "mask_early", "unswapped", "neighbour", "head_xor_1")


def _swap23(t):
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def prefill_f32_emulated(q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, dtype, mutate=None):
    """The prefill in plain numpy fp32, written from include/arcq_kv.h's formula and DESIGN 11 "Prefill", not from the library: blocks of
    32 positions, an online base-2 softmax (score = sm_scale log2(e) (s_t c_t . q - z_t sum_d q_d)), the weight p_t s_t rounded once to
    ``dtype``, fp32 sums of (p s) c, p z and p, one division, the result rounded to ``dtype``.  q float64 [ntok, Nq, 128] (values of
    ``dtype``) -> float64 [ntok, Nq, 128], zeros in rows of no sequence.

    mutate = (name, t) is one mistake an implementation could make (t: a position, where the mistake has one):
      drop        position t is left out                          double      position t is summed twice
      mask_late   own + 1 is allowed (where it exists)            mask_early  own is excluded
      unswapped   the V CODES of a block are taken in the order that has bits 2 and 3 of the position swapped while scale, zero and
                  weight keep theirs (rows past T - 1 clamp to T - 1, as a load would)
      neighbour   the V row of position t is read from t ^ 1 (where that exists), whatever t
      head_xor_1  head h's result is stored to head h ^ 1 (where that exists)"""
    name, at = mutate if mutate else (None, None)
    assert name is None or name in MUTATIONS
    f32 = np.float32
    ntok, Nq, _ = q.shape
    N, P = kv_data.shape[3], kv_data.shape[4]
    g = Nq // N
    lens = R.seq_lens(kv_indptr, last_page_offset, P)
    sm = f32(R.SM_SCALE * np.log2(np.e))
    out = np.zeros((ntok, Nq, R.D))

    def rnd(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).float().numpy()

    for b in range(len(lens)):
        q0, nb, T = int(qo_indptr[b]), int(qo_indptr[b + 1] - qo_indptr[b]), int(lens[b])
        if nb == 0 or T == 0:
            continue
        for n in range(N):
            kr, kp = R.gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 0)
            vr, vp = R.gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 1)
            ck, cv = R.unpack_codes(kr).astype(f32), R.unpack_codes(vr).astype(f32)
            ks, kz = kp[:, 0].astype(f32) * sm, kp[:, 1].astype(f32) * sm
            vs, vz = vp[:, 0].astype(f32), vp[:, 1].astype(f32)
            if name == "neighbour":
                src = np.minimum(np.arange(T) ^ 1, T - 1)
                cv, vs, vz = cv[src], vs[src], vz[src]
            Q = q[q0:q0 + nb, n * g:(n + 1) * g].astype(f32).reshape(nb * g, R.D)          # row = (token, head of the group)
            own = np.repeat(T - nb + np.arange(nb), g)
            limit = own + 1 if name == "mask_late" else own - 1 if name == "mask_early" else own
            nqsum = -Q.sum(-1, dtype=f32)
            rows = nb * g
            m, l, zacc, acc = np.full(rows, IDLE), np.zeros(rows, f32), np.zeros(rows, f32), np.zeros((rows, R.D), f32)
            for tb in range(0, int(min(limit.max(), T - 1)) + 1, BLOCK):
                pos = np.arange(tb, min(tb + BLOCK, T))
                ok = pos[None, :] <= limit[:, None]
                if name == "drop":
                    ok &= pos[None, :] != at
                sc = ks[pos] * (Q @ ck[pos].T) + kz[pos] * nqsum[:, None]
                sc = np.where(ok, sc, IDLE).astype(f32)
                mn = np.maximum(m, sc.max(-1))
                alpha = np.exp2(m - mn, dtype=f32)
                m = mn
                p = np.where(ok, np.exp2(sc - m[:, None], dtype=f32), f32(0))
                if name == "double":
                    p = p * np.where(pos == at, f32(2), f32(1))
                codes = cv[np.minimum(tb + _swap23(np.arange(len(pos))), T - 1)] if name == "unswapped" else cv[pos]
                l = l * alpha + p.sum(-1, dtype=f32)
                zacc = zacc * alpha + (p * vz[pos]).sum(-1, dtype=f32)
                acc = acc * alpha[:, None] + rnd(p * vs[pos]) @ codes
            with np.errstate(divide="ignore", invalid="ignore"):
                y = np.where(l[:, None] > 0, (acc - zacc[:, None]) / l[:, None], f32(0))
            out[q0:q0 + nb, n * g:(n + 1) * g] = rnd(y).astype(np.float64).reshape(nb, g, R.D)
    if name == "head_xor_1":
        moved = out.copy()
        for h in range(Nq):
            if h ^ 1 < Nq:
                moved[:, h ^ 1] = out[:, h]
        out = moved
    return out
