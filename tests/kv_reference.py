"""The paged KV-cache format of include/arcq_kv.h restated with numpy / torch on the CPU: offset arithmetic, the quantiser and its
inverse, the writers and an fp64 paged attention that walks the tables.  Test infrastructure: slow, plain and independent of the library.

    kv_data   uint8 [pages, L, 2, N, P, 64] (int4) | 16-bit [pages, L, 2, N, P, 128];  kv_param float16 [pages, L, 2, N, P, 2]
    byte j of an int4 row = element 2j (low nibble) | element 2j+1 (high nibble);  value = float(code) * float(scale) - float(zero)
    sequence b: pages kv_indices[kv_indptr[b] .. kv_indptr[b+1]), (count - 1) * P + last_page_offset[b] positions; a result <= 0 is a
    sequence without positions (no pages or one page, last_page_offset[b] = 0 -- the two spellings the header names)

Below the format: the launcher's partition restated (``decode_splits``, ``wave_ranges`` -- used to ASSERT that a test case reaches the
path it claims, never to compute an expected value), the ragged decode cases shared by the GPU tests (``CASES``) and input profiles that
write the cache from codes and (scale, zero) pairs so that the scores are controlled (``profile_rows``).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

D = 128
SM_SCALE = 1.0 / np.sqrt(128.0)


# ---- offsets (include/flashinfer/page.cuh:76-103), in ELEMENTS of a row-major [pages, L, 2, N, P, row]
def k_elem_offset(page, head, entry, feat, L, layer, N, P, row):
    return (((page * L + layer) * 2 * N + head) * P + entry) * row + feat


def v_elem_offset(page, head, entry, feat, L, layer, N, P, row):
    return ((((page * L + layer) * 2 + 1) * N + head) * P + entry) * row + feat


def seq_lens(kv_indptr, last_page_offset, P):
    ip, lp = np.asarray(kv_indptr, dtype=np.int64), np.asarray(last_page_offset, dtype=np.int64)
    return np.maximum((ip[1:] - ip[:-1] - 1) * P + lp, 0)      # (no pages and last_page_offset 0: the formula says -P, the sequence is empty)


def locate(kv_indptr, kv_indices, b, pos, P):
    """(page, entry) of position ``pos`` of sequence ``b``."""
    return int(kv_indices[int(kv_indptr[b]) + pos // P]), pos % P


# ---- the quantiser: what torch eager computes on a CPU tensor of the input dtype (model/kv_cache.py:22-33)
def quantize_i4(x: torch.Tensor):
    """x [..., 128] float16 / bfloat16 on the CPU -> (packed uint8 [..., 64], param float16 [..., 2] = (scale, zero))."""
    assert x.device.type == "cpu" and x.dtype in (torch.float16, torch.bfloat16)
    maxq = torch.tensor(15)
    xmax = torch.amax(x, dim=-1, keepdim=True)
    xmin = torch.amin(x, dim=-1, keepdim=True)
    scale = (xmax - xmin).clamp(min=1e-5) / maxq
    zero = -xmin
    q = torch.clamp(torch.round((x + zero) / scale), 0, maxq)
    q = torch.nan_to_num(q, nan=0.0).to(torch.uint8)          # (inf / inf of an overflowing fp16 range: the cast of NaN is code 0)
    packed = q[..., 0::2] | (q[..., 1::2] << 4)
    return packed, torch.cat([scale, zero], dim=-1).to(torch.float16)


def quantize_i4_stepwise(x: torch.Tensor):
    """The same rule spelled out in fp32 with an explicit rounding to the input dtype after every operation (what the kernel does)."""
    T = x.dtype

    def rnd(f):
        return f.to(T).float()
    xf = x.float()
    xmax, xmin = xf.amax(-1, keepdim=True), xf.amin(-1, keepdim=True)
    rng = torch.maximum(rnd(xmax - xmin), rnd(torch.tensor(1e-5)))
    scale, zero = rnd(rng / 15.0), -xmin
    q = torch.round(rnd(rnd(xf + zero) / scale))
    q = torch.nan_to_num(q, nan=0.0).clamp(0, 15).to(torch.uint8)
    return q[..., 0::2] | (q[..., 1::2] << 4), torch.cat([scale, zero], dim=-1).to(T).to(torch.float16)


def unpack_codes(packed: np.ndarray) -> np.ndarray:
    """uint8 [..., 64] -> codes uint8 [..., 128]."""
    packed = np.asarray(packed)
    out = np.empty(packed.shape[:-1] + (packed.shape[-1] * 2,), dtype=np.uint8)
    out[..., 0::2] = packed & 0x0F
    out[..., 1::2] = packed >> 4
    return out


def pack_codes(codes: np.ndarray) -> np.ndarray:
    codes = np.asarray(codes, dtype=np.uint8)
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def dequantize_f32(packed: np.ndarray, param: np.ndarray) -> np.ndarray:
    """float(code) * float(scale) - float(zero) in fp32 (quantization.cuh:76): packed [..., 64], param float16 [..., 2]."""
    c = unpack_codes(packed).astype(np.float32)
    s, z = param[..., 0:1].astype(np.float32), param[..., 1:2].astype(np.float32)
    return (c * s).astype(np.float32) - z


# ---- the writers on numpy copies of the cache
def write_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer):
    """init (seqlen_indptr given: the tokens of sequence b become its LAST positions) or append (None: one token per sequence at
    seq_len - 1) on numpy arrays, in place.  Returns the (page, entry) pairs written."""
    P = kv_data.shape[4]
    lens = seq_lens(kv_indptr, last_page_offset, P)
    B = len(lens)
    if seqlen_indptr is None:
        seqlen_indptr = np.arange(B + 1)
    written = []
    for b in range(B):
        n_new = int(seqlen_indptr[b + 1] - seqlen_indptr[b])
        for j in range(n_new):
            tok, pos = int(seqlen_indptr[b]) + j, int(lens[b]) - n_new + j
            if pos < 0:                                       # (append to a sequence without positions: nothing is written)
                continue
            page, e = locate(kv_indptr, kv_indices, b, pos, P)
            kv_data[page, layer, 0, :, e] = k[tok]
            kv_data[page, layer, 1, :, e] = v[tok]
            kv_param[page, layer, 0, :, e] = k_param[tok]
            kv_param[page, layer, 1, :, e] = v_param[tok]
            written.append((page, e))
    return written


def gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, head, which):
    """The valid rows of one sequence and head, in position order -> (rows [T, row], params float16 [T, 2]); T = 0 gives empty arrays."""
    P = kv_data.shape[4]
    T = int(seq_lens(kv_indptr, last_page_offset, P)[b])
    if T == 0:
        return np.zeros((0,) + kv_data.shape[5:], dtype=kv_data.dtype), np.zeros((0, 2), dtype=kv_param.dtype)
    rows, params = [], []
    for pos in range(T):
        page, e = locate(kv_indptr, kv_indices, b, pos, P)
        rows.append(kv_data[page, layer, which, head, e])
        params.append(kv_param[page, layer, which, head, e])
    return np.stack(rows), np.stack(params)


def paged_attention_f64(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, i4=True):
    """fp64 attention over the pages: q float64 [B, Nq, 128] -> (out [B, Nq, 128], bound_terms) where bound_terms holds, per output
    element, ``sum_t p_t a_td`` and, per (b, h), ``sm_scale * max_t sum_d |q_d| a_td`` with a_td = c_td * s_t + |z_t| (the magnitudes the
    kernel's fp32 error scales with; for a 16-bit cache a_td = |v_td| / |k_td|).  kv_data / kv_param are numpy arrays; a 16-bit cache is
    passed as float64 values.

    A sequence without positions gives rows of zeros and bound terms of zero, so the bound demands exact zeros.  include/arcq_kv.h names
    two spellings of it and promises zeros for both: no pages (kv_indptr[b+1] == kv_indptr[b]) with last_page_offset[b] = 0, and one page
    with last_page_offset[b] = 0."""
    B, Nq, _ = q.shape
    N = kv_data.shape[3]
    g = Nq // N
    out, spa, qa = np.zeros((B, Nq, D)), np.zeros((B, Nq, D)), np.zeros((B, Nq))
    for b in range(B):
        for n in range(N):
            kr, kp = gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 0)
            if len(kr) == 0:
                continue
            vr, vp = gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 1)
            if i4:
                K, V = dequantize_f32(kr, kp).astype(np.float64), dequantize_f32(vr, vp).astype(np.float64)
                ck, cv = unpack_codes(kr).astype(np.float64), unpack_codes(vr).astype(np.float64)
                aK = ck * kp[:, 0:1].astype(np.float64) + np.abs(kp[:, 1:2].astype(np.float64))
                aV = cv * vp[:, 0:1].astype(np.float64) + np.abs(vp[:, 1:2].astype(np.float64))
            else:
                K, V = kr.astype(np.float64), vr.astype(np.float64)
                aK, aV = np.abs(K), np.abs(V)
            for h in range(n * g, (n + 1) * g):
                sc = (K @ q[b, h]) * SM_SCALE
                p = np.exp(sc - sc.max())
                p /= p.sum()
                out[b, h] = p @ V
                spa[b, h] = p @ aV
                qa[b, h] = SM_SCALE * (aK @ np.abs(q[b, h])).max()
    return out, (spa, qa)


def decode_bound(ref, spa, qa, u, n=0):
    """|got - ref| <= u |ref| + (2 Delta + 2^-20 + n 2^-24) sum_t p_t a_td,  Delta = 130 * 2^-24 * sm_scale * max_t sum_d |q_d| a_td.

    n (default 0: the bound as it always was) is the longest chain of fp32 additions one accumulator of the value sum sees, see
    ``accumulation_chain``.  The 2^-20 stands for the sixteen roundings a single term p_t s_t c_td - p_t z_t and the final division meet;
    it has no room for the LENGTH of the sum.  With scores that differ (randn) a handful of positions carry the weight and the term is
    moot; with q = 0 every position weighs 1 / T, the score term Delta vanishes, and the accumulation is all that is left: a sum of n
    terms added one after the other is off by at most (n - 1) 2^-24 sum |terms| to first order, whatever the order."""
    delta = 130.0 * 2.0 ** -24 * qa
    return u * np.abs(ref) + (2.0 * delta[..., None] + 2.0 ** -20 + n * 2.0 ** -24) * spa


# ---- table construction for the tests
def make_tables(lens, P, seed=0, spare=2, empty_pages=0, pad=0):
    """A shuffled, non-contiguous page assignment for sequences of ``lens`` positions, with unused pages in between ->
    (pages, kv_indptr int32 [B+1], kv_indices int32 [nnz], last_page_offset int32 [B]).  A sequence of 0 positions gets ``empty_pages``
    (0 or 1) pages and last_page_offset 0.  ``pad`` appends that many entries to kv_indices that no sequence owns (an over-provisioned
    table: kv_indptr[B] < nnz); they name unused pages."""
    cnt = [(n + P - 1) // P if n else empty_pages for n in lens]
    nnz = sum(cnt)
    pages = (nnz + pad) * spare + 1
    rng = np.random.default_rng(seed)
    indices = rng.permutation(pages)[:nnz + pad].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    last = np.array([n - (c - 1) * P if n else 0 for n, c in zip(lens, cnt)], dtype=np.int32)
    assert (seq_lens(indptr, last, P) == np.asarray(lens)).all()
    return pages, indptr, indices, last


def valid_row_mask(shape, kv_indptr, kv_indices, last_page_offset, layer):
    """bool [pages, L, 2, N, P]: the rows decode may read -- valid positions of the referenced pages, in this layer."""
    pages, L, _, N, P = shape[:5]
    m = np.zeros((pages, L, 2, N, P), dtype=bool)
    for b, T in enumerate(seq_lens(kv_indptr, last_page_offset, P)):
        for pos in range(int(T)):
            page, e = locate(kv_indptr, kv_indices, b, pos, P)
            m[page, layer, :, :, e] = True
    return m


# ---- the launcher's partition, restated (kv_cache.hip: kv_group_chunk, kv_decode_splits, the first lines of kv_decode_kernel)
WAVES = 4


def decode_chunks(g):
    gc = 1 if g == 1 else 2 if g == 2 else 4
    return (g + gc - 1) // gc


def decode_splits(B, Nq, N, nnz, P):
    """Slices per sequence S.  nnz = entries of kv_indices, owned by a sequence or not."""
    work = B * N * decode_chunks(Nq // N)
    return max(1, min((1024 + work - 1) // work, (nnz * P // B) // (32 * WAVES), 32))


def wave_ranges(T, S, block):
    """int [S, 4, 2]: the positions [t0, t1) wave w of slice s streams, ``block`` = 32 (int4) | 16 (16-bit) positions per load block.
    t0 == t1: the wave is idle.  Only for asserting that a case reaches the path it claims."""
    nblk, units = (T + block - 1) // block, S * WAVES
    per = (nblk + units - 1) // units
    out = np.zeros((S, WAVES, 2), dtype=np.int64)
    for s in range(S):
        for w in range(WAVES):
            t0 = min(T, (s * WAVES + w) * per * block)
            out[s, w] = t0, min(T, t0 + per * block)
    return out


def blocks_per_wave(T, S, block):
    r = wave_ranges(T, S, block)
    return int(((r[..., 1] - r[..., 0] + block - 1) // block).max())


def accumulation_chain(T, S, block):
    """n of ``decode_bound`` from the kernel's structure: a lane adds one row per load to its accumulator, four loads per block and
    ``blocks_per_wave`` blocks (one rounding each, an FMA); log2(block / 4) shuffle additions join the rows of a load; one subtraction
    takes the zero sum off; the four waves merge (a product and an addition each) and then the S slices (the same).  At most T, and for the
    cases here a few dozen."""
    return 4 * blocks_per_wave(T, S, block) + int(np.log2(block // 4)) + 1 + 2 * WAVES + 2 * S


# ---- the ragged decode cases (tests/test_kvcache_gpu.py, test_kvstep_gpu.py; lengths include the step's new token)
#   S: slices per sequence, the same at every g in G_ALL;  per: 32-position blocks the busiest wave of the longest sequence streams (int4)
G_ALL = (1, 2, 3, 4, 7, 8, 9)
CASES = {
    "ragged": dict(P=16, lens=(1000, 1, 33, 2), N=1, S=2, per=4),       # two full loop trips, idle slices, T = 1 and T = 2 under S > 1
    "odd": dict(P=16, lens=(700, 1, 67), N=1, S=2, per=3),              # the loop ends on the reloaded buffer
    "five": dict(P=16, lens=(1100, 1, 1, 1), N=2, S=2, per=5),          # N > 1 with deep loops
    "single": dict(P=16, lens=(600, 1, 1, 1), N=1, S=1, per=5),         # deep loop with the direct store, no workspace
    "ragged5": dict(P=5, lens=(1000, 1, 33, 6), N=2, S=2, per=4),       # blocks spanning 6-7 pages
    "padded": dict(P=16, lens=(300, 40), N=1, S=10, per=1, pad=150),    # an over-provisioned table: most slices idle
    "empty": dict(P=16, lens=(1000, 0, 33, 0), N=1, S=2, per=4, empty_pages=0),     # no pages, last_page_offset 0
    "empty1": dict(P=16, lens=(1000, 0, 33, 0), N=1, S=2, per=4, empty_pages=1),    # one page, last_page_offset 0
}


def case_tables(spec, seed):
    return make_tables(spec["lens"], spec["P"], seed, empty_pages=spec.get("empty_pages", 0), pad=spec.get("pad", 0))


# ---- input profiles: the cache written from codes and (scale, zero) pairs, so that the scores are what the test wants
RAMP_BETA = (4.0, 3.0)                     # q = beta * w, alternating over the query heads
_rw = np.random.default_rng(128).permutation(128)
RAMP_PLUS, RAMP_MINUS = np.sort(_rw[:64]), np.sort(_rw[64:])          # w = +1 on PLUS, -1 on MINUS


def profile_rows(profile, lens, N, seed):
    """Rows of ``sum(lens)`` tokens in sequence order -> (k_codes uint8 [ntok, N, 128], k_param float16 [ntok, N, 2], v_codes, v_param).
    Every value code * scale - zero is a multiple of 2^-4 below 8, except the ramps' K rows: exact in float16 and in bfloat16.

      uniform, spike   K and V: random codes, scale in {1/8, 1/4, 1/2} (K of spike: 1/4), zero = 7.5 scale: values symmetric around 0.
                       uniform pairs them with q = 0 (every score exactly 0, o = the mean of the V rows); spike(t) with q = 8 K_t = 2 c_t - 15:
                       score_t = sm_scale 8 |K_t|^2 ~ 120, the others' ~ N(0, 8): o = V_t up to e^-30.
      ramp_up / _down  K row at position t: scale t 2^-9 (down: (T - 1 - t) 2^-9), code r + 7 on the 64 dimensions where w = +1 and r on
                       their partners where w = -1 (r random in 0..8), zero in {0, 1/2, 1, 2}.  With q = beta w the zero cancels and
                       score_t = sm_scale beta 448 t 2^-9 = 0.31 t (beta = 4) | 0.23 t (beta = 3): 7 - 10 units per 32 positions."""
    rng = np.random.default_rng(seed)
    ntok = int(sum(lens))
    scales = np.array([0.125, 0.25, 0.5])

    def sym(fixed=None):
        codes = rng.integers(0, 16, (ntok, N, 128), dtype=np.uint8)
        s = np.full((ntok, N, 1), fixed) if fixed else rng.choice(scales, (ntok, N, 1))
        return codes, np.concatenate([s, 7.5 * s], -1).astype(np.float16)
    v_codes, v_param = sym()
    if profile in ("uniform", "spike"):
        k_codes, k_param = sym(0.25 if profile == "spike" else None)
    elif profile in ("ramp_up", "ramp_down"):
        r = rng.integers(0, 9, (ntok, N, 64), dtype=np.uint8)
        k_codes = np.zeros((ntok, N, 128), dtype=np.uint8)
        k_codes[..., RAMP_PLUS], k_codes[..., RAMP_MINUS] = r + 7, r
        pos = np.concatenate([np.arange(T) if profile == "ramp_up" else np.arange(T)[::-1] for T in lens]).astype(np.float64)
        s = np.broadcast_to((pos * 2.0 ** -9)[:, None, None], (ntok, N, 1))
        k_param = np.concatenate([s, rng.choice(np.array([0.0, 0.5, 1.0, 2.0]), (ntok, N, 1))], -1).astype(np.float16)
    else:
        raise ValueError(profile)
    return k_codes, k_param, v_codes, v_param


def profile_q(profile, lens, N, g, k_codes, targets=None):
    """float64 [B, g N, 128], exact in float16 and bfloat16.  spike: targets int [B, g N], the position each (sequence, head) points at."""
    B = len(lens)
    q = np.zeros((B, g * N, 128))
    if profile in ("ramp_up", "ramp_down"):
        w = np.zeros(128)
        w[RAMP_PLUS], w[RAMP_MINUS] = 1.0, -1.0
        for h in range(g * N):
            q[:, h] = RAMP_BETA[h % 2] * w
    elif profile == "spike":
        start = np.concatenate([[0], np.cumsum(lens)])
        for b in range(B):
            for h in range(g * N):
                q[b, h] = 2.0 * k_codes[start[b] + int(targets[b, h]), h // g].astype(np.float64) - 15.0
    return q


def rows_to_cache(pages, L, P, tables, lens, layer, k_codes, k_param, v_codes, v_param, i4, dtype, fill=0xA5):
    """(kv_data, kv_param) holding the rows in ``layer`` and ``fill`` bytes (16-bit: NaN) elsewhere.  int4: packed codes + the pairs;
    16-bit: float64 values code * scale - zero rounded to ``dtype`` (a torch dtype), parameters of one."""
    import torch
    N = k_codes.shape[1]
    sl = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    param = np.zeros((pages, L, 2, N, P, 2), dtype=np.float16)
    param.view(np.uint8)[...] = fill
    if i4:
        data = np.full((pages, L, 2, N, P, 64), fill, dtype=np.uint8)
        write_rows(data, param, *tables, pack_codes(k_codes), pack_codes(v_codes), k_param, v_param, sl, layer)
        return data, param

    def values(codes, prm):
        x = codes.astype(np.float64) * prm[..., 0:1].astype(np.float64) - prm[..., 1:2].astype(np.float64)
        return torch.from_numpy(x).to(dtype).double().numpy()
    data = np.full((pages, L, 2, N, P, 128), np.nan)
    ones = np.ones(k_param.shape, dtype=np.float16)
    write_rows(data, param, *tables, values(k_codes, k_param), values(v_codes, v_param), ones, ones, sl, layer)
    return data, param


def paged_attention_f32(q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, i4=True):
    """The same attention in plain fp32 numpy (dequantise, scores, exp, weighted sum, one division): what any fp32 implementation owes
    the bound, before rounding to the output dtype."""
    B, Nq, _ = q.shape
    N = kv_data.shape[3]
    g = Nq // N
    out = np.zeros((B, Nq, D), dtype=np.float32)
    q32 = q.astype(np.float32) * np.float32(SM_SCALE)
    for b in range(B):
        for n in range(N):
            kr, kp = gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 0)
            if len(kr) == 0:
                continue
            vr, vp = gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 1)
            K, V = (dequantize_f32(kr, kp), dequantize_f32(vr, vp)) if i4 else (kr.astype(np.float32), vr.astype(np.float32))
            for h in range(n * g, (n + 1) * g):
                sc = K @ q32[b, h]
                p = np.exp(sc - sc.max(), dtype=np.float32)
                out[b, h] = (p @ V) / p.sum(dtype=np.float32)
    return out


@functools.lru_cache(maxsize=None)
def profile_case(case, profile, i4, dtype, g):
    """One of CASES under an input profile, on the CPU -> dict(data, param, tables, pages, q float64, ref, spa, qa, n) with n
    [B, 1, 1] = accumulation_chain of each sequence.  Built once and shared; nothing may modify it."""
    spec = CASES[case]
    P, lens, N = spec["P"], spec["lens"], spec["N"]
    pages, indptr, indices, last = case_tables(spec, seed=len(case) + P)
    rows = profile_rows(profile, lens, N, seed=P + sum(lens) + len(profile))
    data, param = rows_to_cache(pages, 2, P, (indptr, indices, last), lens, 1, *rows, i4, dtype)
    q = profile_q(profile, lens, N, g, rows[0])
    ref, (spa, qa) = paged_attention_f64(q, data, param, indptr, indices, last, 1, i4=i4)
    n = np.array([accumulation_chain(T, spec["S"], 32 if i4 else 16) for T in lens], dtype=np.float64).reshape(-1, 1, 1)
    return dict(P=P, lens=lens, N=N, S=spec["S"], layer=1, pages=pages, data=data, param=param, tables=(indptr, indices, last), q=q,
                ref=ref, spa=spa, qa=qa, n=n)


# ---- the range-edge probes: B x g (sequence, head) pairs over ONE set of pages, each a spike at another position
PROBE_B, PROBE_G, PROBE_P = 10, 7, 16


def probe_positions(T, block):
    """Every multiple of the block, the position before each, and 0, T - 2, T - 1: range starts are multiples of the block, so whatever S
    is, every wave-range edge and every block edge is among them."""
    pos = set(range(0, T, block)) | {t - 1 for t in range(block, T, block)} | {0, T - 2, T - 1}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def probe_case(i4, dtype):
    """T = 1000 (int4) | 500 (16-bit), N = 1: PROBE_B sequences that all name the same pages (decode only reads), PROBE_G query heads each;
    (b, h) is a spike at probe_positions[(b * g + h) % count].  -> profile_case's dict + targets [B, g], want [B, g, 128] (the V rows)."""
    T, block = (1000, 32) if i4 else (500, 16)
    B, g, P = PROBE_B, PROBE_G, PROBE_P
    pos = probe_positions(T, block)
    assert len(pos) <= B * g
    targets = np.array([pos[i % len(pos)] for i in range(B * g)]).reshape(B, g)
    pages, ip1, idx1, last1 = make_tables((T,), P, seed=T)
    rows = profile_rows("spike", (T,), 1, seed=T + 1)
    data, param = rows_to_cache(pages, 2, P, (ip1, idx1, last1), (T,), 1, *rows, i4, dtype)
    cnt = len(idx1)
    indptr, indices, last = (np.arange(B + 1) * cnt).astype(np.int32), np.tile(idx1, B).astype(np.int32), np.repeat(last1, B).astype(np.int32)
    q = profile_q("spike", (T,) * B, 1, g, np.tile(rows[0], (B, 1, 1)), targets)
    ref, (spa, qa) = paged_attention_f64(q, data, param, indptr, indices, last, 1, i4=i4)
    v_codes, v_param = rows[2], rows[3]
    V = v_codes[:, 0].astype(np.float64) * v_param[:, 0, 0:1].astype(np.float64) - v_param[:, 0, 1:2].astype(np.float64)
    S = decode_splits(B, g, 1, len(indices), P)
    n = np.full((B, 1, 1), float(accumulation_chain(T, S, block)))
    return dict(P=P, lens=(T,) * B, N=1, S=S, layer=1, pages=pages, data=data, param=param, tables=(indptr, indices, last), q=q, ref=ref,
                spa=spa, qa=qa, n=n, targets=targets, want=V[targets], T=T, block=block)


def spike_gap(case):
    """min over (b, h) of (the target's fp64 score - the largest other score) for a spike case with N = 1."""
    indptr, indices, last = case["tables"]
    i4 = case["data"].dtype == np.uint8
    gaps = []
    for b in range(len(case["lens"])):
        kr, kp = gather_rows(case["data"], case["param"], indptr, indices, last, case["layer"], b, 0, 0)
        K = dequantize_f32(kr, kp).astype(np.float64) if i4 else kr.astype(np.float64)
        sc = (K @ case["q"][b].T) * SM_SCALE                          # [T, g]
        for h in range(sc.shape[1]):
            t = int(case["targets"][b, h])
            gaps.append(sc[t, h] - np.delete(sc[:, h], t).max())
    return float(min(gaps))
