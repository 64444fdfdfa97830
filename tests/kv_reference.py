"""The paged KV-cache format of include/arcq_kv.h restated with numpy / torch on the CPU: offset arithmetic, the quantiser and its
inverse, the writers and an fp64 paged attention that walks the tables.  Test infrastructure: slow, plain and independent of the library.

    kv_data   uint8 [pages, L, 2, N, P, 64] (int4) | 16-bit [pages, L, 2, N, P, 128];  kv_param float16 [pages, L, 2, N, P, 2]
    byte j of an int4 row = element 2j (low nibble) | element 2j+1 (high nibble);  value = float(code) * float(scale) - float(zero)
    sequence b: pages kv_indices[kv_indptr[b] .. kv_indptr[b+1]), (count - 1) * P + last_page_offset[b] positions
"""
from __future__ import annotations

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
    return (ip[1:] - ip[:-1] - 1) * P + lp


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
            page, e = locate(kv_indptr, kv_indices, b, pos, P)
            kv_data[page, layer, 0, :, e] = k[tok]
            kv_data[page, layer, 1, :, e] = v[tok]
            kv_param[page, layer, 0, :, e] = k_param[tok]
            kv_param[page, layer, 1, :, e] = v_param[tok]
            written.append((page, e))
    return written


def gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, head, which):
    """The valid rows of one sequence and head, in position order -> (rows [T, row], params float16 [T, 2])."""
    P = kv_data.shape[4]
    T = int(seq_lens(kv_indptr, last_page_offset, P)[b])
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
    passed as float64 values."""
    B, Nq, _ = q.shape
    N = kv_data.shape[3]
    g = Nq // N
    out, spa, qa = np.zeros((B, Nq, D)), np.zeros((B, Nq, D)), np.zeros((B, Nq))
    for b in range(B):
        for n in range(N):
            kr, kp = gather_rows(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer, b, n, 0)
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


def decode_bound(ref, spa, qa, u):
    """|got - ref| <= u |ref| + (2 Delta + 2^-20) sum_t p_t a_td,  Delta = 130 * 2^-24 * sm_scale * max_t sum_d |q_d| a_td."""
    delta = 130.0 * 2.0 ** -24 * qa
    return u * np.abs(ref) + (2.0 * delta[..., None] + 2.0 ** -20) * spa


# ---- table construction for the tests
def make_tables(lens, P, seed=0, spare=2):
    """A shuffled, non-contiguous page assignment for sequences of ``lens`` positions, with unused pages in between ->
    (pages, kv_indptr int32 [B+1], kv_indices int32 [nnz], last_page_offset int32 [B])."""
    cnt = [(n + P - 1) // P for n in lens]
    nnz = sum(cnt)
    pages = nnz * spare + 1
    rng = np.random.default_rng(seed)
    indices = rng.permutation(pages)[:nnz].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    last = np.array([n - (c - 1) * P for n, c in zip(lens, cnt)], dtype=np.int32)
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
