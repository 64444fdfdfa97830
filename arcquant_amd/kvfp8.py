"""The FP8 (OCP e4m3) paged KV cache (include/arcq_kv.h "The FP8 cache", DESIGN.md 11 "FP8 cache"; what vLLM calls kv_cache_dtype=fp8):
quantising writers and the GQA decode attention that reads what they wrote.

    kv_data   torch.float8_e4m3fn [pages, L, 2, N, P, 128] -- a row is 128 bytes, one cache line
    kv_param  float16 [pages, L, 2, N, P, 2] = (scale, 0); value = float(code) * float(scale); the second element is written as zero and
              never read.  Tables (kv_indptr, kv_indices, last_page_offset) as in ``kvcache``.

``kvcache.append_kv_quantize_fp8``, ``init_kv_quantize_fp8``, ``batch_decode_gqa_fp8`` and ``quantize_fp8`` are these functions: they live
in their own module, as ``kvgqa``'s do.  The cache check is written here because ``_kvargs._cache`` has no words for an 8-bit float cache;
validation keeps the mirror's order -- dtype / rank / contiguity, then the size relations, and LAST where the tensors live -- and every
rejection is a RuntimeError that starts ``kvcache.<function>:``.
"""
from __future__ import annotations

import torch

from . import _lib
from ._kvargs import _DTYPES, HEAD_DIM
from .agemm import _on, _stream

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0


def quantize_fp8(x: torch.Tensor):
    """The quantiser's rule as torch ops: x float16 / bfloat16 [..., 128] -> (codes float8_e4m3fn [..., 128], scale float16 [..., 1]),
    fp32 arithmetic.  The clamp is part of the rule: torch's conversion does not saturate, and a scale rounded down to fp16 can leave a
    quotient a hair above 448.  The kernels' bytes are this formula's on a CPU tensor."""
    if getattr(x, "dtype", None) not in _DTYPES:
        raise RuntimeError(f"kvcache.quantize_fp8: x must be a float16 or bfloat16 tensor, got {getattr(x, 'dtype', type(x))}")
    amax = x.float().abs().amax(-1, keepdim=True)
    scale = (amax / FP8_MAX).clamp(min=2.0 ** -14).to(torch.float16)
    code = (x.float() / scale.float()).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return code, scale


def _tensor(who, t, dtype, name, ndim):
    if getattr(t, "dtype", None) is not dtype:
        raise RuntimeError(f"kvcache.{who}: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != ndim:
        raise RuntimeError(f"kvcache.{who}: {name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"kvcache.{who}: {name} must be contiguous")


def _row_dtype(who, t, name):
    dtype = getattr(t, "dtype", None)
    if dtype not in _DTYPES:
        raise RuntimeError(f"kvcache.{who}: {name} must be a float16 or bfloat16 tensor, got {getattr(t, 'dtype', type(t))}")
    return dtype


def _cache_layout(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset):
    _tensor(who, kv_data, FP8, "kv_data", 6)
    _tensor(who, kv_param, torch.float16, "kv_param", 6)
    _tensor(who, kv_indptr, torch.int32, "kv_indptr", 1)
    _tensor(who, kv_indices, torch.int32, "kv_indices", 1)
    _tensor(who, last_page_offset, torch.int32, "last_page_offset", 1)


def _cache_sizes(who, kv_data, kv_param, kv_indptr, last_page_offset, layer_idx):
    """-> (L, N, P, B, layer_idx)."""
    pages, L, two, N, P, row = kv_data.shape
    if two != 2 or row != HEAD_DIM:
        raise RuntimeError(f"kvcache.{who}: kv_data must be [pages, L, 2, N, P, {HEAD_DIM}] (head dimension {HEAD_DIM} only), got {tuple(kv_data.shape)}")
    if tuple(kv_param.shape) != (pages, L, 2, N, P, 2):
        raise RuntimeError(f"kvcache.{who}: kv_param must be {(pages, L, 2, N, P, 2)}, got {tuple(kv_param.shape)}")
    if L < 1 or N < 1 or P < 1:
        raise RuntimeError(f"kvcache.{who}: the cache needs at least one layer, head and page entry, got {tuple(kv_data.shape)}")
    layer_idx = int(layer_idx)
    if not 0 <= layer_idx < L:
        raise RuntimeError(f"kvcache.{who}: layer_idx={layer_idx} is not a layer of a cache with {L}")
    B = last_page_offset.numel()
    if kv_indptr.numel() != B + 1:
        raise RuntimeError(f"kvcache.{who}: kv_indptr has {kv_indptr.numel()} entries for {B} sequences (last_page_offset), expected {B + 1}")
    return L, N, P, B, layer_idx


def _on_one_gpu(who, first, *ts):
    idx = first.get_device()
    if idx < 0:
        raise RuntimeError(f"kvcache.{who}: the operands must live on the GPU (there is no CPU path)")
    for t in ts:
        if t.get_device() != idx:
            raise RuntimeError(f"kvcache.{who}: every operand must live on the GPU of the first one ({first.device}), got {t.device}")


def _write(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, seqlen_indptr, layer_idx):
    init = who.startswith("init")
    dtype = _row_dtype(who, k, "k")
    _cache_layout(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset)
    if init:
        _tensor(who, seqlen_indptr, torch.int32, "seqlen_indptr", 1)
    _tensor(who, k, dtype, "k", 3)
    _tensor(who, v, dtype, "v", 3)
    L, N, P, B, layer_idx = _cache_sizes(who, kv_data, kv_param, kv_indptr, last_page_offset, layer_idx)
    if init and seqlen_indptr.numel() != B + 1:
        raise RuntimeError(f"kvcache.{who}: seqlen_indptr has {seqlen_indptr.numel()} entries for {B} sequences, expected {B + 1}")
    if k.shape != v.shape or tuple(k.shape[1:]) != (N, HEAD_DIM) or (not init and k.shape[0] != B):
        raise RuntimeError(f"kvcache.{who}: k and v must be [{'tokens' if init else B}, {N}, {HEAD_DIM}], got {tuple(k.shape)} / {tuple(v.shape)}")
    _on_one_gpu(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, *((seqlen_indptr,) if init else ()))
    lib, ntok = _lib.lib(), k.shape[0]
    with _on(kv_data.device):
        tables = (kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr())
        if init:
            st = lib.arcq_kv_fp8_init_quantize(*tables, k.data_ptr(), v.data_ptr(), seqlen_indptr.data_ptr(), ntok, B, L, layer_idx, N, P,
                                               _DTYPES[dtype], _stream(kv_data))
        else:
            st = lib.arcq_kv_fp8_append_quantize(*tables, k.data_ptr(), v.data_ptr(), B, L, layer_idx, N, P, _DTYPES[dtype], _stream(kv_data))
    _lib.check(st, f"kvcache.{who}")


def append_kv_quantize_fp8(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, layer_idx):
    """``quantize_fp8`` of k and v (float16 or bfloat16 [B, N, 128]) written at position seq_len - 1 of each sequence, one launch; codes
    and scales byte for byte what ``quantize_fp8`` gives on a CPU tensor, the second parameter zero."""
    _write("append_kv_quantize_fp8", kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, None, layer_idx)


def init_kv_quantize_fp8(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, seqlen_indptr, layer_idx):
    """The same for k, v [tokens, N, 128]: tokens seqlen_indptr[b] .. seqlen_indptr[b+1] become the last positions of sequence b."""
    _write("init_kv_quantize_fp8", kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, seqlen_indptr, layer_idx)


def batch_decode_gqa_fp8(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """o[b, h] = softmax(q[b, h] . K / sqrt(128)) V over sequence b's positions of an FP8 cache; o, q float16 or bfloat16 [B, Nq, 128],
    Nq = g N with 1 <= g <= 16, query head h reads kv head h // g.  The codes are converted exactly to q's dtype and multiplied on the
    16-bit matrix cores; the row scales multiply the fp32 score and the fp32 weight, which is rounded once to q's dtype.  Allocates its own
    workspace.  Returns o."""
    who = "batch_decode_gqa_fp8"
    dtype = _row_dtype(who, q, "q")
    _tensor(who, q, dtype, "q", 3)
    _tensor(who, o, dtype, "o", 3)
    _cache_layout(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset)
    L, N, P, B, layer_idx = _cache_sizes(who, kv_data, kv_param, kv_indptr, last_page_offset, layer_idx)
    if q.shape != o.shape or q.shape[0] != B or q.shape[2] != HEAD_DIM:
        raise RuntimeError(f"kvcache.{who}: o and q must be [{B}, Nq, {HEAD_DIM}], got {tuple(o.shape)} / {tuple(q.shape)}")
    Nq = q.shape[1]
    if Nq < 1 or Nq % N:
        raise RuntimeError(f"kvcache.{who}: {Nq} query heads are not a multiple of the cache's {N} kv heads")
    if Nq // N > 16:
        raise RuntimeError(f"kvcache.{who}: {Nq // N} query heads per kv head, at most 16")
    _on_one_gpu(who, q, o, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset)
    lib, nnz = _lib.lib(), kv_indices.numel()
    ws_bytes = int(lib.arcq_kv_decode_gqa_workspace_bytes(B, Nq, N, nnz, P))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device) if ws_bytes else None
    with _on(q.device):
        st = lib.arcq_kv_batch_decode_gqa_fp8(o.data_ptr(), q.data_ptr(), kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(),
                                              kv_indices.data_ptr(), last_page_offset.data_ptr(), B, Nq, L, layer_idx, N, P, nnz, _DTYPES[dtype],
                                              None if ws is None else ws.data_ptr(), ws_bytes, _stream(q))
    _lib.check(st, f"kvcache.{who}")
    return o
