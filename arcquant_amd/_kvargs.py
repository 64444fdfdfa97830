"""The argument checks that ``kvcache``, ``kvstep``, ``kvprefill`` and ``kvrope`` share: each relation and each message once.  The four
validate in one order -- dtype / rank / layout, then the size relations, and LAST where everything lives -- and the exact text of every
rejection is recorded in tests/golden/kv_python_rejections.json.  The prefixes are part of those texts: the cache's checks report as
``kvcache.<function>`` and the row layout as ``kvstep``, whichever module calls them; ``who`` is the caller's function name where the
prefix is fixed, and ``module.function`` where it is the caller's.  Nothing here touches a tensor's contents or asks for a device.
"""
from __future__ import annotations

import torch

from . import _lib
from .agemm import _need

HEAD_DIM = 128
_DTYPES = {torch.float16: _lib.KV_F16, torch.bfloat16: _lib.KV_BF16}


def _dtype_of(who, t, name="q"):
    """The 16-bit dtype of a call: that of its ``name`` tensor."""
    dtype = getattr(t, "dtype", None)
    if dtype not in _DTYPES:
        raise RuntimeError(f"{who}: {name} must be a float16 or bfloat16 tensor, got {getattr(t, 'dtype', type(t))}")
    return dtype


def _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, i4, dtype16=None):
    """dtype / rank / contiguity of the cache and its tables, then their size relations -> (L, N, P, B, layer_idx)."""
    if i4:
        _need(kv_data, torch.uint8, "kv_data", 6)
    else:
        if dtype16 is None:
            dtype16 = kv_data.dtype if getattr(kv_data, "dtype", None) in _DTYPES else torch.float16
        _need(kv_data, dtype16, "kv_data", 6)
    _need(kv_param, torch.float16, "kv_param", 6)
    _need(kv_indptr, torch.int32, "kv_indptr", 1)
    _need(kv_indices, torch.int32, "kv_indices", 1)
    _need(last_page_offset, torch.int32, "last_page_offset", 1)
    pages, L, two, N, P, row = kv_data.shape
    if two != 2 or row != (HEAD_DIM // 2 if i4 else HEAD_DIM):
        raise RuntimeError(f"kvcache.{who}: kv_data must be [pages, L, 2, N, P, {HEAD_DIM // 2 if i4 else HEAD_DIM}] (head dimension {HEAD_DIM} "
                           f"only), got {tuple(kv_data.shape)}")
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


def _rows(who, k, v, dtype, N, row, ntok=None):
    for t, name in ((k, "k"), (v, "v")):
        _need(t, dtype, name, 3)
    if k.shape != v.shape or tuple(k.shape[1:]) != (N, row) or (ntok is not None and k.shape[0] != ntok):
        raise RuntimeError(f"kvcache.{who}: k and v must be [{'tokens' if ntok is None else ntok}, {N}, {row}], got {tuple(k.shape)} / {tuple(v.shape)}")


def _params(who, k_param, v_param, ntok, N):
    for t, name in ((k_param, "k_param"), (v_param, "v_param")):
        _need(t, torch.float16, name, 3)
        if tuple(t.shape) != (ntok, N, 2):
            raise RuntimeError(f"kvcache.{who}: {name} must be [{ntok}, {N}, 2], got {tuple(t.shape)}")


def _seqlens(who, seqlen_indptr, B):
    _need(seqlen_indptr, torch.int32, "seqlen_indptr", 1)
    if seqlen_indptr.numel() != B + 1:
        raise RuntimeError(f"kvcache.{who}: seqlen_indptr has {seqlen_indptr.numel()} entries for {B} sequences, expected {B + 1}")


def _heads(who, Nq, N):
    if Nq < 1 or Nq % N:
        raise RuntimeError(f"{who}: {Nq} query heads are not a multiple of the cache's {N} kv heads")


def _row(t, dtype, name):
    """q / k / v: 3-D of ``dtype``, heads 128 elements apart, tokens a multiple of 8 elements apart (a view is fine)."""
    if getattr(t, "dtype", None) is not dtype:
        raise RuntimeError(f"kvstep: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 3:
        raise RuntimeError(f"kvstep: {name} must be 3-D, got shape {tuple(t.shape)}")
    if t.shape[2] != HEAD_DIM or t.stride(2) != 1 or (t.shape[1] > 1 and t.stride(1) != HEAD_DIM):
        raise RuntimeError(f"kvstep: {name} must be [tokens, heads, {HEAD_DIM}] with contiguous heads (strides (s, {HEAD_DIM}, 1)), got shape "
                           f"{tuple(t.shape)} strides {tuple(t.stride())}")
    if t.shape[0] > 1 and (t.stride(0) % 8 or t.stride(0) < t.shape[1] * HEAD_DIM):
        raise RuntimeError(f"kvstep: {name}'s token stride {t.stride(0)} must be a multiple of 8 elements and at least {t.shape[1] * HEAD_DIM}")


def _token_stride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * HEAD_DIM       # (the stride of a dimension of one entry says nothing)


def _qkv_rows(who, q, k, v, dtype):
    """``_row`` of q, k and v, k's and v's tokens equally far apart."""
    _row(q, dtype, "q")
    _row(k, dtype, "k")
    _row(v, dtype, "v")
    if _token_stride(k) != _token_stride(v):
        raise RuntimeError(f"{who}: k and v must have one token stride, got {k.stride(0)} / {v.stride(0)}")


def _rope_tables(who, cos, sin, dtype):
    """cos, sin: ``dtype`` [rope_len, 128] -> rope_len."""
    _need(cos, dtype, "cos", 2)
    _need(sin, dtype, "sin", 2)
    if cos.shape != sin.shape or cos.shape[1] != HEAD_DIM or cos.shape[0] < 1:
        raise RuntimeError(f"kvrope.{who}: cos and sin must be [rope_len, {HEAD_DIM}] with rope_len >= 1, got {tuple(cos.shape)} / {tuple(sin.shape)}")
    return cos.shape[0]
