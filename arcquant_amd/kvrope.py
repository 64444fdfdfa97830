"""Rotary position embedding on the KV path (include/arcq_kv.h ``arcq_rope_qk``, ``arcq_kv_rope_append_quantize``,
``arcq_kv_rope_init_quantize``; DESIGN.md 11 "RoPE"): the reference's model path -- ``apply_rotary_pos_emb(q, k, cos, sin, position_ids)``
and then ``past_key_value.update`` -- so the int4 cache holds rotated keys and the attention operators stay as they are.

    cos, sin  float16 / bfloat16 [rope_len, 128], the Hugging Face tables (``rope_tables``); element i at position p reads cos[p, i]
    result    x * cos + rotate_half(x) * sin as torch eager computes it on a CPU tensor of that dtype, bit for bit (three roundings)

``rope_qk_`` rotates q and k in place.  ``rope_append_kv_quantize_i4`` / ``rope_init_kv_quantize_i4`` are ``kvcache``'s quantising writers
with the rotation of k in front and the rotation of q beside it, one launch: the position of a token is the one it is written at.  Every
position used must be below ``rope_len``: the caller's contract, like the index tables.

A ctypes mirror only, as ``kvcache`` is.  Validation follows the mirror's order: dtype / rank / layout, then the size relations, and LAST
where everything lives.
"""
from __future__ import annotations

import torch

from . import _lib
from ._kvargs import _DTYPES, HEAD_DIM, _cache, _dtype_of, _heads, _qkv_rows, _rope_tables, _row, _seqlens, _token_stride
from .agemm import _need, _on, _same_device, _stream


def rope_tables(rope_len: int, theta: float = 10000.0, dtype=torch.bfloat16, device=None):
    """(cos, sin), each ``dtype`` [rope_len, 128], as Hugging Face builds them: fp32 on the CPU, ``inv_freq = 1 / theta ** (arange(0, 128, 2)
    / 128)``, the outer product with the positions, ``cat((freqs, freqs))``, ``.cos()`` / ``.sin()``, ``.to(dtype)``; then moved to
    ``device``.  Computed on the CPU so that the tables are the same bits on every machine."""
    if int(rope_len) < 1:
        raise RuntimeError(f"kvrope.rope_tables: rope_len must be at least 1, got {rope_len}")
    if dtype not in _DTYPES:
        raise RuntimeError(f"kvrope.rope_tables: dtype must be float16 or bfloat16, got {dtype}")
    inv_freq = 1.0 / (float(theta) ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).float() / HEAD_DIM))
    freqs = torch.outer(torch.arange(int(rope_len), dtype=torch.int64).float(), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)
    return (cos, sin) if device is None else (cos.to(device), sin.to(device))


def rope_qk_(q, k, positions, cos, sin):
    """Rotate q ([tokens, Nq, 128]) and k ([tokens, N, 128], or None) IN PLACE: token i to ``positions[i % n_pos]``, positions int32
    [n_pos] with n_pos dividing the token count (n_pos = tokens: one position per token; q_len: a batch of equal-length sequences; 1: a
    decode step).  q and k may be views whose heads are contiguous and whose token strides are multiples of 8 elements.  Returns (q, k)."""
    who = "rope_qk_"
    dtype = _dtype_of(f"kvrope.{who}", q)
    _row(q, dtype, "q")
    if k is not None:
        _row(k, dtype, "k")
    _need(positions, torch.int32, "positions", 1)
    rope_len = _rope_tables(who, cos, sin, dtype)
    ntok, Nq = q.shape[0], q.shape[1]
    N = 0 if k is None else k.shape[1]
    if Nq < 1 or (k is not None and (k.shape[0] != ntok or N < 1 or Nq % N)):
        raise RuntimeError(f"kvrope.{who}: q [tokens, Nq, {HEAD_DIM}] and k [tokens, N, {HEAD_DIM}] need one token count and Nq a positive multiple "
                           f"of N, got {tuple(q.shape)} / {tuple(k.shape) if k is not None else None}")
    n_pos = positions.numel()
    if n_pos < 1 or ntok % n_pos:
        raise RuntimeError(f"kvrope.{who}: {n_pos} positions do not divide {ntok} tokens")
    _same_device(f"kvrope.{who}", q, k, positions, cos, sin)
    with _on(q.device):
        st = _lib.lib().arcq_rope_qk(q.data_ptr(), None if k is None else k.data_ptr(), _token_stride(q), 0 if k is None else _token_stride(k),
                                     positions.data_ptr(), n_pos, cos.data_ptr(), sin.data_ptr(), rope_len, ntok, Nq, N, _DTYPES[dtype], _stream(q))
    _lib.check(st, f"kvrope.{who}")
    return q, k


def _rope_write(who, init, q_out, q, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, seqlen_indptr, layer_idx):
    dtype = _dtype_of(f"kvrope.{who}", q)
    _need(q_out, dtype, "q_out", 3)
    _qkv_rows(f"kvrope.{who}", q, k, v, dtype)
    rope_len = _rope_tables(who, cos, sin, dtype)
    L, N, P, B, layer_idx = _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, True)
    if init:
        _seqlens(who, seqlen_indptr, B)
    ntok, Nq = q.shape[0], q.shape[1]
    if q_out.shape != q.shape or (not init and ntok != B):
        raise RuntimeError(f"kvrope.{who}: q_out and q must be [{'tokens' if init else B}, Nq, {HEAD_DIM}], got {tuple(q_out.shape)} / {tuple(q.shape)}")
    if k.shape != v.shape or tuple(k.shape[:2]) != (ntok, N):
        raise RuntimeError(f"kvrope.{who}: k and v must be [{ntok}, {N}, {HEAD_DIM}], got {tuple(k.shape)} / {tuple(v.shape)}")
    _heads(f"kvrope.{who}", Nq, N)
    _same_device(f"kvrope.{who}", q, q_out, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, seqlen_indptr)
    lib = _lib.lib()
    with _on(q.device):
        head = (kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr(), q_out.data_ptr(),
                q.data_ptr(), k.data_ptr(), v.data_ptr(), _token_stride(q), _token_stride(k), cos.data_ptr(), sin.data_ptr(), rope_len)
        tail = (B, Nq, L, layer_idx, N, P, _lib.KV_INT4, _DTYPES[dtype], _stream(q))
        if init:
            st = lib.arcq_kv_rope_init_quantize(*head, seqlen_indptr.data_ptr(), ntok, *tail)
        else:
            st = lib.arcq_kv_rope_append_quantize(*head, *tail)
    _lib.check(st, f"kvrope.{who}")
    return q_out


def rope_append_kv_quantize_i4(q_out, q, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """One launch for what a decode step does in front of attention: rotate q ([B, Nq, 128]) and k ([B, N, 128]) to the position the
    token is written at (seq_len - 1), write the rotated q into ``q_out`` ([B, Nq, 128], contiguous; it may be q itself when q is
    contiguous), quantise the rotated k and v and store them in the int4 pages.  Byte for byte ``rope_qk_`` + ``kvcache.append_kv_quantize_i4``
    + a copy of q.  q, k and v may be slices of one projection output (``kvstep``'s rules).  Returns q_out."""
    return _rope_write("rope_append_kv_quantize_i4", False, q_out, q, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset,
                       None, layer_idx)


def rope_init_kv_quantize_i4(q_out, q, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, seqlen_indptr, layer_idx):
    """The same in front of ``kvcache.init_kv_quantize_i4``: tokens seqlen_indptr[b] .. seqlen_indptr[b+1] become the last positions of
    sequence b and are rotated to them; rows of q_out at or beyond seqlen_indptr[B] are not written.  Returns q_out."""
    return _rope_write("rope_init_kv_quantize_i4", True, q_out, q, k, v, cos, sin, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset,
                       seqlen_indptr, layer_idx)
