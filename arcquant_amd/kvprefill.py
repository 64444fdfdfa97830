"""Causal prefill attention over the int4 paged KV cache (include/arcq_kv.h ``arcq_kv_batch_prefill``, DESIGN.md 11 "Prefill"): several
query tokens per sequence, each attending over everything the pages hold up to and including its own position -- chunked prefill, a
second turn, verification of speculated tokens.  ``kvcache.batch_prefill_i4`` is this function: it lives in its own module, as
``kvstep.decode_step_i4`` does, because ``kvcache``'s own functions are the reference's six and their quantising pair.

A ctypes mirror only.  Validation follows the mirror's order: dtype / rank / contiguity, then the size relations, and LAST where
everything lives.  The CONTENTS of the index tensors (``qo_indptr`` included) are the caller's contract.
"""
from __future__ import annotations

import torch

from . import _lib
from ._kvargs import _DTYPES, HEAD_DIM, _cache, _dtype_of, _heads
from .agemm import _need, _on, _same_device, _stream


def batch_prefill_i4(o, q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """o[qo_indptr[b] + i, h] = softmax over positions 0 .. T_b - n_b + i of (q . K / sqrt(128)) V: the n_b = qo_indptr[b+1] - qo_indptr[b]
    query tokens of sequence b are its LAST positions, already written (``init_kv_*``) and counted by the tables (n_b <= T_b); o, q
    float16 or bfloat16 [tokens, Nq, 128], qo_indptr int32 [B + 1], query head h reads kv head h // g.  n_b = 1 everywhere is
    ``batch_decode_i4``; n_b = 0 and rows at or beyond qo_indptr[B] are not written.  Returns o."""
    who = "batch_prefill_i4"
    dtype = _dtype_of(f"kvcache.{who}", q)
    _need(q, dtype, "q", 3)
    _need(o, dtype, "o", 3)
    _need(qo_indptr, torch.int32, "qo_indptr", 1)
    L, N, P, B, layer_idx = _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, True)
    if qo_indptr.numel() != B + 1:
        raise RuntimeError(f"kvcache.{who}: qo_indptr has {qo_indptr.numel()} entries for {B} sequences, expected {B + 1}")
    if q.shape != o.shape or q.shape[2] != HEAD_DIM:
        raise RuntimeError(f"kvcache.{who}: o and q must be [tokens, Nq, {HEAD_DIM}], got {tuple(o.shape)} / {tuple(q.shape)}")
    ntok, Nq = q.shape[0], q.shape[1]
    _heads(f"kvcache.{who}", Nq, N)
    _same_device(f"kvcache.{who}", q, o, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset)
    with _on(q.device):
        st = _lib.lib().arcq_kv_batch_prefill(o.data_ptr(), q.data_ptr(), qo_indptr.data_ptr(), kv_data.data_ptr(), kv_param.data_ptr(),
                                              kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr(), ntok, B, Nq, L, layer_idx, N, P,
                                              kv_indices.numel(), _lib.KV_INT4, _DTYPES[dtype], _stream(q))
    _lib.check(st, f"kvcache.{who}")
    return o
