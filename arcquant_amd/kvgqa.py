"""Decode attention over the paged KV cache for GQA models (include/arcq_kv.h ``arcq_kv_batch_decode_gqa`` over int4 pages,
``arcq_kv_batch_decode_gqa_16bit`` over 16-bit pages; DESIGN.md 11 "GQA decode on MFMA" and "GQA decode over a 16-bit cache"):
``batch_decode_i4``'s / ``batch_decode_f16``'s arguments, checks and result with the g = Nq / N <= 16 query heads of a kv head as the
columns of one MFMA tile, so every K and V row is read once whatever g is.  ``kvcache.batch_decode_gqa_i4`` and
``kvcache.batch_decode_gqa_f16`` are these functions: they live in their own module, as ``kvprefill.batch_prefill_i4`` does, because
``kvcache``'s own functions are the reference's six and their quantising pair.  The argument checks are ``kvcache._decode``'s -- one set
for all the decode entry points.
"""
from __future__ import annotations


def batch_decode_gqa_i4(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """o[b, h] = softmax(q[b, h] . K / sqrt(128)) V over sequence b's positions of an int4 cache; o, q float16 or bfloat16 [B, Nq, 128],
    Nq = g N with g <= 16, query head h reads kv head h // g.  Agrees with ``batch_decode_i4`` within the two kernels' error bounds (the
    weights p_t s_t are rounded once to q's dtype for the matrix cores), not bit for bit.  Allocates its own workspace.  Returns o."""
    from . import kvcache
    return kvcache._decode("batch_decode_gqa_i4", True, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, gqa=True)


def batch_decode_gqa_f16(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """The same over a 16-bit cache of q's dtype (float16 or bfloat16 pages [pages, L, 2, N, P, 128]; kv_param is checked and never read).
    Agrees with ``batch_decode_f16`` within the two kernels' error bounds (the weights p_t are rounded once to q's dtype for the matrix
    cores), not bit for bit.  Allocates its own workspace.  Returns o."""
    from . import kvcache
    return kvcache._decode("batch_decode_gqa_f16", False, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, gqa=True)
