"""Decode attention over the int4 paged KV cache for GQA models (include/arcq_kv.h ``arcq_kv_batch_decode_gqa``, DESIGN.md 11 "GQA decode
on MFMA"): ``batch_decode_i4``'s arguments, checks and result with the g = Nq / N <= 16 query heads of a kv head as the columns of one
MFMA tile, so every K and V row is read and converted once whatever g is.  ``kvcache.batch_decode_gqa_i4`` is this function: it lives in
its own module, as ``kvprefill.batch_prefill_i4`` does, because ``kvcache``'s own functions are the reference's six and their quantising
pair.  The argument checks are ``kvcache._decode``'s -- one set for the two decode entry points.
"""
from __future__ import annotations


def batch_decode_gqa_i4(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """o[b, h] = softmax(q[b, h] . K / sqrt(128)) V over sequence b's positions of an int4 cache; o, q float16 or bfloat16 [B, Nq, 128],
    Nq = g N with g <= 16, query head h reads kv head h // g.  Agrees with ``batch_decode_i4`` within the two kernels' error bounds (the
    weights p_t s_t are rounded once to q's dtype for the matrix cores), not bit for bit.  Allocates its own workspace.  Returns o."""
    from . import kvcache
    return kvcache._decode("batch_decode_gqa_i4", True, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, gqa=True)
