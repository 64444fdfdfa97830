"""The decode step of the int4 paged KV cache in one launch (include/arcq_kv.h ``arcq_kv_decode_step``): what
``kvcache.append_kv_quantize_i4`` followed by ``kvcache.batch_decode_i4`` computes -- pages, parameters and ``o`` bit for bit -- without
the launches in between.  ``q``, ``k`` and ``v`` may be slices of one ``[B, (Nq + 2 N) * 128]`` projection output, so the transposing
copy in front of the chain goes as well; the slices of a sequence are merged inside the launch by the last workgroup to arrive.

A ctypes mirror only, as ``kvcache`` is.  Validation follows the mirror's order: dtype / rank / layout, then the size relations, and LAST
where everything lives.  The CONTENTS of the index tensors are the caller's contract.
"""
from __future__ import annotations

import torch

from . import _lib
from ._kvargs import _DTYPES, HEAD_DIM, _cache, _dtype_of, _heads, _qkv_rows, _token_stride
from .agemm import _need, _on, _same_device, _stream

_MAX_SLICES = 32          # the most slices per sequence arcq_kv_decode_workspace_bytes ever answers for (kv_decode_splits' cap, kv_cache.hip)
_RECORD = HEAD_DIM + 2    # floats of a slice's record: max, sum, 128 accumulators


class DecodeStepState:
    """What ``decode_step_i4`` keeps between calls for a batch of ``batch_size`` sequences: the arrival counters (zeroed here, once; every
    call leaves them zero) and the record scratch for the most slices a call can use.  Nothing is allocated afterwards, so a step that is
    given one can be captured in a graph.  Calls that share a state are stream-ordered."""

    def __init__(self, batch_size: int, num_q_heads: int, num_kv_heads: int, device):
        if batch_size < 1 or num_kv_heads < 1 or num_q_heads < 1 or num_q_heads % num_kv_heads:
            raise RuntimeError(f"kvstep.DecodeStepState: need batch_size >= 1 and num_q_heads a positive multiple of num_kv_heads, got "
                               f"{batch_size}, {num_q_heads}, {num_kv_heads}")
        self.batch_size, self.num_q_heads, self.num_kv_heads = batch_size, num_q_heads, num_kv_heads
        n = int(_lib.lib().arcq_kv_decode_step_state_bytes(batch_size, num_q_heads, num_kv_heads)) // 4
        self.counters = torch.zeros(n, dtype=torch.int32, device=device)
        self.workspace = torch.empty(batch_size * num_q_heads * _MAX_SLICES * _RECORD, dtype=torch.float32, device=device)


def decode_step_i4(o, q, k, v, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, state=None):
    """Quantise and store this token's k, v (float16 or bfloat16 [B, N, 128]) at position seq_len - 1 of an int4 cache, attend q
    ([B, Nq, 128]) over the sequence including it and write o ([B, Nq, 128], contiguous): one launch, bit for bit
    ``append_kv_quantize_i4`` + ``batch_decode_i4``.  The tables describe the sequences including the new position.  q, k and v may be
    views whose heads are contiguous and whose token strides are multiples of 8 elements (k's and v's equal).  ``state``: a
    ``DecodeStepState`` of this batch and head counts; None allocates one for the call (a zero-fill launch more)."""
    who = "decode_step_i4"
    dtype = _dtype_of(f"kvstep.{who}", q)
    _need(o, dtype, "o", 3)
    _qkv_rows(f"kvstep.{who}", q, k, v, dtype)
    if state is not None and not isinstance(state, DecodeStepState):
        raise RuntimeError(f"kvstep.{who}: state must be a DecodeStepState or None, got {type(state)}")
    L, N, P, B, layer_idx = _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, True)
    if q.shape != o.shape or q.shape[0] != B:
        raise RuntimeError(f"kvstep.{who}: o and q must be [{B}, Nq, {HEAD_DIM}], got {tuple(o.shape)} / {tuple(q.shape)}")
    if k.shape != v.shape or tuple(k.shape[:2]) != (B, N):
        raise RuntimeError(f"kvstep.{who}: k and v must be [{B}, {N}, {HEAD_DIM}], got {tuple(k.shape)} / {tuple(v.shape)}")
    Nq = q.shape[1]
    _heads(f"kvstep.{who}", Nq, N)
    if state is not None and (state.batch_size, state.num_q_heads, state.num_kv_heads) != (B, Nq, N):
        raise RuntimeError(f"kvstep.{who}: the state was built for (batch, Nq, N) = {(state.batch_size, state.num_q_heads, state.num_kv_heads)}, "
                           f"the call has {(B, Nq, N)}")
    _same_device(f"kvstep.{who}", q, o, k, v, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset,
                 *(() if state is None else (state.counters, state.workspace)))
    lib, nnz = _lib.lib(), kv_indices.numel()
    ws_bytes = int(lib.arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P))
    if state is None and ws_bytes:
        state = DecodeStepState(B, Nq, N, q.device)
    ws, cnt = (None, None) if state is None else (state.workspace, state.counters)
    with _on(q.device):
        st = lib.arcq_kv_decode_step(o.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), _token_stride(q), _token_stride(k), kv_data.data_ptr(),
                                     kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr(), B, Nq, L, layer_idx, N,
                                     P, nnz, _lib.KV_INT4, _DTYPES[dtype], None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                                     None if cnt is None else cnt.data_ptr(), 0 if cnt is None else cnt.numel() * 4, _stream(q))
    _lib.check(st, f"kvstep.{who}")
    return o
