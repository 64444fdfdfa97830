"""The KV-cache half of the reference's operator module (include/arcq_kv.h): ``init_kv_*``, ``append_kv_*`` and
``batch_decode_*`` over the reference's paged cache, int4 (``_i4``) or 16-bit (``_f16``), under the reference's names, positional order and
keyword names (model/kv_cache.py:45-110) -- a ``kernels/build/agemm.py`` shim forwards to them.  ``agemm``'s own six
functions of these names stay ``NotImplementedError`` stubs.

    kv_data   uint8 [pages, L, 2, N, P, 64] (int4: element 2j in the low nibble of byte j) | 16-bit [pages, L, 2, N, P, 128]
    kv_param  float16 [pages, L, 2, N, P, 2] = (scale, zero); value = float(code) * float(scale) - float(zero)
    kv_indptr int32 [B + 1], kv_indices int32 [nnz], last_page_offset int32 [B]; a sequence holds
              (kv_indptr[b+1] - kv_indptr[b] - 1) * P + last_page_offset[b] positions, those being written included.

Extensions: ``append_kv_quantize_i4`` / ``init_kv_quantize_i4`` quantise fp16 / bf16 rows and write them in one launch (the reference:
five torch launches per tensor, then the append); ``batch_decode_*`` also takes bf16 and ``Nq = g * N`` query heads (GQA: query head h
reads kv head h // g).  ``asym_quantize_and_pack_i4`` / ``unpack_i4_and_asym_dequantize`` are the torch formulas for callers that keep the
reference's flow, ``PagedKVCacheI4`` holds the pages and builds the tables.  ``batch_prefill_i4`` (kvprefill.py) is the causal attention
of several query tokens per sequence over the int4 pages: chunked prefill, a second turn, speculative verification.

This module is a ctypes mirror only.  Validation follows the mirror's order (``agemm._need`` ...): dtype / rank / contiguity, then the size
relations, and LAST where everything lives.  The CONTENTS of the index tensors are the caller's contract, as in the reference.
"""
from __future__ import annotations

import torch

from . import _lib
from ._kvargs import _DTYPES, HEAD_DIM, _cache, _dtype_of, _heads, _params, _rows, _seqlens
from .agemm import _need, _on, _same_device, _stream
# extensions in modules of their own, as kvstep is: causal prefill attention over the int4 pages (several query tokens per sequence), and
# rotary position embedding at write time, fused into the quantising writers
from .kvprefill import batch_prefill_i4  # noqa: F401
from .kvrope import rope_append_kv_quantize_i4, rope_init_kv_quantize_i4, rope_qk_, rope_tables  # noqa: F401


# ---- the quantiser as torch ops (model/kv_cache.py:22-40 computes the same)
def asym_quantize_and_pack_i4(x: torch.Tensor):
    """Per-row asymmetric 4-bit quantisation over the last dimension -> (codes uint8 [..., D/2], scale [..., 1], zero [..., 1]), the
    parameters in x's dtype: scale = max(amax - amin, 1e-5) / 15, zero = -amin, code = clamp(round((x + zero) / scale), 0, 15); element
    2j goes to the low nibble of byte j."""
    hi, lo = x.amax(dim=-1, keepdim=True), x.amin(dim=-1, keepdim=True)
    scale = (hi - lo).clamp(min=1e-5) / 15
    zero = -lo
    codes = ((x + zero) / scale).round().clamp(0, 15).to(torch.uint8)
    return codes[..., 0::2] | (codes[..., 1::2] << 4), scale, zero


def unpack_i4_and_asym_dequantize(q: torch.Tensor, scale: torch.Tensor, zero: torch.Tensor):
    """The inverse: codes uint8 [..., D/2] -> [..., D] values ``code * scale - zero``."""
    if q.dtype is not torch.uint8:
        raise RuntimeError(f"kvcache.unpack_i4_and_asym_dequantize: q must be uint8, got {q.dtype}")
    codes = torch.stack((q & 0x0F, q >> 4), dim=-1).reshape(*q.shape[:-1], q.shape[-1] * 2)
    return codes * scale - zero


# ---- the calls (the argument checks they share with kvstep, kvprefill and kvrope: _kvargs.py)
def _write(who, i4, quantize, init, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer_idx):
    row_dtype = _dtype_of(f"kvcache.{who}", k, "k") if quantize else None
    L, N, P, B, layer_idx = _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, i4)
    if init:
        _seqlens(who, seqlen_indptr, B)
    if quantize:
        _rows(who, k, v, row_dtype, N, HEAD_DIM, None if init else B)
    else:
        _rows(who, k, v, kv_data.dtype, N, kv_data.shape[-1], None if init else B)
        _params(who, k_param, v_param, k.shape[0], N)
    _same_device(f"kvcache.{who}", kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr)
    fmt = _lib.KV_INT4 if i4 else _lib.KV_16BIT
    lib, ntok = _lib.lib(), k.shape[0]
    with _on(kv_data.device):
        tables = (kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(), last_page_offset.data_ptr())
        if quantize and init:
            st = lib.arcq_kv_init_quantize(*tables, k.data_ptr(), v.data_ptr(), seqlen_indptr.data_ptr(), ntok, B, L, layer_idx, N, P, fmt,
                                           _DTYPES[row_dtype], _stream(kv_data))
        elif quantize:
            st = lib.arcq_kv_append_quantize(*tables, k.data_ptr(), v.data_ptr(), B, L, layer_idx, N, P, fmt, _DTYPES[row_dtype], _stream(kv_data))
        elif init:
            st = lib.arcq_kv_init(*tables, k.data_ptr(), v.data_ptr(), k_param.data_ptr(), v_param.data_ptr(), seqlen_indptr.data_ptr(), ntok, B, L,
                                  layer_idx, N, P, fmt, _stream(kv_data))
        else:
            st = lib.arcq_kv_append(*tables, k.data_ptr(), v.data_ptr(), k_param.data_ptr(), v_param.data_ptr(), B, L, layer_idx, N, P, fmt,
                                    _stream(kv_data))
    _lib.check(st, f"kvcache.{who}")


def _decode(who, i4, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    dtype = _dtype_of(f"kvcache.{who}", q)
    _need(q, dtype, "q", 3)
    _need(o, dtype, "o", 3)
    L, N, P, B, layer_idx = _cache(who, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx, i4, dtype)
    if q.shape != o.shape or q.shape[0] != B or q.shape[2] != HEAD_DIM:
        raise RuntimeError(f"kvcache.{who}: o and q must be [{B}, Nq, {HEAD_DIM}], got {tuple(o.shape)} / {tuple(q.shape)}")
    Nq = q.shape[1]
    _heads(f"kvcache.{who}", Nq, N)
    _same_device(f"kvcache.{who}", q, o, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset)
    lib, nnz = _lib.lib(), kv_indices.numel()
    ws_bytes = int(lib.arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P))
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device) if ws_bytes else None
    with _on(q.device):
        st = lib.arcq_kv_batch_decode(o.data_ptr(), q.data_ptr(), kv_data.data_ptr(), kv_param.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr(),
                                      last_page_offset.data_ptr(), B, Nq, L, layer_idx, N, P, nnz, _lib.KV_INT4 if i4 else _lib.KV_16BIT, _DTYPES[dtype],
                                      None if ws is None else ws.data_ptr(), ws_bytes, _stream(q))
    _lib.check(st, f"kvcache.{who}")
    return o


# ---- the reference's six (model/kv_cache.py:45-110: same positional order, same keyword names)
def init_kv_i4(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer_idx):
    """Prefill write into an int4 cache: k, v uint8 [tokens, N, 64], k_param, v_param float16 [tokens, N, 2]; tokens
    seqlen_indptr[b] .. seqlen_indptr[b+1] become the last positions of sequence b."""
    _write("init_kv_i4", True, False, True, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer_idx)


def append_kv_i4(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, layer_idx):
    """Decode write into an int4 cache: one token per sequence (k, v uint8 [B, N, 64]) at position seq_len - 1."""
    _write("append_kv_i4", True, False, False, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, None, layer_idx)


def batch_decode_i4(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """o[b, h] = softmax(q[b, h] . K / sqrt(128)) V over sequence b's positions of an int4 cache; o, q float16 or bfloat16 [B, Nq, 128]."""
    return _decode("batch_decode_i4", True, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx)


def init_kv_f16(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer_idx):
    """init_kv_i4 over a 16-bit cache [pages, L, 2, N, P, 128]; the parameters are stored and never applied."""
    _write("init_kv_f16", False, False, True, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, seqlen_indptr, layer_idx)


def append_kv_f16(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, layer_idx):
    """append_kv_i4 over a 16-bit cache."""
    _write("append_kv_f16", False, False, False, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, k_param, v_param, None, layer_idx)


def batch_decode_f16(o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx):
    """batch_decode_i4 over a 16-bit cache of q's dtype."""
    return _decode("batch_decode_f16", False, o, q, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, layer_idx)


# ---- extensions: the quantiser in front of the write, one launch
def append_kv_quantize_i4(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, layer_idx):
    """``asym_quantize_and_pack_i4`` of k and v (float16 or bfloat16 [B, N, 128]) + ``append_kv_i4`` in one launch; byte for byte what
    the torch formula gives on a CPU tensor of that dtype with the parameters converted ``.to(float16)``."""
    _write("append_kv_quantize_i4", True, True, False, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, None, None, None, layer_idx)


def init_kv_quantize_i4(kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, seqlen_indptr, layer_idx):
    """The same in front of ``init_kv_i4``: k, v float16 or bfloat16 [tokens, N, 128]."""
    _write("init_kv_quantize_i4", True, True, True, kv_data, kv_param, kv_indptr, kv_indices, last_page_offset, k, v, None, None, seqlen_indptr, layer_idx)


class PagedKVCacheI4:
    """The pages of an int4 cache and the tables of a batch whose sequences have one common length (what
    MultiLayerPagedKVCache4Bit.get_cache_specs_for_flash_infer builds on every call): sequence b owns pages b, b + batch, b + 2 * batch, ...
    The tables of every length 1 .. max_seq_len are built here, once, so ``tables`` allocates nothing and may be called while a graph is
    being captured."""

    def __init__(self, batch_size: int, page_size: int, max_seq_len: int, device, n_layers: int, num_heads: int, head_dim: int = HEAD_DIM):
        if head_dim != HEAD_DIM:
            raise RuntimeError(f"kvcache.PagedKVCacheI4: head dimension {HEAD_DIM} only, got {head_dim}")
        if batch_size < 1 or page_size < 1 or max_seq_len < 1 or n_layers < 1 or num_heads < 1:
            raise RuntimeError("kvcache.PagedKVCacheI4: batch_size, page_size, max_seq_len, n_layers and num_heads must be positive")
        self.batch_size, self.page_size, self.max_seq_len, self.device = batch_size, page_size, max_seq_len, torch.device(device)
        per_seq, bs = self.page_cnt_from_length(max_seq_len), batch_size
        self.pages = torch.zeros((per_seq * bs, n_layers, 2, num_heads, page_size, head_dim // 2), dtype=torch.uint8, device=device)
        self.scales = torch.zeros((per_seq * bs, n_layers, 2, num_heads, page_size, 2), dtype=torch.float16, device=device)
        cnt = torch.arange(1, per_seq + 1, dtype=torch.int32)
        # row c - 1: the tables of sequences of c pages; row t - 1 of _last: last_page_offset at length t
        self._indptr = (cnt.unsqueeze(1) * torch.arange(bs + 1, dtype=torch.int32).unsqueeze(0)).to(device)
        own = torch.arange(per_seq, dtype=torch.int32).unsqueeze(0) * bs + torch.arange(bs, dtype=torch.int32).unsqueeze(1)      # [bs, per_seq]
        self._indices = [own[:, :c].reshape(-1).to(device) for c in range(1, per_seq + 1)]
        length = torch.arange(1, max_seq_len + 1, dtype=torch.int32)
        self._last = (length - (length - 1) // page_size * page_size).unsqueeze(1).expand(-1, bs).contiguous().to(device)
        self._qo = {}         # n_new -> qo_indptr of prefill_tables

    def page_cnt_from_length(self, length: int) -> int:
        return (length + self.page_size - 1) // self.page_size

    def tables(self, length: int) -> dict:
        """The keyword arguments every function of this module shares, for sequences of ``length`` positions each (the positions a
        write is about to fill included)."""
        if not 1 <= length <= self.max_seq_len:
            raise RuntimeError(f"kvcache.PagedKVCacheI4: length {length} is outside 1 .. {self.max_seq_len}")
        c = self.page_cnt_from_length(length)
        return {"kv_data": self.pages, "kv_param": self.scales, "kv_indptr": self._indptr[c - 1], "kv_indices": self._indices[c - 1],
                "last_page_offset": self._last[length - 1]}

    def prefill_tables(self, length: int, n_new: int) -> dict:
        """``tables(length)`` plus ``qo_indptr`` for ``n_new`` query tokens per sequence, the last ``n_new`` of its ``length`` positions
        (also the ``seqlen_indptr`` of the ``init_kv_*`` call that writes them).  Built once per distinct ``n_new``: nothing is allocated
        when one comes back."""
        if not 1 <= n_new <= length:
            raise RuntimeError(f"kvcache.PagedKVCacheI4: {n_new} new tokens do not fit a sequence of {length} positions")
        out = self.tables(length)
        qo = self._qo.get(n_new)
        if qo is None:
            qo = self._qo[n_new] = (torch.arange(self.batch_size + 1, dtype=torch.int32) * n_new).to(self.device)
        out["qo_indptr"] = qo
        return out
