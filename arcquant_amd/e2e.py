"""Synthetic-weight decode / prefill harness for the ARC-NVFP4 hot path.

Reproduces the CALLER side of the reference's latency benchmark -- benchmarks/modeling_arc.py (decoder layer
structure :279-310, MLP :109-111, RMSNorm+quantise :211-228, QLinearLayer :19-56) and
benchmarks/benchmark_e2e_arc.py (MODEL_CFGS :26-77, protocol :84-115) -- on top of ``arcquant_amd.agemm``:

    per layer:  rmsnorm_quantize_x -> q/k/v GEMMs -> attention -> reorder_quantize_x -> o GEMM -> +residual
                rmsnorm_quantize_x -> gate/up GEMMs -> silu*mul -> reorder_quantize_x -> down GEMM -> +residual

Differences from the reference files (which cannot run here: they need the `flashinfer` package and
transformers-4.44 internals): attention is torch SDPA over a dense bf16 KV cache instead of flashinfer paged KV;
weights are random-init and quantised once with ``agemm.reorder_quantize_w`` (the reference uses all-zero codes);
``select_num`` is 64 for every linear (the calibration artefact is not in the repo); the decode step is captured
in a HIP graph, so host launch overhead does not pace the GPU (every arcquant_amd launch is stream-ordered and
allocation-free apart from torch's caching allocator).

``quant_type="MXFP4"`` runs the same layer structure on the block-scaled fp4 MFMA (``DecoderModel._forward_mx``): weights quantised with
``agemm.mx_reorder_quantize_w`` (no per-tensor scale, alpha = 1), activations with the one-launch operators of ``arcquant_amd.mx``.

``kv_cache="int4"`` (``--kv-cache int4``) swaps the dense bf16 cache for the reference's int4 paged cache served by ``arcquant_amd.kvcache``
(``DecoderModel._attention_int4``); the default is the dense cache.  ``kv_paged_prefill=True`` (``--kv-paged-prefill``) on top of it makes
every multi-token call, at any position, attend over the pages with ``kvcache.batch_prefill_i4`` instead of SDPA over its own k / v.

``rope=True`` (``--rope``, ``--rope-theta``) rotates q and k to their positions before the cache write and attention, on every call path
(``arcquant_amd.kvrope``, DESIGN.md 11 "RoPE"); the default is the RoPE-free layer every published figure was measured on.
"""
from __future__ import annotations

import dataclasses
import time

import torch
import torch.nn.functional as F

from . import agemm, kvcache, kvstep, mx


@dataclasses.dataclass
class ModelConfig:
    name: str
    num_layers: int
    num_heads: int
    hidden_size: int
    intermediate_size: int
    vocab_size: int = 32000          # LlamaConfig default used by benchmarks/modeling_arc.py:431
    select_num: int = 64
    eps: float = 1e-6
    attention_bias: bool = False     # benchmarks/benchmark_e2e_arc.py:21-22, 27-77: q/k/v/o (modeling_arc.py:19-56)
    mlp_bias: bool = False           # gate/up/down


# benchmarks/benchmark_e2e_arc.py:26-77
MODEL_CFGS = {
    "qwen2.5-7b": ModelConfig("qwen2.5-7b", 28, 28, 3584, 18944, attention_bias=True, mlp_bias=True),
    "llama-2-7b": ModelConfig("llama-2-7b", 32, 32, 4096, 11008),
    "llama-3.1-8b": ModelConfig("llama-3.1-8b", 32, 32, 4096, 14336),
    "qwen2.5-14b": ModelConfig("qwen2.5-14b", 48, 40, 5120, 13824, attention_bias=True, mlp_bias=True),
    "qwen2.5-32b": ModelConfig("qwen2.5-32b", 64, 40, 5120, 27648, attention_bias=True, mlp_bias=True),
}


class QLinear:
    """Quantised weight of one linear (random init), model/qLinearLayer.py:30-62 without the nn.Module shell.
    ``out_f`` may be the concatenation of several projections that share their input (q|k|v, gate|up): they are
    then quantised as ONE tensor (one per-tensor scale) and computed by one GEMM launch."""

    def __init__(self, in_f, out_f, select_num, device, gen, bias=False, quant_type="NVFP4"):
        w = (torch.randn(out_f, in_f, generator=gen, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16)
        # modeling_arc.py:37-40: QLinearLayer(bias=config.attention_bias | mlp_bias); added after the GEMM (`y = y + self.bias`)
        self.bias = (torch.randn(out_f, generator=gen, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16) if bias else None
        self.idx = torch.arange(in_f, dtype=torch.int16, device=device)
        self.in_f, self.out_f, self.KE = in_f, out_f, select_num
        self.RW = self.RSF = self.MRW = self.MRSF = None
        self.quant_type = quant_type
        if quant_type == "MXFP4":            # codes [out_f, Kp/2] + E8M0 bytes [out_f, Kp/32]; no per-tensor scale: alpha = 1
            self.W, self.SFW = agemm.mx_reorder_quantize_w(w, self.idx, select_num)
            self.scale, self.scale_f = torch.ones(1, dtype=torch.float32, device=device), 1.0
            return
        scale = torch.max(w).float() / (448.0 * 6.0)
        self.W, self.SFW = agemm.reorder_quantize_w((w / scale).contiguous(), self.idx, select_num)
        self.scale = scale.reshape(1)
        self.scale_f = float(scale)          # one sync at load time; lets alpha = scale_f * (device activation scale)

    def repack(self, release_reference=False):
        """Second copy of the weight in MFMA-operand-order tiles for the decode path (agemm.repack_w).  release_reference: keep
        ONLY that copy (W / SFW dropped; every M then runs through agemm.matmul_rw)."""
        self.RW, self.RSF = agemm.repack_w(self.W, self.SFW)
        if release_reference:
            self.W = self.SFW = None

    def mx_repack(self, release_reference=False):
        """Second copy of an MXFP4 weight in MFMA operand order for calls of at most agemm.MX_REPACKED_MAX_M tokens (agemm.mx_repack_w).
        release_reference: keep ONLY that copy (W / SFW dropped; every M then runs through agemm.mx_matmul_rw)."""
        self.MRW, self.MRSF = agemm.mx_repack_w(self.W, self.SFW)
        if release_reference:
            self.W = self.SFW = None

    def matmul(self, A, SFA, scale, ops=agemm, **kw):
        """GEMM against this weight (+ its bias, in the epilogue): the repacked kernel for decode-sized token counts where available.
        ``ops``: the module whose ``matmul_repacked`` / ``matmul_rw`` is called (the ctypes mirror or the extension module)."""
        kw.setdefault("bias", self.bias)
        if self.quant_type == "MXFP4" and self.W is None:     # repacked only: one copy for every M
            return agemm.mx_matmul_rw(A, self.MRW, SFA, self.MRSF, scale, self.out_f, **kw)
        if self.MRW is not None and A.shape[0] <= agemm.MX_REPACKED_MAX_M:
            return agemm.mx_matmul_repacked(A, self.MRW, SFA, self.MRSF, scale, self.out_f, **kw)
        if self.quant_type == "MXFP4":
            return agemm.mx_matmul(A, self.W, SFA, self.SFW, scale, **kw)
        if self.W is None:           # repacked only: one copy for every M (the repacked kernels where matmul_repacked would run)
            return ops.matmul_rw(A, self.RW, SFA, self.RSF, scale, self.out_f, **kw)
        if self.RW is not None and agemm.repacked_supported(A.shape[0], self.out_f, self.in_f + self.KE):
            return ops.matmul_repacked(A, self.RW, SFA, self.RSF, scale, self.out_f, **kw)
        return agemm.matmul(A, self.W, SFA, self.SFW, scale, **kw)

    def bytes(self):
        if self.quant_type == "MXFP4":   # Kp/2 code bytes + Kp/32 scale bytes per row (a decode step reads one copy, whichever it is)
            if self.W is None:           # repacked only: the MRW / MRSF it holds (MRSF padded to whole rounds)
                return self.MRW.numel() + self.MRSF.numel()
            return self.W.numel() + self.SFW.numel()
        if self.W is None:           # repacked only: the padded RW / RSF it holds
            return self.RW.numel() + self.RSF.numel()
        return self.W.numel() + self.out_f * (self.in_f + self.KE) // 16


# What mx_fused_linears=True / --mx-fused-linears without a list selects: the linears whose fused call beat the two-launch chain by
# more than twice the larger band at M = 4 on MI355X (tools/mx_linear_bench.py, profiles/mxfp4_linear_fused.json).  None
# did (o tied, q|k|v and gate|up lost 2.2 and 1.7 us), so the selection is empty: fusing a linear takes naming it.
MX_FUSED_LINEARS_DEFAULT = ""


class DecoderModel:
    """fused=False: the reference's call structure (model/qLlamaLayer.py: separate q/k/v and gate/up GEMMs, torch
    abs/max/div before each activation quantise, torch residual adds).  fused=True: q|k|v and gate|up as one GEMM each,
    `reorder_quantize_x_dynamic` (1-2 launches instead of 5), SiLU*up in the gate|up GEMM epilogue (`matmul_silu_mul`),
    residual add in the GEMM epilogue, one strided K|V cache append.
    quant_type="MXFP4": the same two call structures on the MXFP4 operators (_forward_mx)."""

    # MXFP4, fused=True: how a decode step (T <= 64 tokens, where mx_small_kernel runs) forms the down projection's input:
    # "epilogue" = mx.matmul_silu_mul + mx_reorder_quantize_x (as prefill), "quantiser" = mx_matmul + mx.silu_mul_quantize_x(GU_PAIRS).
    # Chosen by measurement (tools/mx_fused_bench.py): at the Qwen2.5-7B gate|up shape the epilogue route takes 34.3 us
    # against 35.5 at M = 4 and 134 against 140 at M = 64.
    mx_decode_route = "epilogue"
    kv_page_size = 16         # kv_cache="int4": positions per page (the reference's benchmark default)

    def __init__(self, cfg: ModelConfig, batch: int, max_len: int, device, fused: bool = False, attention: str = "current",
                 repacked_only: bool = False, quant_type: str = "NVFP4", mx_quantised_epilogue: bool = False, kv_cache: str = "bf16",
                 kv_fused_step: bool = False, kv_paged_prefill: bool = False, mx_repacked_decode: bool = False,
                 mx_repacked_only: bool = False, mx_fused_linears=None, rope: bool = False, rope_theta: float = 1e6, rope_tables=None):
        """attention="current": what benchmarks/modeling_arc.py:169-198 times -- K/V are appended to the cache and each
        sequence attends (causally) over its CURRENT tokens only; attention="cache": attend over the whole KV cache.
        repacked_only (fused=True only): every linear keeps ONLY its repacked weight -- the reference-layout copy is released after
        the repack and every GEMM the repacked kernels do not serve runs through agemm.matmul_rw / matmul_rw_silu_mul.
        mx_quantised_epilogue (quant_type="MXFP4", fused=True only): the gate|up GEMM writes the down projection's quantised input itself
        (mx.matmul_silu_mul_quantize) instead of mx.matmul_silu_mul + mx_reorder_quantize_x, prefill and decode alike; same logits.
        mx_repacked_decode (quant_type="MXFP4", fused=True only, not with mx_quantised_epilogue): every linear additionally keeps its weight
        as agemm.mx_repack_w lays it out; calls of at most agemm.MX_REPACKED_MAX_M tokens run q|k|v, o, gate|up and down through
        agemm.mx_matmul_repacked / mx.matmul_silu_mul_repacked.  Same logits, bit for bit.
        mx_repacked_only (quant_type="MXFP4", fused=True only, not with mx_repacked_decode): every linear keeps ONLY its repacked weight and
        every GEMM, at any token count, runs over it (agemm.mx_matmul_rw, mx.matmul_silu_mul_rw; with mx_quantised_epilogue the gate|up call is
        mx.matmul_silu_mul_quantize_rw).  Same logits, bit for bit, at half of mx_repacked_decode's weight memory.
        mx_fused_linears (needs mx_repacked_decode or mx_repacked_only): a subset of "qkv,o,gateup" (a string, or True for
        MX_FUSED_LINEARS_DEFAULT) -- in a call of at most 16 tokens for which mx.linear_fused_supported holds, those linears run their
        activation quantiser as the prologue of the repacked GEMM (mx.linear_rmsnorm_repacked, mx.linear_quantize_repacked,
        mx.linear_rmsnorm_silu_repacked): one launch instead of two; every other call takes the unfused path.  Same logits, bit for bit.
        down is never fused (an intermediate_size-wide prologue in every workgroup), and gate|up not together with mx_quantised_epilogue
        (that kernel has no prologue), nor with mx_decode_route = "quantiser" (forward raises: the fused gate|up is the "epilogue" route's).
        kv_cache="int4" (attention="cache", head dimension 128): the reference's int4 paged cache (arcquant_amd.kvcache)
        instead of the dense bf16 one -- a prefill writes its k / v through init_kv_quantize_i4, a decode step appends with
        append_kv_quantize_i4 and attends with batch_decode_i4.  "bf16" (default) is the dense cache.
        kv_paged_prefill (kv_cache="int4" only): a multi-token call at ANY position writes its k / v into the pages and attends over them
        with batch_prefill_i4 (chunked prefill, a second turn); off, a multi-token call starts at position 0 and attends with SDPA.
        rope (head dimension 128): q and k are rotated to their positions (rotate-half, the Hugging Face tables of ``rope_theta`` for
        ``max_len`` positions, or the caller's ``rope_tables`` = (cos, sin), bfloat16 [>= max_len, 128]) before the cache write and
        attention: kvrope.rope_qk_ in place on the dense paths, SDPA prefill and the one-launch step; kvrope.rope_append_kv_quantize_i4 /
        rope_init_kv_quantize_i4 in place of the quantising writers on the int4 chain and the paged prefill."""
        if kv_cache not in ("bf16", "int4"):
            raise ValueError(f"DecoderModel: kv_cache must be 'bf16' or 'int4', got {kv_cache!r}")
        if kv_cache == "int4" and (attention != "cache" or cfg.hidden_size // cfg.num_heads != kvcache.HEAD_DIM):
            raise ValueError("DecoderModel: kv_cache='int4' needs attention='cache' and a head dimension of 128")
        if kv_fused_step and kv_cache != "int4":
            raise ValueError("DecoderModel: kv_fused_step=True needs kv_cache='int4' (the one-launch decode step is the int4 paged cache's)")
        if kv_paged_prefill and kv_cache != "int4":
            raise ValueError("DecoderModel: kv_paged_prefill=True needs kv_cache='int4' (the prefill attention is the int4 paged cache's)")
        if rope_tables is not None and not rope:
            raise ValueError("DecoderModel: rope_tables needs rope=True")
        if rope and cfg.hidden_size // cfg.num_heads != kvcache.HEAD_DIM:
            raise ValueError("DecoderModel: rope=True needs a head dimension of 128")
        if rope_tables is not None:
            if not (isinstance(rope_tables, (tuple, list)) and len(rope_tables) == 2):
                raise ValueError("DecoderModel: rope_tables must be a (cos, sin) pair")
            for t in rope_tables:
                if getattr(t, "dtype", None) is not torch.bfloat16 or t.dim() != 2 or t.shape[1] != kvcache.HEAD_DIM or t.shape[0] < max_len:
                    raise ValueError(f"DecoderModel: rope_tables must be two bfloat16 tensors [>= {max_len}, {kvcache.HEAD_DIM}], got "
                                     f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if repacked_only and not fused:
            raise ValueError("DecoderModel: repacked_only=True needs fused=True (the unfused model is the reference's call structure)")
        if quant_type not in ("NVFP4", "MXFP4"):
            raise NotImplementedError(f"quant_type={quant_type!r} is not built (NVFP4 and MXFP4 are)")
        if quant_type == "MXFP4" and repacked_only:
            raise ValueError("DecoderModel: repacked_only applies to the NVFP4 weight layout only, not to quant_type='MXFP4'")
        if mx_quantised_epilogue and (quant_type != "MXFP4" or not fused):
            raise ValueError("DecoderModel: mx_quantised_epilogue needs quant_type='MXFP4' and fused=True (NVFP4's per-tensor scale needs the "
                             "whole activation first; the unfused model is the reference's call structure)")
        if mx_repacked_decode and (quant_type != "MXFP4" or not fused or mx_quantised_epilogue):
            raise ValueError("DecoderModel: mx_repacked_decode needs quant_type='MXFP4' and fused=True, and has no form of the quantising "
                             "epilogue (mx_quantised_epilogue)")
        if mx_repacked_only and (quant_type != "MXFP4" or not fused or mx_repacked_decode):
            raise ValueError("DecoderModel: mx_repacked_only needs quant_type='MXFP4' and fused=True, and replaces mx_repacked_decode (it keeps "
                             "the repacked copy alone; NVFP4 has repacked_only)")
        if mx_fused_linears is True:
            mx_fused_linears = MX_FUSED_LINEARS_DEFAULT
        mx_fuse = frozenset(filter(None, (mx_fused_linears or "").split(",")))
        if mx_fuse - {"qkv", "o", "gateup"}:
            raise ValueError(f"DecoderModel: mx_fused_linears must be a subset of 'qkv,o,gateup' (down is not fused), got {mx_fused_linears!r}")
        if mx_fuse and not (mx_repacked_decode or mx_repacked_only):
            raise ValueError("DecoderModel: mx_fused_linears needs mx_repacked_decode or mx_repacked_only (the fused linears run over the "
                             "repacked weight)")
        if "gateup" in mx_fuse and mx_quantised_epilogue:
            raise ValueError("DecoderModel: mx_fused_linears='gateup' has no form of the quantising epilogue (mx_quantised_epilogue): that "
                             "kernel has no prologue")
        self.mx_fuse = mx_fuse
        self.quant_type = quant_type
        self.mx_quantised_epilogue = mx_quantised_epilogue
        self.mx_repacked_only = mx_repacked_only
        self.mx_repacked_decode = mx_repacked_decode
        self.cfg, self.device, self.batch, self.max_len, self.fused = cfg, device, batch, max_len, fused
        self.repacked_only = repacked_only
        self.attention = attention
        self.kv_cache, self.kv_fused_step, self.kv_paged_prefill = kv_cache, kv_fused_step, kv_paged_prefill
        self.kv_trace = None      # a list: _attention_int4 appends (layer, pos, q, k, v, out) of every decode step to it (tests)
        # the down projection's quantiser as its GEMM's prologue: every CU then quantises the whole M x intermediate activation
        # itself, which only pays while that is small (measured: Qwen2.5-7B, 4 x 18944: slower than the separate launch)
        self.fused_down = batch * cfg.intermediate_size <= 4 * 8192
        # which decode linears run their activation quantiser as the GEMM's prologue (one launch instead of two); A-B'ed on
        # MI355X with tools/e2e_fuse_ab.py, the default is the fastest combination measured there
        import os
        self.fuse = set(filter(None, os.environ.get("ARCQ_E2E_FUSE", "qkv,o,gateup").split(",")))
        # the decode step's attention over the bf16 cache (harness glue, outside SURVEY 8): "stream" = the harness's own streaming
        # kernel (include/arcq_harness.h; it also appends k / v), "sdpa" / "bmm" = torch (45-48 us per layer at 1040 tokens)
        self.decode_attention = os.environ.get("ARCQ_E2E_DECODE_ATTENTION", "stream" if fused else "sdpa")
        self._attn_ws = None
        # the decode step's hot calls go through the extension module when it is built (same C-ABI entry points, ~half the host time per
        # call: an eager step is host-paced through ctypes); ARCQ_E2E_EXT=0 keeps the ctypes mirror
        self.fast = agemm
        if fused and os.environ.get("ARCQ_E2E_EXT", "1") == "1":
            try:
                from . import _build_ext
                self.fast = _build_ext.import_agemm_extension()
            except ImportError:
                pass
        g = torch.Generator(device=device).manual_seed(0)
        h, it, ke = cfg.hidden_size, cfg.intermediate_size, cfg.select_num
        ab, mb, qt = cfg.attention_bias, cfg.mlp_bias, quant_type
        self.layers = []
        for _ in range(cfg.num_layers):
            self.layers.append(dict(
                ln1=torch.ones(h, dtype=torch.bfloat16, device=device), ln2=torch.ones(h, dtype=torch.bfloat16, device=device),
                **(dict(qkv=QLinear(h, 3 * h, ke, device, g, ab, qt), gateup=QLinear(h, 2 * it, ke, device, g, mb, qt)) if fused else
                   dict(q=QLinear(h, h, ke, device, g, ab, qt), k=QLinear(h, h, ke, device, g, ab, qt), v=QLinear(h, h, ke, device, g, ab, qt),
                        gate=QLinear(h, it, ke, device, g, mb, qt), up=QLinear(h, it, ke, device, g, mb, qt))),
                o=QLinear(h, h, ke, device, g, ab, qt), down=QLinear(it, h, ke, device, g, mb, qt),
                kv=torch.zeros(2, batch, cfg.num_heads, max_len if kv_cache == "bf16" else 0, h // cfg.num_heads, dtype=torch.bfloat16, device=device)))
            self.layers[-1]["kc"], self.layers[-1]["vc"] = self.layers[-1]["kv"][0], self.layers[-1]["kv"][1]
        if fused and quant_type == "NVFP4":
            for L in self.layers:
                for name in ("qkv", "o", "gateup", "down"):
                    L[name].repack(release_reference=repacked_only)
        if mx_repacked_decode or mx_repacked_only:
            for L in self.layers:
                for name in ("qkv", "o", "gateup", "down"):
                    L[name].mx_repack(release_reference=mx_repacked_only)
        self.idx_h = torch.arange(h, dtype=torch.int16, device=device)
        self.idx_i = torch.arange(it, dtype=torch.int16, device=device)
        self.inv_idx_i = torch.argsort(self.idx_i.long()).to(torch.int16)     # act_scatter_index of the gate|up epilogue
        agemm._check_scatter_index(self.inv_idx_i, it)                      # (the extension binding does not re-check the permutation)
        self.act_scatter = os.environ.get("ARCQ_E2E_ACT_SCATTER", "1") == "1"
        self.norm = torch.ones(h, dtype=torch.bfloat16, device=device)
        self.lm_head = (torch.randn(cfg.vocab_size, h, generator=g, device=device) * 0.02).to(torch.bfloat16)
        self.embed = (torch.randn(cfg.vocab_size, h, generator=g, device=device) * 0.02).to(torch.bfloat16)
        self.one = torch.ones(1, dtype=torch.float32, device=device)
        # every layer's pages in one paged cache, with the page tables of every length built here -- before any graph capture
        self.kvc = kvcache.PagedKVCacheI4(batch, self.kv_page_size, max_len, device, cfg.num_layers, cfg.num_heads) if kv_cache == "int4" else None
        self.kv_step_state = kvstep.DecodeStepState(batch, cfg.num_heads, cfg.num_heads, device) if kv_fused_step else None
        # RoPE: the tables and the positions of every call are built here, once -- nothing is allocated per step (graph capture)
        self.rope = bool(rope)
        self.rope_cos = self.rope_sin = self.rope_pos = None
        if self.rope:
            if rope_tables is None:
                rope_tables = kvcache.rope_tables(max_len, rope_theta, torch.bfloat16)
            self.rope_cos, self.rope_sin = (t.to(device).contiguous() for t in rope_tables)
            self.rope_pos = torch.arange(max_len, dtype=torch.int32, device=device)

    def weight_bytes(self):
        per_layer = sum(v.bytes() for v in self.layers[0].values() if isinstance(v, QLinear))
        return per_layer * self.cfg.num_layers + self.lm_head.numel() * 2

    def _rope_(self, q, k, pos, q_len):
        """rope=True: q (and k, unless None) -- [tokens, heads * 128] rows, views included -- rotated in place to positions pos .. pos + q_len - 1
        (token i of a call is position pos + i % q_len); returns the [tokens, heads, 128] views."""
        hd = kvcache.HEAD_DIM
        q3 = q.unflatten(-1, (-1, hd))
        k3 = None if k is None else k.unflatten(-1, (-1, hd))
        kvcache.rope_qk_(q3, k3, self.rope_pos[pos:pos + q_len], self.rope_cos, self.rope_sin)
        return q3, k3

    @staticmethod
    def _quant_x(x, idx, ke):
        # model/qLlamaLayer.py:73-77 semantics, with the per-tensor scale kept on the device
        scale = agemm.absmax_scale(x)
        qx, sfx = agemm.reorder_quantize_x((x / scale).contiguous(), idx, ke)
        return qx, sfx, scale

    def forward(self, tokens: torch.Tensor, pos: int):
        """tokens [batch, q_len] int64; appends K/V at [pos, pos+q_len) and attends over [0, pos+q_len)."""
        if self.quant_type == "MXFP4":
            return self._forward_mx(tokens, pos)
        cfg = self.cfg
        bsz, q_len = tokens.shape
        nh, hd = cfg.num_heads, cfg.hidden_size // cfg.num_heads
        hcur = F.embedding(tokens, self.embed).reshape(bsz * q_len, cfg.hidden_size)      # one gather launch (advanced indexing: ~10)
        h, it, ke = cfg.hidden_size, cfg.intermediate_size, cfg.select_num
        T = bsz * q_len
        for li, L in enumerate(self.layers):
            # ---- attention block: RMSNorm + quantise, q|k|v projection
            if self.fused:
                Q = L["qkv"]
                if "qkv" in self.fuse and Q.RW is not None and agemm.fused_supported(agemm.SRC_RMSNORM, T, Q.out_f, h, ke):
                    # decode: ONE launch (the quantiser is the GEMM's prologue; bias in its epilogue)
                    qkv = self.fast.rmsnorm_matmul_repacked(hcur, L["ln1"], cfg.eps, self.idx_h, ke, Q.RW, Q.RSF, Q.scale, Q.out_f, bias=Q.bias)
                else:
                    A, SFA = agemm.rmsnorm_quantize_x(hcur, L["ln1"], cfg.eps, self.idx_h, ke)
                    qkv = Q.matmul(A, SFA, Q.scale)
                q, k, v = qkv[:, :h], qkv[:, h:2 * h], qkv[:, 2 * h:]
            else:
                A, SFA = agemm.rmsnorm_quantize_x(hcur, L["ln1"], cfg.eps, self.idx_h, ke)
                q, k, v = (self._ref_linear(L[n], A, SFA, L[n].scale) for n in ("q", "k", "v"))
            if self.kv_cache == "int4":
                att = self._attention_int4(li, q, k, v, qkv if self.fused else None, pos, bsz, q_len)
            elif self.fused and q_len == 1 and hd == 128 and self.decode_attention == "stream":
                att = self._attn_decode_stream(qkv, L, pos)          # K|V append + attention over [0, pos]: the harness's own kernel
            else:
                att = self._attention_torch(L, q, k, v, qkv if self.fused else None, pos, bsz, q_len)
            # ---- output projection (+ residual)
            if self.fused:
                O_ = L["o"]
                if "o" in self.fuse and O_.RW is not None and agemm.fused_supported(agemm.SRC_DYNAMIC, T, O_.out_f, h, ke):
                    hcur, _ = self.fast.dynamic_matmul_repacked(att, self.idx_h, ke, O_.RW, O_.RSF, O_.scale_f, O_.out_f, bias=O_.bias, residual=hcur)
                else:
                    qa, sfa, sa = agemm.reorder_quantize_x_dynamic(att, self.idx_h, ke)
                    hcur = O_.matmul(qa, sfa, sa, scale_host=O_.scale_f, residual=hcur)
            else:
                qa, sfa, sa = self._quant_x(att, self.idx_h, ke)
                hcur = hcur + self._ref_linear(L["o"], qa, sfa, sa * L["o"].scale)
            # ---- MLP
            if self.fused:
                Gt, D_ = L["gateup"], L["down"]         # one weight with gate and up rows interleaved (g0, u0, g1, u1, ...)
                slots = None
                if "gateup" in self.fuse and Gt.RW is not None and agemm.fused_supported(agemm.SRC_RMSNORM, T, Gt.out_f, h, ke):
                    # decode: RMSNorm + quantise + gate|up GEMM + bias + SiLU*up + abs-max words in ONE launch
                    # "scatter": its epilogue stores the activation in the DOWN projection's channel order, the quantiser below then
                    # reads contiguous groups (reorder_index=None) instead of staging + gathering each row
                    scatter = self.inv_idx_i if self.act_scatter and not (("down" in self.fuse or self.fused_down)) else None
                    act, slots = self.fast.rmsnorm_matmul_repacked_silu(hcur, L["ln2"], cfg.eps, self.idx_h, ke, Gt.RW, Gt.RSF, Gt.scale, Gt.out_f, bias=Gt.bias,
                                                                        act_scatter_index=scatter)
                    if scatter is not None:
                        qa, sfa, sa = self.fast.reorder_quantize_x_dynamic(act, None, ke, absmax_slots=slots)
                        hcur = D_.matmul(qa, sfa, sa, scale_host=D_.scale_f, residual=hcur, ops=self.fast)
                        continue
                else:
                    A, SFA = agemm.rmsnorm_quantize_x(hcur, L["ln2"], cfg.eps, self.idx_h, ke)
                    if T > 16:      # prefill: act_fn(gate) * up and its abs-max in the tile GEMM's epilogue
                        if Gt.W is None:
                            act, slots = agemm.matmul_rw_silu_mul(A, Gt.RW, SFA, Gt.RSF, Gt.scale, Gt.out_f, bias=Gt.bias)
                        else:
                            act, slots = agemm.matmul_silu_mul(A, Gt.W, SFA, Gt.SFW, Gt.scale, bias=Gt.bias)
                    elif Gt.RW is not None and Gt.bias is None and agemm.repacked_supported(T, Gt.out_f, h + ke):
                        # r1 path: the repacked GEMM leaves max |silu(g) * u| per row block, the quantiser applies SiLU*up itself
                        gu, slots = agemm.matmul_repacked_silu_absmax(A, Gt.RW, SFA, Gt.RSF, Gt.scale, Gt.out_f)
                        act = None
                    else:
                        gu = Gt.matmul(A, SFA, Gt.scale)
                        act = (F.silu(gu[:, 0::2]) * gu[:, 1::2]).contiguous()
                if act is None:
                    qa, sfa, sa = agemm.silu_mul_quantize_x_dynamic(gu, self.idx_i, ke, layout=agemm.GU_PAIRS, absmax_slots=slots)
                    hcur = D_.matmul(qa, sfa, sa, scale_host=D_.scale_f, residual=hcur)
                elif ("down" in self.fuse or self.fused_down) and D_.RW is not None and agemm.fused_supported(agemm.SRC_DYNAMIC, T, D_.out_f, it, ke):
                    hcur, _ = agemm.dynamic_matmul_repacked(act, self.idx_i, ke, D_.RW, D_.RSF, D_.scale_f, D_.out_f, absmax_slots=slots,
                                                            bias=D_.bias, residual=hcur)
                else:
                    qa, sfa, sa = agemm.reorder_quantize_x_dynamic(act, self.idx_i, ke, absmax_slots=slots)
                    hcur = D_.matmul(qa, sfa, sa, scale_host=D_.scale_f, residual=hcur)
            else:
                A, SFA = agemm.rmsnorm_quantize_x(hcur, L["ln2"], cfg.eps, self.idx_h, ke)
                gate = self._ref_linear(L["gate"], A, SFA, L["gate"].scale)
                up = self._ref_linear(L["up"], A, SFA, L["up"].scale)
                act = F.silu(gate) * up
                qa, sfa, sa = self._quant_x(act, self.idx_i, ke)
                hcur = hcur + self._ref_linear(L["down"], qa, sfa, sa * L["down"].scale)
        return self._logits(hcur, bsz, q_len)

    def _logits(self, hcur, bsz, q_len):
        """Final norm of each sequence's last token and the lm_head product."""
        cfg = self.cfg
        last = hcur.view(bsz, q_len, -1)[:, -1]                 # [bsz, hidden], row stride q_len * hidden
        if self.fused:
            # the final norm as one launch (include/arcq_harness.h; torch's F.rms_norm is ~15 small kernels on this stack)
            from . import _lib
            hn = torch.empty((bsz, cfg.hidden_size), dtype=torch.bfloat16, device=hcur.device)
            with torch.cuda.device(hcur.device):
                st = _lib.lib().arcq_harness_rmsnorm(last.data_ptr(), last.stride(0), self.norm.data_ptr(), hn.data_ptr(), bsz, cfg.hidden_size,
                                                     float(cfg.eps), torch.cuda.current_stream(hcur.device).cuda_stream)
            _lib.check(st, "harness rmsnorm")
        else:
            hn = F.rms_norm(last, (cfg.hidden_size,), self.norm, cfg.eps)
        return hn @ self.lm_head.t()

    def _forward_mx(self, tokens: torch.Tensor, pos: int):
        """forward() for quant_type="MXFP4".  Per layer, fused=True:
            mx.rmsnorm_quantize_x -> q|k|v mx_matmul (+bias) -> attention -> mx_reorder_quantize_x -> o mx_matmul (+bias, +residual)
            mx.rmsnorm_quantize_x -> mx.matmul_silu_mul (+bias) -> mx_reorder_quantize_x -> down mx_matmul (+bias, +residual)
        (a decode step may take mx_matmul + mx.silu_mul_quantize_x instead of the middle two: mx_decode_route; with
        mx_quantised_epilogue the middle two are mx.matmul_silu_mul_quantize at every T -- idx_i is the identity; with mx_repacked_decode a
        call of at most agemm.MX_REPACKED_MAX_M tokens takes every GEMM over the repacked weight, with mx_repacked_only every call does:
        the *_rw forms); fused=False, the
        reference's call structure (model/qQwenLayer.py): separate q, k, v and gate, up GEMMs, bias / SiLU*up / residual as torch ops.
        Every activation quantiser is one launch either way -- MXFP4 has no per-tensor scale to find first."""
        if "gateup" in self.mx_fuse and self.mx_decode_route != "epilogue":
            raise ValueError("DecoderModel: mx_fused_linears='gateup' is the fused form of the 'epilogue' decode route (SiLU*up in the GEMM); "
                             f"mx_decode_route={self.mx_decode_route!r} has none")
        cfg = self.cfg
        bsz, q_len = tokens.shape
        h, ke, hd = cfg.hidden_size, cfg.select_num, cfg.hidden_size // cfg.num_heads
        T = bsz * q_len
        hcur = F.embedding(tokens, self.embed).reshape(T, h)
        fz = self.mx_fuse if T <= mx.MX_LINEAR_MAX_M else ()

        def fuses(name, kind, lin):                         # this call's `name` linear runs its quantiser as the GEMM's prologue
            return name in fz and mx.linear_fused_supported(kind, T, lin.out_f, h, ke)

        for li, L in enumerate(self.layers):
            if self.fused:
                Q = L["qkv"]
                if fuses("qkv", mx.SRC_RMSNORM, Q):
                    qkv = mx.linear_rmsnorm_repacked(hcur, L["ln1"], cfg.eps, self.idx_h, ke, Q.MRW, Q.MRSF, 1.0, Q.out_f, bias=Q.bias)
                else:
                    A, SFA = mx.rmsnorm_quantize_x(hcur, L["ln1"], cfg.eps, self.idx_h, ke)
                    qkv = Q.matmul(A, SFA, 1.0)
                if self.kv_cache == "int4":
                    att = self._attention_int4(li, qkv[:, :h], qkv[:, h:2 * h], qkv[:, 2 * h:], qkv, pos, bsz, q_len)
                elif q_len == 1 and hd == 128 and self.decode_attention == "stream":
                    att = self._attn_decode_stream(qkv, L, pos)
                else:
                    att = self._attention_torch(L, qkv[:, :h], qkv[:, h:2 * h], qkv[:, 2 * h:], qkv, pos, bsz, q_len)
                O_ = L["o"]
                if fuses("o", mx.SRC_PLAIN, O_):
                    hcur = mx.linear_quantize_repacked(att, self.idx_h, ke, O_.MRW, O_.MRSF, 1.0, O_.out_f, bias=O_.bias, residual=hcur)
                else:
                    qa, sfa = agemm.mx_reorder_quantize_x(att, self.idx_h, ke)
                    hcur = O_.matmul(qa, sfa, 1.0, residual=hcur)
                Gt = L["gateup"]                            # one weight with gate and up rows interleaved (g0, u0, g1, u1, ...)
                fuse_gu = fuses("gateup", mx.SRC_RMSNORM, Gt)
                if not fuse_gu:
                    A, SFA = mx.rmsnorm_quantize_x(hcur, L["ln2"], cfg.eps, self.idx_h, ke)
                if fuse_gu:
                    act = mx.linear_rmsnorm_silu_repacked(hcur, L["ln2"], cfg.eps, self.idx_h, ke, Gt.MRW, Gt.MRSF, 1.0, Gt.out_f, bias=Gt.bias)
                    qa, sfa = agemm.mx_reorder_quantize_x(act, self.idx_i, ke)
                elif self.mx_quantised_epilogue and Gt.W is None:
                    qa, sfa = mx.matmul_silu_mul_quantize_rw(A, Gt.MRW, SFA, Gt.MRSF, 1.0, Gt.out_f, ke, bias=Gt.bias)
                elif self.mx_quantised_epilogue:
                    qa, sfa = mx.matmul_silu_mul_quantize(A, Gt.W, SFA, Gt.SFW, 1.0, ke, bias=Gt.bias)
                elif T <= 64 and self.mx_decode_route == "quantiser":
                    qa, sfa = mx.silu_mul_quantize_x(Gt.matmul(A, SFA, 1.0), self.idx_i, ke, layout=agemm.GU_PAIRS)
                elif Gt.W is None:
                    act = mx.matmul_silu_mul_rw(A, Gt.MRW, SFA, Gt.MRSF, 1.0, Gt.out_f, bias=Gt.bias)
                    qa, sfa = agemm.mx_reorder_quantize_x(act, self.idx_i, ke)
                elif Gt.MRW is not None and T <= agemm.MX_REPACKED_MAX_M:
                    act = mx.matmul_silu_mul_repacked(A, Gt.MRW, SFA, Gt.MRSF, 1.0, Gt.out_f, bias=Gt.bias)
                    qa, sfa = agemm.mx_reorder_quantize_x(act, self.idx_i, ke)
                else:
                    act = mx.matmul_silu_mul(A, Gt.W, SFA, Gt.SFW, 1.0, bias=Gt.bias)
                    qa, sfa = agemm.mx_reorder_quantize_x(act, self.idx_i, ke)
                hcur = L["down"].matmul(qa, sfa, 1.0, residual=hcur)
            else:
                A, SFA = mx.rmsnorm_quantize_x(hcur, L["ln1"], cfg.eps, self.idx_h, ke)
                q, k, v = (self._ref_linear_mx(L[n], A, SFA) for n in ("q", "k", "v"))
                att = (self._attention_int4(li, q, k, v, None, pos, bsz, q_len) if self.kv_cache == "int4" else
                       self._attention_torch(L, q, k, v, None, pos, bsz, q_len))
                qa, sfa = agemm.mx_reorder_quantize_x(att, self.idx_h, ke)
                hcur = hcur + self._ref_linear_mx(L["o"], qa, sfa)
                A, SFA = mx.rmsnorm_quantize_x(hcur, L["ln2"], cfg.eps, self.idx_h, ke)
                act = F.silu(self._ref_linear_mx(L["gate"], A, SFA)) * self._ref_linear_mx(L["up"], A, SFA)
                qa, sfa = agemm.mx_reorder_quantize_x(act, self.idx_i, ke)
                hcur = hcur + self._ref_linear_mx(L["down"], qa, sfa)
        return self._logits(hcur, bsz, q_len)

    @staticmethod
    def _ref_linear_mx(lin, A, SFA):
        """QLinearLayer.forward's MXFP4 branch the way the reference writes it: GEMM, then `y = y + self.bias` as its own op."""
        y = agemm.mx_matmul(A, lin.W, SFA, lin.SFW, 1.0)
        return y if lin.bias is None else y + lin.bias

    def _attention_torch(self, L, q, k, v, qkv, pos, bsz, q_len):
        """KV append + attention with torch ops (prefill always; decode when the streaming kernel is switched off)."""
        cfg = self.cfg
        nh, hd, h = cfg.num_heads, cfg.hidden_size // cfg.num_heads, cfg.hidden_size
        if self.rope:           # in place on the projection output (or its q, k views): the cache write below stores the rotated k
            self._rope_(q, k, pos, q_len)
        q = q.reshape(bsz, q_len, nh, hd).transpose(1, 2)
        if qkv is not None:     # k|v are adjacent columns of the fused projection: ONE strided copy appends both to the cache
            L["kv"][:, :, :, pos:pos + q_len] = qkv[:, h:].reshape(bsz, q_len, 2, nh, hd).permute(2, 0, 3, 1, 4)
        else:
            L["kc"][:, :, pos:pos + q_len] = k.reshape(bsz, q_len, nh, hd).transpose(1, 2)
            L["vc"][:, :, pos:pos + q_len] = v.reshape(bsz, q_len, nh, hd).transpose(1, 2)
        if self.attention == "cache" and q_len == 1 and self.decode_attention == "bmm":
            kc, vc = L["kc"][:, :, :pos + 1], L["vc"][:, :, :pos + 1]
            sc = torch.matmul(q, kc.transpose(2, 3)) * (hd ** -0.5)
            att = torch.matmul(torch.softmax(sc.float(), dim=-1).to(q.dtype), vc)
        elif self.attention == "cache":
            att = F.scaled_dot_product_attention(q, L["kc"][:, :, :pos + q_len], L["vc"][:, :, :pos + q_len],
                                                 is_causal=(q_len > 1 and pos == 0))
        else:                   # benchmarks/modeling_arc.py:169-198: each sequence attends over the tokens of THIS call only
            att = F.scaled_dot_product_attention(q, k.reshape(bsz, q_len, nh, hd).transpose(1, 2),
                                                 v.reshape(bsz, q_len, nh, hd).transpose(1, 2), is_causal=q_len > 1)
        return att.transpose(1, 2).reshape(bsz * q_len, h)

    def _attention_int4(self, li, q, k, v, qkv, pos, bsz, q_len):
        """kv_cache="int4": layer ``li``'s K / V go into the int4 paged cache and a decode step attends over it (arcquant_amd.kvcache).
        Prefill (q_len > 1, from position 0 only): init_kv_quantize_i4 writes the pages; the prompt's own causal attention is torch
        SDPA over this call's k / v, as with the dense cache.  With kv_paged_prefill a multi-token call at any position writes the pages
        of positions pos .. pos + q_len - 1 and attends over positions 0 .. with batch_prefill_i4: no SDPA, and what the prompt attends
        over is what the decode steps will read (the call is also traced, with ``n_new`` = q_len).  Decode:
        append_kv_quantize_i4, then batch_decode_i4 over positions [0, pos], on the q, k and v slices of the projection output (one
        transposing copy makes the three contiguous); with kv_fused_step the three become ONE kvstep.decode_step_i4 launch on views of
        the projection output, bit for bit the same.  Harness glue around the operators, like the dense cache's kernel.
        rope=True: the two quantising writers become kvrope's (rotation, contiguous q and write in one launch, on views: no transposing
        copy), the SDPA prefill and the one-launch step rotate q and k in place first; the trace records the rotated q and k."""
        cfg = self.cfg
        nh, hd, h = cfg.num_heads, cfg.hidden_size // cfg.num_heads, cfg.hidden_size
        if q_len > 1 and self.kv_paged_prefill:
            tables = self.kvc.prefill_tables(pos + q_len, q_len)
            qo_indptr = tables.pop("qo_indptr")
            if self.rope:       # rotation, the contiguous q and the quantising write in one launch, on the views of the projection output
                qs, kk, vv = (t.unflatten(-1, (nh, hd)) for t in (q, k, v))
                qq = torch.empty((bsz * q_len, nh, hd), dtype=q.dtype, device=q.device)
                kvcache.rope_init_kv_quantize_i4(qq, qs, kk, vv, self.rope_cos, self.rope_sin, **tables, seqlen_indptr=qo_indptr, layer_idx=li)
                if self.kv_trace is not None:       # (the rotated k exists only as codes: the trace rotates a copy)
                    kk = self._rope_(kk.clone(memory_format=torch.contiguous_format).view(bsz * q_len, h), None, pos, q_len)[0]
            else:
                qq, kk, vv = (t.reshape(bsz * q_len, nh, hd).contiguous() for t in (q, k, v))
                kvcache.init_kv_quantize_i4(**tables, k=kk, v=vv, seqlen_indptr=qo_indptr, layer_idx=li)
            out = torch.empty_like(qq)
            kvcache.batch_prefill_i4(out, qq, qo_indptr, **tables, layer_idx=li)
            if self.kv_trace is not None:
                self.kv_trace.append(dict(layer=li, pos=pos, n_new=q_len, q=qq.clone(), k=kk.clone(), v=vv.clone(), out=out.clone()))
            return out.view(bsz * q_len, h)
        if q_len > 1:
            if pos != 0:
                raise ValueError("DecoderModel(kv_cache='int4'): a multi-token call must start at position 0 (no prefill attention over the int4 pages)")
            if self.rope:       # SDPA below needs the rotated k in 16 bit
                self._rope_(q, k, pos, q_len)
            kk, vv = k.reshape(bsz * q_len, nh, hd).contiguous(), v.reshape(bsz * q_len, nh, hd).contiguous()
            seqlens = torch.arange(bsz + 1, dtype=torch.int32, device=kk.device) * q_len
            kvcache.init_kv_quantize_i4(**self.kvc.tables(q_len), k=kk, v=vv, seqlen_indptr=seqlens, layer_idx=li)
            att = F.scaled_dot_product_attention(q.reshape(bsz, q_len, nh, hd).transpose(1, 2), kk.view(bsz, q_len, nh, hd).transpose(1, 2),
                                                 vv.view(bsz, q_len, nh, hd).transpose(1, 2), is_causal=True)
            return att.transpose(1, 2).reshape(bsz * q_len, h)
        tables = self.kvc.tables(pos + 1)
        if self.kv_fused_step:      # one launch on views of the projection output (kvstep, DESIGN.md 11 "Decode step")
            qq, kk, vv = (qkv.view(bsz, 3 * nh, hd).split(nh, dim=1) if qkv is not None else (t.reshape(bsz, nh, hd) for t in (q, k, v)))
            if self.rope:
                kvcache.rope_qk_(qq, kk, self.rope_pos[pos:pos + 1], self.rope_cos, self.rope_sin)
            out = torch.empty((bsz, nh, hd), dtype=qq.dtype, device=qq.device)
            kvstep.decode_step_i4(out, qq, kk, vv, **tables, layer_idx=li, state=self.kv_step_state)
        elif self.rope:             # the rotation, the contiguous q and the quantising append in one launch: no transposing copy
            qs, kk, vv = (qkv.view(bsz, 3 * nh, hd).split(nh, dim=1) if qkv is not None else (t.reshape(bsz, nh, hd) for t in (q, k, v)))
            qq = torch.empty((bsz, nh, hd), dtype=qs.dtype, device=qs.device)
            kvcache.rope_append_kv_quantize_i4(qq, qs, kk, vv, self.rope_cos, self.rope_sin, **tables, layer_idx=li)
            out = torch.empty_like(qq)
            kvcache.batch_decode_i4(out, qq, **tables, layer_idx=li)
            if self.kv_trace is not None:           # (the rotated k exists only as codes: the trace rotates a copy)
                kk = self._rope_(kk.clone(memory_format=torch.contiguous_format).view(bsz, h), None, pos, 1)[0]
        else:
            if qkv is not None:
                qq, kk, vv = qkv.view(bsz, 3, nh, hd).transpose(0, 1).contiguous().unbind(0)
            else:
                qq, kk, vv = (t.reshape(bsz, nh, hd).contiguous() for t in (q, k, v))
            kvcache.append_kv_quantize_i4(**tables, k=kk, v=vv, layer_idx=li)
            out = torch.empty_like(qq)
            kvcache.batch_decode_i4(out, qq, **tables, layer_idx=li)
        if self.kv_trace is not None:
            self.kv_trace.append(dict(layer=li, pos=pos, q=qq.clone(), k=kk.clone(), v=vv.clone(), out=out.clone()))
        return out.view(bsz, h)

    def _attn_decode_stream(self, qkv, L, pos):
        """One decode step of attention over the dense bf16 cache with the harness kernel (include/arcq_harness.h): appends this
        token's k / v at `pos` and attends over [0, pos] (attention="cache") or over the current token only ("current", what
        benchmarks/modeling_arc.py:169-198 times); fp32 math, bf16 out [batch, hidden]."""
        from . import _lib
        lib = _lib.lib()
        bsz, nh = qkv.shape[0], self.cfg.num_heads
        if self.rope:           # one launch more: q and k rotated in place in the projection output, the kernel below as it is
            h = self.cfg.hidden_size
            self._rope_(qkv[:, :h], qkv[:, h:2 * h], pos, 1)
        tmax = L["kc"].shape[2]
        if self._attn_ws is None:
            self._attn_ws = torch.empty(int(lib.arcq_harness_attn_workspace_bytes(bsz, nh, tmax)) // 4, dtype=torch.float32, device=qkv.device)
        out = torch.empty((bsz, self.cfg.hidden_size), dtype=torch.bfloat16, device=qkv.device)
        with torch.cuda.device(qkv.device):
            st = lib.arcq_harness_attn_decode_window(qkv.data_ptr(), L["kc"].data_ptr(), L["vc"].data_ptr(), out.data_ptr(), self._attn_ws.data_ptr(),
                                                     bsz, nh, tmax, int(pos), 0 if self.attention == "cache" else int(pos),
                                                     torch.cuda.current_stream(qkv.device).cuda_stream)
        _lib.check(st, "harness attn_decode")
        return out

    @staticmethod
    def _ref_linear(lin, A, SFA, scale):
        """The reference's QLinearLayer.forward (benchmarks/modeling_arc.py:47-56): GEMM, then `y = y + self.bias` as its own op."""
        y = agemm.matmul(A, lin.W, SFA, lin.SFW, scale)
        return y if lin.bias is None else y + lin.bias


def bench_decode(name="qwen2.5-7b", batch=4, prefill=1024, steps=16, device="cuda:0", repeats=3, layers=None, fused=False,
                 attention="current", repacked_only=False, quant_type="NVFP4", mx_quantised_epilogue=False, kv_cache="bf16",
                 kv_fused_step=False, kv_paged_prefill=False, rope=False, rope_theta=1e6, mx_repacked_decode=False,
                 mx_repacked_only=False, mx_fused_linears=None):
    """Decode tok/s with the decode step replayed from a HIP graph (attention window fixed at prefill+steps).  repacked_only: one
    weight copy per linear (DecoderModel); the result then also reports it and the device memory the built model holds.  mx_repacked_only:
    the same for quant_type="MXFP4"."""
    cfg = dataclasses.replace(MODEL_CFGS[name])
    if layers:
        cfg.num_layers = layers
    device = torch.device(device)
    with torch.no_grad():
        mem0 = torch.cuda.memory_allocated(device)
        model = DecoderModel(cfg, batch, prefill + steps + 1, device, fused=fused, attention=attention, repacked_only=repacked_only,
                             quant_type=quant_type, mx_quantised_epilogue=mx_quantised_epilogue, kv_cache=kv_cache, kv_fused_step=kv_fused_step,
                             kv_paged_prefill=kv_paged_prefill, rope=rope, rope_theta=rope_theta, mx_repacked_decode=mx_repacked_decode,
                             mx_repacked_only=mx_repacked_only, mx_fused_linears=mx_fused_linears)
        model_bytes = torch.cuda.memory_allocated(device) - mem0
        tok = torch.randint(100, 200, (batch, prefill), device=device)
        t0 = time.perf_counter()
        model.forward(tok, 0)
        torch.cuda.synchronize()
        t_prefill_first = time.perf_counter() - t0
        t0 = time.perf_counter()
        model.forward(tok, 0)
        torch.cuda.synchronize()
        t_prefill = time.perf_counter() - t0
        nxt = torch.randint(100, 200, (batch, 1), device=device)
        pos = prefill + steps          # fixed attention window: the graph is shape-static
        for _ in range(2):
            model.forward(nxt, pos)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            model.forward(nxt, pos)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                out = model.forward(nxt, pos)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        best = None
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / steps
            best = ms if best is None else min(best, ms)
        # eager (no graph) for comparison: host-paced
        t0 = time.perf_counter()
        for _ in range(4):
            model.forward(nxt, pos)
        torch.cuda.synchronize()
        eager_ms = (time.perf_counter() - t0) / 4 * 1e3
        wb = model.weight_bytes()
        kv = 2 * cfg.num_layers * batch * cfg.hidden_size * pos * 2 if attention == "cache" else 0
        if kv_cache == "int4":      # 64 bytes of codes + a 4-byte (scale, zero) pair per head and position
            kv = 2 * cfg.num_layers * batch * cfg.num_heads * pos * 68
        assert out.shape == (batch, cfg.vocab_size)
    res = {"model": name, "fused": fused, "attention": attention, "layers": cfg.num_layers, "batch": batch, "prefill": prefill, "attn_window": pos,
           "decode_ms_per_step_graph": round(best, 4), "decode_tok_per_s": round(batch / best * 1e3, 1),
           "decode_ms_per_step_eager": round(eager_ms, 3), "prefill_ms": round(t_prefill * 1e3, 2),
           "prefill_tok_per_s": round(batch * prefill / t_prefill, 0), "prefill_first_call_ms": round(t_prefill_first * 1e3, 1),
           "weight_bytes": wb, "kv_bytes_read_per_step": kv,
           "hbm_floor_ms_at_8TBps": round((wb + kv) / 8e12 * 1e3, 4)}
    if repacked_only:
        res.update(repacked_only=True, model_resident_bytes=int(model_bytes))
    if quant_type != "NVFP4":
        res["quant_type"] = quant_type
    if mx_quantised_epilogue:
        res["mx_quantised_epilogue"] = True
    if mx_repacked_decode:
        res["mx_repacked_decode"] = True
    if mx_repacked_only:
        res.update(mx_repacked_only=True, model_resident_bytes=int(model_bytes))
    if model.mx_fuse:
        res["mx_fused_linears"] = ",".join(sorted(model.mx_fuse))
    if kv_cache != "bf16":
        res["kv_cache"] = kv_cache
    if kv_fused_step:
        res["kv_fused_step"] = True
    if kv_paged_prefill:
        res["kv_paged_prefill"] = True
    if rope:
        res["rope"] = True
    return res


def bench_protocol(name="qwen2.5-7b", batch=4, prefill=1024, decode_steps=128, device="cuda:0", repeats=10, warmup=2, steps=4,
                   fused=True, attention="cache", graph=True, layers=None, repacked_only=False, quant_type="NVFP4", mx_quantised_epilogue=False,
                   kv_cache="bf16", kv_fused_step=False, kv_paged_prefill=False, rope=False, rope_theta=1e6, mx_repacked_decode=False,
                   mx_repacked_only=False, mx_fused_linears=None):
    """The reference's latency protocol (benchmarks/benchmark_e2e_arc.py): three timed modules -- prefill (:133-140), decode
    for `decode_steps` steps over a GROWING cache (:142-155) and prefill + decode (:157-166) -- each run `warmup` times
    untimed and `steps` times timed between two device synchronisations, repeated `repeats` times (:81-115); reported as
    mean +- 1.96 sigma of the per-call milliseconds plus the peak device memory (:208-216).  graph=True replays the whole
    multi-step decode (every step at its own cache length) from ONE HIP graph; graph=False issues it eagerly like the
    reference does."""
    cfg = dataclasses.replace(MODEL_CFGS[name])
    if layers:
        cfg.num_layers = layers
    device = torch.device(device)

    def module_benchmark(fn):
        times, peaks = [], []
        for _ in range(repeats):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated())
            times.append((time.perf_counter() - t0) * 1e3 / steps)
        t = torch.tensor(times, dtype=torch.float64)
        return round(float(t.mean()), 3), round(1.96 * float(t.std(unbiased=False)), 3), max(peaks)

    with torch.no_grad():
        mem0 = torch.cuda.memory_allocated(device)
        model = DecoderModel(cfg, batch, prefill + decode_steps, device, fused=fused, attention=attention, repacked_only=repacked_only,
                             quant_type=quant_type, mx_quantised_epilogue=mx_quantised_epilogue, kv_cache=kv_cache, kv_fused_step=kv_fused_step,
                             kv_paged_prefill=kv_paged_prefill, rope=rope, rope_theta=rope_theta, mx_repacked_decode=mx_repacked_decode,
                             mx_repacked_only=mx_repacked_only, mx_fused_linears=mx_fused_linears)
        model_bytes = torch.cuda.memory_allocated(device) - mem0
        tok = torch.randint(100, 200, (batch, prefill), device=device)
        nxt = torch.full((batch, 1), 100, device=device, dtype=torch.int64)          # benchmark_e2e_arc.py:150

        def run_prefill():
            model.forward(tok, 0)

        def decode_eager():
            for i in range(decode_steps):
                model.forward(nxt, prefill + i)

        run_prefill()
        decode_eager()
        torch.cuda.synchronize()
        run_decode = decode_eager
        if graph:
            g = torch.cuda.CUDAGraph()
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    decode_eager()
            torch.cuda.synchronize()
            run_decode = g.replay

        def run_e2e():
            run_prefill()
            run_decode()

        p_ms, p_ci, p_mem = module_benchmark(run_prefill)
        d_ms, d_ci, d_mem = module_benchmark(run_decode)
        e_ms, e_ci, e_mem = module_benchmark(run_e2e)
    res = {"protocol": "benchmark_e2e_arc.py: %d warm-up + %d timed calls x %d repeats, mean +- 1.96 sigma" % (warmup, steps, repeats),
           "model": name, "layers": cfg.num_layers, "batch": batch, "prefill": prefill, "decode_steps": decode_steps, "fused": fused,
           "attention": attention, "decode_from_hip_graph": bool(graph),
           "prefill_ms": [p_ms, p_ci], "decode_ms": [d_ms, d_ci], "e2e_ms": [e_ms, e_ci],
           "prefill_tok_per_s": round(batch * prefill / p_ms * 1e3, 0), "decode_tok_per_s": round(batch * decode_steps / d_ms * 1e3, 1),
           "peak_memory_gb": round(max(p_mem, d_mem, e_mem) / 2 ** 30, 3)}
    if repacked_only:
        res["repacked_only"] = True
    if quant_type != "NVFP4":
        res["quant_type"] = quant_type
    if mx_quantised_epilogue:
        res["mx_quantised_epilogue"] = True
    if mx_repacked_decode:
        res["mx_repacked_decode"] = True
    if mx_repacked_only:
        res.update(mx_repacked_only=True, model_resident_bytes=int(model_bytes))
    if model.mx_fuse:
        res["mx_fused_linears"] = ",".join(sorted(model.mx_fuse))
    if kv_cache != "bf16":
        res["kv_cache"] = kv_cache
    if kv_fused_step:
        res["kv_fused_step"] = True
    if kv_paged_prefill:
        res["kv_paged_prefill"] = True
    if rope:
        res["rope"] = True
    return res


# ---- BASELINE config[4]: one Llama-3-70B-shape decoder layer per rank of a tensor-parallel group -------------------------------------
LLAMA3_70B = dict(hidden=8192, heads=64, kv_heads=8, head_dim=128, inter=28672, layers=80)


def build_tp_layer(rank, world, device, batch, max_len, cfg=None, KE=64, seed=0, ops=None, repack=True, group=None):
    """This rank's shard of ONE decoder layer with random weights (tp.TPDecoderLayer; the shards are drawn directly, seed + rank,
    each with its own per-tensor weight scale), identity reorder indices, ``select_num`` = KE for every linear (per shard for the
    row-parallel ones: hand-off B)."""
    from . import tp
    cfg = dict(LLAMA3_70B if cfg is None else cfg)
    h, hd = cfg["hidden"], cfg["head_dim"]
    hq, hk, it = cfg["heads"] // world * hd, cfg["kv_heads"] // world * hd, cfg["inter"] // world
    g = torch.Generator(device=device).manual_seed(seed * 1000 + rank)

    def rnd(n, k):
        return (torch.randn(n, k, generator=g, device=device, dtype=torch.float32) * 0.02).to(torch.bfloat16)

    shards = dict(wqkv=rnd(hq + 2 * hk, h), wo=rnd(h, hq), wgu=rnd(2 * it, h), wd=rnd(h, it))
    ones = torch.ones(h, dtype=torch.bfloat16, device=device)
    idx_h = torch.arange(h, dtype=torch.int16, device=device)
    idx_o = torch.arange(hq, dtype=torch.int16, device=device)
    idx_d = torch.arange(it, dtype=torch.int16, device=device)
    return tp.TPDecoderLayer.build(shards, ones, ones.clone(), idx_h, idx_o, idx_d, KE, KE, KE, rank, world, cfg["heads"], cfg["kv_heads"], hd,
                                   batch, max_len, eps=1e-5, group=group, ops=ops, repack=repack)


def bench_tp_layer(rank, world, device, batch=4, pos=1040, steps=50, warmup=10, cfg=None):
    """Decode step of ONE tensor-parallel decoder layer (Llama-3-70B shape by default): per-layer time with its four collectives
    (2 x all-reduce(MAX) of 4 B, 2 x all-reduce(SUM) of the fp32 [batch, hidden] partial), the same step with the collectives
    skipped (what the rank's four launches + attention cost alone), max over ranks.  Launches are issued eagerly."""
    import torch.distributed as dist
    from . import tp
    cfg = dict(LLAMA3_70B if cfg is None else cfg)
    with torch.no_grad():
        layer = build_tp_layer(rank, world, device, batch, pos + 8, cfg)
        h = (torch.randn(batch, cfg["hidden"], device=device, generator=torch.Generator(device=device).manual_seed(7)) * 0.5).to(torch.bfloat16)

        def timed(fn):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t = torch.tensor([e0.elapsed_time(e1) * 1e3 / steps], dtype=torch.float64, device=device)
            if world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        with_coll = timed(lambda: layer.forward(h, pos))
        out = layer.forward(h, pos)
        # the same launches without the exchange: the linears think they are alone (world = 1); results are then partial sums
        for m in (layer.o, layer.down):
            m.world = 1
        grp, layer.group = layer.group, None
        saved = tp.handoff_local_scale
        tp.handoff_local_scale = lambda y_local=None, group=None, word=None: (tp.absmax_word(y_local) if word is None else word)
        try:
            no_coll = timed(lambda: layer.forward(h, pos))
        finally:
            tp.handoff_local_scale = saved
            layer.group = grp
            for m in (layer.o, layer.down):
                m.world = world
        same = True
        if world > 1:                                          # the replicated hidden state must be bit-identical on every rank
            ref = out.clone()
            dist.broadcast(ref, src=0)
            flag = torch.tensor([int(torch.equal(ref, out))], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            same = bool(flag.item())
    wbytes = sum(m.W.numel() * 9 // 8 for m in (layer.qkv, layer.o, layer.gateup, layer.down))
    return {"model": "llama-3-70b-shape decoder layer", "tp": world, "batch": batch, "attn_window": pos, "launches": "eager",
            "layer_us_with_collectives": round(with_coll, 1), "layer_us_without_collectives": round(no_coll, 1),
            "weight_bytes_per_rank": int(wbytes), "collective_bytes": tp.TPDecoderLayer.collective_bytes_per_layer(batch, cfg["hidden"], world),
            "output_identical_on_all_ranks": same,
            "decode_tok_per_s_80_layers_est": round(batch / (with_coll * cfg["layers"]) * 1e6, 1)}


def _tp_main(argv):
    """python -m arcquant_amd.e2e --tp N [--steps K]: one rank per GPU (self-launched, or under torch.distributed.run).
    Rehearsal on a one-GPU box: ARCQ_BENCH_ONE_DEVICE=1 ARCQ_BENCH_BACKEND=gloo."""
    import json
    import os
    import sys
    from . import launch
    n = int(argv[argv.index("--tp") + 1])
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 50
    if n > 1 and not launch.launched():
        sys.exit(launch.launch_ranks(n, [sys.executable, "-m", "arcquant_amd.e2e"] + list(argv)))
    world, rank, local_rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    one_device = os.environ.get("ARCQ_BENCH_ONE_DEVICE") == "1"
    backend = os.environ.get("ARCQ_BENCH_BACKEND", "nccl")
    dev_index = 0 if one_device else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    cfg = None
    if "--small" in argv:                                      # a quick functional pass (tests): 1/8 of the 70B layer in every dimension
        cfg = dict(hidden=2048, heads=16, kv_heads=2 * max(1, world), head_dim=128, inter=7168 // 8 * 8, layers=80)
    res = bench_tp_layer(rank, world, device, steps=steps, cfg=cfg)
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    import json
    import sys
    if "--tp" in sys.argv:
        _tp_main(sys.argv[1:])
        sys.exit(0)
    argv = sys.argv[1:]
    qt = "NVFP4"
    if "--quant-type" in argv:        # --quant-type {NVFP4,MXFP4}
        i = argv.index("--quant-type")
        qt = argv[i + 1] if i + 1 < len(argv) else ""
        if qt not in ("NVFP4", "MXFP4"):
            sys.exit("--quant-type takes NVFP4 or MXFP4")
        del argv[i:i + 2]
    kvc = "bf16"
    if "--kv-cache" in argv:          # --kv-cache {bf16,int4}: int4 = the reference's paged cache (attention over the whole cache only)
        i = argv.index("--kv-cache")
        kvc = argv[i + 1] if i + 1 < len(argv) else ""
        if kvc not in ("bf16", "int4"):
            sys.exit("--kv-cache takes bf16 or int4")
        del argv[i:i + 2]
    rope_theta = 1e6
    if "--rope-theta" in argv:        # --rope-theta BASE (with --rope)
        i = argv.index("--rope-theta")
        try:
            rope_theta = float(argv[i + 1])
        except (IndexError, ValueError):
            sys.exit("--rope-theta takes a number")
        del argv[i:i + 2]
    rope = "--rope" in argv           # q and k rotated to their positions before the cache write and attention (kvrope)
    args = [a for a in argv if not a.startswith("--")]
    name = args[0] if args else "qwen2.5-7b"
    kfs = "--kv-fused-step" in sys.argv      # --kv-cache int4 only: the decode step's append + attention as one launch (kvstep)
    if kfs and kvc != "int4":
        sys.exit("--kv-fused-step needs --kv-cache int4")
    kpp = "--kv-paged-prefill" in sys.argv   # --kv-cache int4 only: multi-token calls attend over the pages (kvcache.batch_prefill_i4)
    if kpp and kvc != "int4":
        sys.exit("--kv-paged-prefill needs --kv-cache int4")
    ro = "--repacked-only" in sys.argv       # one weight copy per linear (the fused model only)
    qe = "--mx-quantised-epilogue" in sys.argv   # MXFP4, the fused model only: the gate|up GEMM quantises the down projection's input
    if qe and qt != "MXFP4":
        sys.exit("--mx-quantised-epilogue needs --quant-type MXFP4")
    mrd = "--mx-repacked-decode" in sys.argv     # MXFP4, the fused model only: decode GEMMs over the repacked weight (agemm.mx_repack_w)
    if mrd and (qt != "MXFP4" or qe):
        sys.exit("--mx-repacked-decode needs --quant-type MXFP4 and excludes --mx-quantised-epilogue")
    mro = "--mx-repacked-only" in sys.argv       # MXFP4, the fused model only: one weight copy per linear, every GEMM over the repacked weight
    if mro and (qt != "MXFP4" or mrd):
        sys.exit("--mx-repacked-only needs --quant-type MXFP4 and replaces --mx-repacked-decode")
    mfl = None                                   # --mx-fused-linears[=LIST]: LIST a subset of qkv,o,gateup; without one, the linears measured faster
    for arg in sys.argv:
        if arg == "--mx-fused-linears" or arg.startswith("--mx-fused-linears="):
            mfl = arg.partition("=")[2] if "=" in arg else MX_FUSED_LINEARS_DEFAULT
            if set(filter(None, mfl.split(","))) - {"qkv", "o", "gateup"}:
                sys.exit("--mx-fused-linears takes a subset of qkv,o,gateup")
    if mfl and not (mrd or mro):
        sys.exit("--mx-fused-linears needs --mx-repacked-decode or --mx-repacked-only")
    if mfl and qe and "gateup" in mfl.split(","):
        sys.exit("--mx-fused-linears=gateup excludes --mx-quantised-epilogue")
    if "--protocol" in sys.argv:      # the reference's own benchmark protocol (growing cache, mean +- 1.96 sigma)
        for graph in (True, False):
            print(json.dumps(bench_protocol(name, graph=graph, repacked_only=ro, quant_type=qt, mx_quantised_epilogue=qe, kv_cache=kvc,
                                            kv_fused_step=kfs, kv_paged_prefill=kpp, rope=rope, rope_theta=rope_theta, mx_repacked_decode=mrd,
                                            mx_repacked_only=mro, mx_fused_linears=mfl)), flush=True)
            torch.cuda.empty_cache()
    else:
        for fused, att in ((False, "current"), (True, "current"), (True, "cache")):
            if ((ro or qe or mrd or mro or mfl) and not fused) or (kvc == "int4" and att != "cache"):
                continue
            print(json.dumps(bench_decode(name, fused=fused, attention=att, repacked_only=ro, quant_type=qt, mx_quantised_epilogue=qe, kv_cache=kvc,
                                          kv_fused_step=kfs, kv_paged_prefill=kpp, rope=rope, rope_theta=rope_theta, mx_repacked_decode=mrd,
                                          mx_repacked_only=mro, mx_fused_linears=mfl)), flush=True)
            torch.cuda.empty_cache()
