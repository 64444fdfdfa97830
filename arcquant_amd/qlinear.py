"""Host-side mirror of the reference's quantised-linear operator.

Mirrors, with the same names, argument meaning and tuple protocol:
  * ``NVFP4_reorder_quantize_w``  model/qLinearLayer.py:25-28
  * ``NVFP4_reorder_quantize_x``  model/qLlamaLayer.py:73-77 == model/qQwenLayer.py:72-75
  * ``QLinearLayer``              model/qLinearLayer.py:30-78  (forward takes ``(qx, scale_x, scale, bsz, q_len)``)
  * ``MXFP4_rmsnorm_quantize_x``  RMSNorm + ``MXFP4_reorder_quantize_x`` in one launch (arcquant_amd/mx.py)
  * ``MXFP4_reorder_quantize_{w,x}``  the packed form of the reference's MXFP4 branch (model/quantize.py:219-268 as called by
    the commented-out model/qLinearLayer.py:58 and model/qQwenLayer.py:81-83), on the block-scaled fp4 MFMA

so that the decoder-layer wrappers of the reference (qLlamaLayer.py / qQwenLayer.py) run unchanged on
top of ``arcquant_amd.agemm``.  What differs from the reference, deliberately:
  * no ``torch.cuda.synchronize()`` after every op and no ``.item()`` on the scale: the per-tensor scales
    stay on the device (0-dim fp32 tensors) and everything is ordered on torch's current stream;
  * ``quant_type`` 'NVFP4' and 'MXFP4' are built; 'INT4' (a fake-quant study path of the reference) is not.
    MXFP4 is real packed e2m1 + E8M0 data here, where the reference dequantises it in place (DESIGN.md "MXFP4").
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import agemm, mx

FP8_MAX = 448.0
FP4_MAX = 6.0


def NVFP4_reorder_quantize_w(w: torch.Tensor, reorder_index: torch.Tensor, select_num: int):
    """(qw, scale_w, scale): per-tensor scale = max(w)/2688 -- the SIGNED max, as in the reference."""
    scale = torch.max(w).float() / (FP8_MAX * FP4_MAX)
    qw, scale_w = agemm.reorder_quantize_w((w / scale).contiguous(), reorder_index, select_num)
    return qw, scale_w, scale


def NVFP4_reorder_quantize_x(x: torch.Tensor, reorder_index: torch.Tensor, select_num: int):
    """(qx, scale_x, scale): per-tensor scale = max|x|/2688."""
    scale = torch.max(x.abs()).float() / (FP8_MAX * FP4_MAX)
    qx, scale_x = agemm.reorder_quantize_x((x / scale).contiguous(), reorder_index, select_num)
    return qx, scale_x, scale


def _unit_scale(t: torch.Tensor) -> torch.Tensor:
    # the reference's MXFP4 branch uses scale = 1.0 (model/quantize.py:225-227,251-253): E8M0 covers the bf16 range
    return torch.ones((), dtype=torch.float32, device=t.device)


def MXFP4_reorder_quantize_w(w: torch.Tensor, reorder_index: torch.Tensor, select_num: int):
    """(qw [N, Kp/2], scale_w [N, Kp/32] E8M0, scale = 1): the weight reordered, with copies of its last ``select_num``
    reordered channels (the form of model/qLinearLayer.py:58)."""
    qw, scale_w = agemm.mx_reorder_quantize_w(w.contiguous(), reorder_index, select_num)
    return qw, scale_w, _unit_scale(w)


def MXFP4_reorder_quantize_x(x: torch.Tensor, reorder_index: torch.Tensor, select_num: int):
    """(qx [M, Kp/2], scale_x [M, Kp/32] E8M0, scale = 1): the activation reordered, with the quantised residual of its last
    ``select_num`` reordered channels (model/qQwenLayer.py:81-83)."""
    qx, scale_x = agemm.mx_reorder_quantize_x(x.contiguous(), reorder_index, select_num)
    return qx, scale_x, _unit_scale(x)


def MXFP4_rmsnorm_quantize_x(x: torch.Tensor, norm_weight: torch.Tensor, eps: float, reorder_index: torch.Tensor, select_num: int):
    """(qx, scale_x, scale = 1): RMSNorm fused into ``MXFP4_reorder_quantize_x`` (one launch, ``mx.rmsnorm_quantize_x``); the same tuple
    protocol, so the result feeds ``QLinearLayer.forward`` directly."""
    qx, scale_x = mx.rmsnorm_quantize_x(x.contiguous(), norm_weight, eps, reorder_index, select_num)
    return qx, scale_x, _unit_scale(x)


def reorder_quantize_x(x, reorder_index, select_num, quant_type="NVFP4"):
    """model/qLlamaLayer.py:79-86."""
    if quant_type == "NVFP4":
        return NVFP4_reorder_quantize_x(x, reorder_index, select_num)
    if quant_type == "MXFP4":
        return MXFP4_reorder_quantize_x(x, reorder_index, select_num)
    raise NotImplementedError(f"quant_type={quant_type!r} is not built (NVFP4 and MXFP4 are)")


def find_qlinear_layers(module, name=""):
    """model/qLinearLayer.py:14-23."""
    if type(module) == QLinearLayer:
        return {name: module}
    res = {}
    for child_name, child in module.named_children():
        res.update(find_qlinear_layers(child, name=name + "." + child_name if name != "" else child_name))
    return res


class QLinearLayer(nn.Module):
    """Weight quantised once at construction; forward = ARC-NVFP4 GEMM (+ bias) on pre-quantised activations."""

    def __init__(self, originalLayer: nn.Linear, select_num, reorder_index, out_reorder_index=None, quant_type="NVFP4",
                 repack_for_decode: bool = False, repacked_only: bool = False, mx_repack_for_decode: bool = False,
                 mx_repacked_only: bool = False):
        """``repack_for_decode`` (extension, default off = the reference's behaviour and memory): additionally keep the
        weight in MFMA-operand-order tiles (``agemm.repack_w``) and use ``agemm.matmul_repacked`` for calls of at most 16
        tokens.  ``repacked_only`` (extension): keep ONLY that copy -- ``W`` / ``scale_w`` are registered as None, every call
        runs through ``agemm.matmul_rw`` (the same results as ``repack_for_decode``, but the decode shapes ``matmul`` serves with
        an LDS-transposing kernel: there up to fp32 summation order); ``agemm.unrepack_w(RW, RSF, ...)`` rebuilds the
        reference-layout pair.  ``mx_repack_for_decode`` (extension, quant_type='MXFP4' only): additionally keep the weight as
        ``agemm.mx_repack_w`` lays it out (``MRW`` / ``MRSF``); calls of at most ``agemm.MX_REPACKED_MAX_M`` tokens run through
        ``agemm.mx_matmul_repacked``, longer ones through ``agemm.mx_matmul`` -- the same bits either way.  ``mx_repacked_only``
        (extension, quant_type='MXFP4' only): keep ONLY ``MRW`` / ``MRSF`` -- ``W`` / ``scale_w`` are registered as None and every call, at
        any token count, runs through ``agemm.mx_matmul_rw`` (the same bits again); ``agemm.mx_unrepack_w(MRW, MRSF, out_features, Kp)``
        rebuilds the reference-layout pair."""
        super().__init__()
        if quant_type not in ("NVFP4", "MXFP4"):
            raise NotImplementedError(f"quant_type={quant_type!r} is not built (NVFP4 and MXFP4 are)")
        if quant_type == "MXFP4" and (repack_for_decode or repacked_only):
            raise ValueError("repack_for_decode / repacked_only apply to the NVFP4 weight layout only, not to quant_type='MXFP4'")
        if mx_repack_for_decode and quant_type != "MXFP4":
            raise ValueError("mx_repack_for_decode applies to quant_type='MXFP4' only (NVFP4 has repack_for_decode / repacked_only)")
        if mx_repacked_only and quant_type != "MXFP4":
            raise ValueError("mx_repacked_only applies to quant_type='MXFP4' only (NVFP4 has repacked_only)")
        self.in_features = originalLayer.in_features
        self.out_features = originalLayer.out_features
        if originalLayer.bias is not None:
            self.register_buffer("bias", originalLayer.bias.data)
        else:
            self.bias = None
        self.select_num = int(select_num)
        self.quant_type = quant_type
        dev = originalLayer.weight.device
        if dev.type != "cuda":
            raise RuntimeError("QLinearLayer: the weight must be on the GPU (quantisation runs there)")
        idx = reorder_index.to(device=dev, dtype=torch.int16)
        w = originalLayer.weight.data.to(torch.bfloat16)
        quantize_w = MXFP4_reorder_quantize_w if quant_type == "MXFP4" else NVFP4_reorder_quantize_w
        W, scale_w, scale = quantize_w(w, idx, self.select_num)
        RW, RSF = agemm.repack_w(W, scale_w) if (repack_for_decode or repacked_only) else (None, None)
        MRW, MRSF = agemm.mx_repack_w(W, scale_w) if (mx_repack_for_decode or mx_repacked_only) else (None, None)
        if repacked_only or mx_repacked_only:
            W = scale_w = None
        self.register_buffer("W", W)
        self.register_buffer("scale_w", scale_w)
        self.register_buffer("scale", scale)
        self.register_buffer("RW", RW)
        self.register_buffer("RSF", RSF)
        self.register_buffer("MRW", MRW)
        self.register_buffer("MRSF", MRSF)

    @torch.no_grad()
    def forward(self, x):
        qx, scale_x, scale, bsz, q_len = x
        # `y = matmul(...); y = y + bias` (model/qLinearLayer.py:74-76): the bias add runs in the GEMM epilogue with the same
        # two roundings (the bf16 product, then the bf16 sum), so the result is bit-identical to the two torch steps
        bias = self.bias if self.bias is None or self.bias.dtype == torch.bfloat16 else None
        if self.quant_type == "MXFP4" and self.W is None:         # mx_repacked_only: the one copy serves every token count
            y = agemm.mx_matmul_rw(qx, self.MRW, scale_x, self.MRSF, scale * self.scale, self.out_features, bias=bias)
        elif getattr(self, "MRW", None) is not None and qx.shape[0] <= agemm.MX_REPACKED_MAX_M:
            y = agemm.mx_matmul_repacked(qx, self.MRW, scale_x, self.MRSF, scale * self.scale, self.out_features, bias=bias)
        elif self.quant_type == "MXFP4":
            y = agemm.mx_matmul(qx, self.W, scale_x, self.scale_w, scale * self.scale, bias=bias)
        elif self.W is None:
            y = agemm.matmul_rw(qx, self.RW, scale_x, self.RSF, scale * self.scale, self.out_features, bias=bias)
        elif getattr(self, "RW", None) is not None and agemm.repacked_supported(qx.shape[0], self.out_features, qx.shape[1] * 2):
            y = agemm.matmul_repacked(qx, self.RW, scale_x, self.RSF, scale * self.scale, self.out_features, bias=bias)
        else:
            y = agemm.matmul(qx, self.W, scale_x, self.scale_w, scale * self.scale, bias=bias)
        if self.bias is not None and bias is None:
            y = y + self.bias
        return y.reshape(bsz, q_len, -1)
