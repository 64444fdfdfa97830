"""MXFP4 decoder-layer operators (include/arcq.h "MXFP4 decoder-layer operators"): the fused RMSNorm and SiLU*up
quantisers and the gate|up GEMM with SiLU*up in its epilogue -- what ``agemm.rmsnorm_quantize_x``, ``silu_mul_quantize_x_dynamic`` and
``matmul_silu_mul`` are to NVFP4.  MXFP4 has no per-tensor scale, so each operator is ONE launch and returns no scale and no abs-max
slots.

The plain MXFP4 quantisers and GEMM stay in ``agemm`` (``mx_reorder_quantize_{x,w}``, ``mx_matmul``).  This module is a ctypes mirror
only: the extension module ``agemm.so`` does not bind these operators.  Validation follows the mirror's order (``agemm._need`` ...):
dtype / rank / contiguity, then the size relations, then the optional tensors, and LAST where everything lives.
"""
from __future__ import annotations

import torch

from . import _lib
from .agemm import GU_HALVES, GU_PAIRS, _alpha, _need, _on, _opt, _out, _same_device, _stream, mx_k_padded


def _outputs(M: int, KQ: int, KE: int, like: torch.Tensor):
    Kp = mx_k_padded(KQ + KE)
    return (torch.empty((M, Kp // 2), dtype=torch.uint8, device=like.device), torch.empty((M, Kp // 32), dtype=torch.uint8, device=like.device))


def rmsnorm_quantize_x(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int):
    """RMSNorm + MXFP4-ARC activation quantiser in one launch -> (QX u8 [M, Kp/2], SFX u8 E8M0 [M, Kp/32]).  The normalised row is
    ``agemm.rmsnorm_quantize_x``'s (bf16(x * w * rstd), the project's fused-kernel formula), quantised as ``mx_reorder_quantize_x``
    quantises a bf16 row.  2048 <= KQ <= 8192."""
    _need(X, torch.bfloat16, "X", 2)
    _need(W, torch.bfloat16, "W", 1)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    M, KQ = X.shape
    KE = int(KE)
    if W.numel() != KQ or reorder_index.numel() != KQ:
        raise RuntimeError(f"mx.rmsnorm_quantize_x: W / reorder_index must have X.shape[1] = {KQ} entries, got {W.numel()} / {reorder_index.numel()}")
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or not (2048 <= KQ <= 8192):
        raise RuntimeError(f"Value error in mx.rmsnorm_quantize_x: KQ={KQ}, KE={KE} is not valid (2048 <= KQ <= 8192, multiples of 64, KE <= KQ)")
    _same_device("mx.rmsnorm_quantize_x", X, W, reorder_index)
    QX, SFX = _outputs(M, KQ, KE, X)
    with _on(X.device):
        st = _lib.lib().arcq_mx_rmsnorm_quantize_x(X.data_ptr(), W.data_ptr(), float(eps), reorder_index.data_ptr(), QX.data_ptr(), SFX.data_ptr(),
                                                   M, KQ, KE, _stream(X))
    _lib.check(st, "mx.rmsnorm_quantize_x")
    return QX, SFX


def silu_mul_quantize_x(GU: torch.Tensor, reorder_index: torch.Tensor, KE: int, layout: int = GU_HALVES):
    """The MLP's ``act_fn(gate) * up`` (SiLU) folded into the MXFP4-ARC quantiser, one launch -> (QX, SFX).  ``GU`` is bf16 [M, 2*KQ]:
    ``layout=GU_HALVES`` (gate | up) or ``GU_PAIRS`` (g0, u0, g1, u1, ...).  Byte for byte what
    ``agemm.mx_reorder_quantize_x(F.silu(gate) * up, reorder_index, KE)`` returns; the product is never materialised."""
    _need(GU, torch.bfloat16, "GU", 2)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    if GU.shape[1] % 2:
        raise RuntimeError("Value error in mx.silu_mul_quantize_x: GU must hold gate and up halves of equal width")
    if layout not in (GU_HALVES, GU_PAIRS):
        raise RuntimeError("Value error in mx.silu_mul_quantize_x: layout must be GU_HALVES or GU_PAIRS")
    M, KQ = GU.shape[0], GU.shape[1] // 2
    KE = int(KE)
    if reorder_index.numel() != KQ:
        raise RuntimeError(f"mx.silu_mul_quantize_x: reorder_index has {reorder_index.numel()} entries, expected {KQ}")
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or KQ > 32767:
        raise RuntimeError(f"Value error in mx.silu_mul_quantize_x: KQ={KQ}, KE={KE} is not valid")
    _same_device("mx.silu_mul_quantize_x", GU, reorder_index)
    QX, SFX = _outputs(M, KQ, KE, GU)
    with _on(GU.device):
        st = _lib.lib().arcq_mx_silu_mul_quantize_x(GU.data_ptr(), reorder_index.data_ptr(), QX.data_ptr(), SFX.data_ptr(), M, KQ, KE, int(layout),
                                                    _stream(GU))
    _lib.check(st, "mx.silu_mul_quantize_x")
    return QX, SFX


def matmul_silu_mul(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale, *, scale_host: float = 1.0, bias=None, out=None):
    """The gate|up GEMM on the block-scaled fp4 MFMA with ``act_fn(gate) * up`` in its epilogue.  ``B`` is the quantised weight whose
    ROWS INTERLEAVE gate and up (g0, u0, g1, u1, ...; ``bias``, bf16 [N], likewise).  Returns ``act`` bf16 [M, N/2], bit for bit
    ``F.silu(y[:, 0::2]) * y[:, 1::2]`` of ``y = agemm.mx_matmul(A, B, SFA, SFB, scale, bias=bias)``; ``y`` is never written.
    ``scale`` / ``scale_host`` as ``mx_matmul``.  N % 16 == 0."""
    for t, name in ((A, "A"), (B, "B"), (SFA, "SFA"), (SFB, "SFB")):
        _need(t, torch.uint8, name, 2)
    M, N, K = A.shape[0], B.shape[0], A.shape[1] * 2
    if B.shape[1] * 2 != K:
        raise RuntimeError(f"mx.matmul_silu_mul: A has K={K}, B has K={B.shape[1] * 2}")
    if K % 128:
        raise RuntimeError(f"mx.matmul_silu_mul: K={K} is not a padded MXFP4 K (a multiple of 128)")
    if N % 16:
        raise RuntimeError(f"mx.matmul_silu_mul: N={N} must be a multiple of 16")
    if tuple(SFA.shape) != (M, K // 32) or tuple(SFB.shape) != (N, K // 32):
        raise RuntimeError("mx.matmul_silu_mul: SFA / SFB must be [rows, K/32]")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, _ = _out(out, M, N // 2, torch.bfloat16, A, "mx.matmul_silu_mul")
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("mx.matmul_silu_mul", A, B, SFA, SFB, alpha_dev, out, bias)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_silu_mul(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), out.data_ptr(), M, N, K, alpha_host,
                                                 alpha_p, bias_p, _stream(A))
    _lib.check(st, "mx.matmul_silu_mul")
    return out
