"""MXFP6 (quant_type='MXFP6'; include/arcq.h "MXFP6-ARC"): the e3m2 quantisers and the GEMM on the scaled MFMA with e3m2
activations against an e3m2 or an e2m1 weight.  Reached as ``agemm.mx6_reorder_quantize_{x,w}`` and ``agemm.mx6_matmul`` (``agemm``
re-exports them); a ctypes mirror only, the extension module ``agemm.so`` does not bind them.  Validation follows the mirror's order
(``agemm._need`` ...): dtype / rank / contiguity, then the size relations, then the optional tensors, and LAST where everything lives.
"""
from __future__ import annotations

import torch

from . import _lib
from .agemm import _alpha, _need, _on, _opt, _out, _same_device, _stream, mx_k_padded


def _mx6_quantize(fn_name: str, X: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    _need(X, torch.bfloat16, "X" if fn_name.endswith("_x") else "W", 2)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    rows, KQ = X.shape
    KE = int(KE)
    if reorder_index.numel() != KQ:
        raise RuntimeError(f"agemm: reorder_index has {reorder_index.numel()} entries, expected {KQ}")
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or KQ > 32767:
        raise RuntimeError(f"Value error in {fn_name}: KQ={KQ}, KE={KE} is not valid")
    _same_device(fn_name, X, reorder_index)
    Kp = mx_k_padded(KQ + KE)
    Q = torch.empty((rows, 3 * Kp // 4), dtype=torch.uint8, device=X.device)
    SF = torch.empty((rows, Kp // 32), dtype=torch.uint8, device=X.device)
    L = _lib.lib()
    fn = L.arcq_mx6_quantize_x if fn_name.endswith("_x") else L.arcq_mx6_quantize_w
    with _on(X.device):
        st = fn(X.data_ptr(), reorder_index.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, _stream(X))
    _lib.check(st, fn_name)
    return Q, SF


def mx6_reorder_quantize_x(X: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    """MXFP6-ARC activation quantiser -> (QX u8 [M, 3 Kp/4] e3m2, SFX u8 E8M0 [M, Kp/32]); K = KQ + KE, Kp = round_up(K, 128).
    Positions [KQ, K) hold the quantised residual of reordered channels [KQ-KE, KQ)."""
    return _mx6_quantize("mx6_reorder_quantize_x", X, reorder_index, KE)


def mx6_reorder_quantize_w(W: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    """MXFP6-ARC weight quantiser -> (QW [N, 3 Kp/4], SFW [N, Kp/32]); positions [KQ, K) copy reordered channels [KQ-KE, KQ)."""
    return _mx6_quantize("mx6_reorder_quantize_w", W, reorder_index, KE)


_MX6_B_FORMATS = {"e3m2": (_lib.MX_B_E3M2, 3, 4), "e2m1": (_lib.MX_B_E2M1, 1, 2)}     # name -> (ARCQ_MX_B_*, bytes per K element = num / den)


def mx6_matmul(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale=1.0, *, b_format: str = "e3m2", bias=None,
               residual=None, out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """D = scale * deq(A) . deq(B)^T on the block-scaled MFMA with e3m2 activations -> [M, N].  ``b_format`` names the weight's
    element: "e3m2" (B [N, 3 K/4] of ``mx6_reorder_quantize_w``) or "e2m1" (B [N, K/2] of ``mx_reorder_quantize_w`` with the same
    KQ, KE and reorder_index: W4A6).  Everything else is ``mx_matmul``'s."""
    for t, name in ((A, "A"), (B, "B"), (SFA, "SFA"), (SFB, "SFB")):
        _need(t, torch.uint8, name, 2)
    if b_format not in _MX6_B_FORMATS:
        raise RuntimeError(f"agemm.mx6_matmul: b_format must be 'e3m2' or 'e2m1', got {b_format!r}")
    code, num, den = _MX6_B_FORMATS[b_format]
    M, N = A.shape[0], B.shape[0]
    if A.shape[1] % 96:
        raise RuntimeError(f"agemm.mx6_matmul: A has {A.shape[1]} bytes per row, not a padded MXFP6 K (a multiple of 96 bytes = 128 elements)")
    K = A.shape[1] // 3 * 4
    if B.shape[1] * den != K * num:
        raise RuntimeError(f"agemm.mx6_matmul: A has K={K}, B ({b_format}) has {B.shape[1]} bytes per row, expected {K * num // den}")
    if N % 16:
        raise RuntimeError(f"agemm.mx6_matmul: N={N} must be a multiple of 16")
    if tuple(SFA.shape) != (M, K // 32) or tuple(SFB.shape) != (N, K // 32):
        raise RuntimeError("agemm.mx6_matmul: SFA / SFB must be [rows, K/32]")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "mx6_matmul")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("mx6_matmul", A, B, SFA, SFB, alpha_dev, out, bias, residual)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp6(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), out.data_ptr(), M, N, K, code,
                                        alpha_host, alpha_p, bias_p, residual_p, oc, _stream(A))
    _lib.check(st, "mx6_matmul")
    return out
