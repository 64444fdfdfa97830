"""MXFP6 (quant_type='MXFP6'; include/arcq.h "MXFP6-ARC"): the e3m2 quantisers and the GEMM on the scaled MFMA with e3m2
activations against an e3m2 or an e2m1 weight, and the decode GEMM over the weight repacked into MFMA operand order.  Reached as
``agemm.mx6_reorder_quantize_{x,w}``, ``agemm.mx6_matmul``, ``agemm.mx6_repack_w`` / ``mx6_unrepack_w`` and ``agemm.mx6_matmul_repacked``
(``agemm`` re-exports them); a ctypes mirror only, the extension module ``agemm.so`` does not bind them.  Validation follows the mirror's order
(``agemm._need`` ...): dtype / rank / contiguity, then the size relations, then the optional tensors, and LAST where everything lives.
"""
from __future__ import annotations

import functools

import torch

from . import _lib
from .agemm import _alpha, _need, _on, _opt, _out, _same_device, _stream, mx_k_padded
from .mx import _mx_repack_sf, _mx_unrepack_sf


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


# ---- the MXFP6 repacked weight (include/arcq.h "MXFP6 repacked weight") and the decode GEMM over it; reachable as agemm.mx6_repack_w,
# agemm.mx6_unrepack_w, agemm.mx6_repacked_supported, agemm.mx6_matmul_repacked and agemm.MX6_REPACKED_MAX_M.  An e2m1 weight (W4A6) has
# no layout of its own: its repacked form is ``agemm.mx_repack_w``'s.  Layers take the repacked GEMM for calls of at most
# MX6_REPACKED_MAX_M tokens and ``mx6_matmul`` above; the constant follows from profiles/mxfp6_repacked_decode.json.
MX6_REPACKED_MAX_M = 64


@functools.lru_cache(maxsize=None)
def _mx6_repacked_bytes(N: int, K: int, b_format: str = "e3m2"):
    L = _lib.lib()
    w = L.arcq_mx6_repacked_w_bytes(N, K) if b_format == "e3m2" else L.arcq_mx_repacked_w_bytes(N, K)
    return int(w), int(L.arcq_mx_repacked_sf_bytes(N, K))


def mx6_repack_w(QW: torch.Tensor, SFW: torch.Tensor):
    """One-time re-layout of an e3m2 weight for the decode path (include/arcq.h, "MXFP6 repacked weight"): returns ``(MRW, MRSF)``.
    Pure data movement with torch ops -- the codes and E8M0 bytes are those ``mx6_reorder_quantize_w`` wrote:
    MRW  = layout MRW6, [row blocks of 16][steps of 128 K][1536 bytes]: bytes 0..15 of the 24-byte block of each lane 16*q + r, then
           bytes 16..23 of each lane's; as many bytes as QW;
    MRSF = ``mx_repack_w``'s scale array for the same SFW.
    ``mx6_unrepack_w`` is its inverse; both also run on CPU tensors.  N % 16 == 0, K % 128 == 0 (K is the stored Kp).  An e2m1 weight
    (``b_format="e2m1"``) is repacked with ``mx_repack_w``."""
    _need(QW, torch.uint8, "QW", 2)            # (pure data movement: no device rule)
    _need(SFW, torch.uint8, "SFW", 2)
    N, K = QW.shape[0], QW.shape[1] // 3 * 4
    if N == 0 or K == 0 or N % 16 or QW.shape[1] % 96:
        raise RuntimeError(f"Value error in mx6_repack_w: N={N} must be a multiple of 16 and a row a multiple of 96 bytes (128 elements), got {QW.shape[1]}")
    if tuple(SFW.shape) != (N, K // 32):
        raise RuntimeError(f"Value error in mx6_repack_w: SFW must be [{N}, {K // 32}]")
    RB, T = N // 16, K // 128
    x = QW.view(RB, 16, T, 4, 24).permute(0, 2, 3, 1, 4)        # [RB, r, T, q, 24 B] -> [RB, T, q, r, 24 B]
    MRW = torch.cat([x[..., :16].reshape(RB, T, 1024), x[..., 16:].reshape(RB, T, 512)], -1).reshape(-1)
    MRSF = _mx_repack_sf(SFW)
    assert (MRW.numel(), MRSF.numel()) == _mx6_repacked_bytes(N, K)
    return MRW, MRSF


def mx6_unrepack_w(MRW: torch.Tensor, MRSF: torch.Tensor, N: int, K: int):
    """The exact inverse of ``mx6_repack_w`` (pure data movement with torch ops, on MRW's device): returns ``(QW u8 [N, 3 K/4], SFW u8
    [N, K/32])`` as ``mx6_reorder_quantize_w`` wrote them; the padding bytes of MRSF are dropped."""
    _need(MRW, torch.uint8, "MRW", 1)
    _need(MRSF, torch.uint8, "MRSF", 1)
    N, K = int(N), int(K)
    if N <= 0 or K <= 0 or N % 16 or K % 128 or (MRW.numel(), MRSF.numel()) != _mx6_repacked_bytes(N, K):
        raise RuntimeError(f"Value error in mx6_unrepack_w: MRW / MRSF do not belong to a [{N}, {K}] e3m2 weight (N % 16 == 0, K % 128 == 0)")
    RB, T = N // 16, K // 128
    t = MRW.view(RB, T, 1536)
    x = torch.cat([t[..., :1024].reshape(RB, T, 4, 16, 16), t[..., 1024:].reshape(RB, T, 4, 16, 8)], -1)      # [RB, T, q, r, 24 B]
    return x.permute(0, 3, 1, 2, 4).reshape(N, 3 * K // 4), _mx_unrepack_sf(MRSF, N, K)


@functools.lru_cache(maxsize=None)
def mx6_repacked_supported(M: int, N: int, K: int) -> bool:
    """Whether ``mx6_matmul_repacked`` can run this shape: 1 <= M <= 64, N % 16 == 0, K % 128 == 0."""
    return bool(_lib.lib().arcq_gemm_mxfp6_repacked_supported(int(M), int(N), int(K)))


def mx6_matmul_repacked(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *, b_format: str = "e3m2",
                        bias=None, residual=None, out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """``mx6_matmul`` for decode shapes (1 <= M <= 64) over a repacked weight of ``N`` rows: ``mx6_repack_w``'s arrays for
    ``b_format="e3m2"``, ``mx_repack_w``'s for ``"e2m1"`` (W4A6: the copy an MXFP4 layer already keeps).  Every weight load is a contiguous
    span and the weight is read once whatever M is.  Against an e2m1 weight the result is bit for bit ``mx6_matmul``'s on the un-repacked
    operands; against an e3m2 weight the same exact products are summed in another grouping (the weight's codes are split, not the
    activations'), so the result agrees within the fp32 summation bound."""
    who = "agemm.mx6_matmul_repacked"
    _need(A, torch.uint8, "A", 2)
    _need(MRW, torch.uint8, "MRW", 1)
    _need(SFA, torch.uint8, "SFA", 2)
    _need(MRSF, torch.uint8, "MRSF", 1)
    if b_format not in _MX6_B_FORMATS:
        raise RuntimeError(f"{who}: b_format must be 'e3m2' or 'e2m1', got {b_format!r}")
    code = _MX6_B_FORMATS[b_format][0]
    M, N = A.shape[0], int(N)
    if A.shape[1] % 96:
        raise RuntimeError(f"{who}: A has {A.shape[1]} bytes per row, not a padded MXFP6 K (a multiple of 96 bytes = 128 elements)")
    K = A.shape[1] // 3 * 4
    if N <= 0 or N % 16:
        raise RuntimeError(f"{who}: N={N} must be a positive multiple of 16")
    if (MRW.numel(), MRSF.numel()) != _mx6_repacked_bytes(N, K, b_format):
        raise RuntimeError(f"{who}: MRW / MRSF do not belong to a [{N}, {K}] {b_format} weight")
    if tuple(SFA.shape) != (M, K // 32):
        raise RuntimeError(f"{who}: SFA must be [rows, K/32]")
    if not mx6_repacked_supported(M, N, K):
        raise RuntimeError(f"{who}: M={M} is outside the repacked path (1 <= M <= 64; see mx6_repacked_supported)")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "mx6_matmul_repacked")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("mx6_matmul_repacked", A, MRW, SFA, MRSF, alpha_dev, out, bias, residual)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp6_repacked(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N, K, code,
                                                 alpha_host, alpha_p, bias_p, residual_p, oc, _stream(A))
    _lib.check(st, "mx6_matmul_repacked")
    return out
