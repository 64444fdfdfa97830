"""MXFP4 decoder-layer operators (include/arcq.h "MXFP4 decoder-layer operators"): the fused RMSNorm and SiLU*up
quantisers and the gate|up GEMM with SiLU*up in its epilogue -- what ``agemm.rmsnorm_quantize_x``, ``silu_mul_quantize_x_dynamic`` and
``matmul_silu_mul`` are to NVFP4.  MXFP4 has no per-tensor scale, so each operator is ONE launch and returns no scale and no abs-max
slots.  ``matmul_silu_mul_quantize`` ends the family: the gate|up GEMM that writes the down projection's quantised input itself, which
NVFP4's per-tensor scale rules out (``gate_up_rows`` lays the weight out for it).  The decode path over a weight repacked into MFMA
operand order is here too: ``mx_repack_w`` / ``mx_unrepack_w``, ``mx_matmul_repacked`` and ``matmul_silu_mul_repacked`` (1 <= M <= 64, bit
for bit the results of ``mx_matmul`` / ``matmul_silu_mul``), and the three GEMMs over the repacked weight ALONE at every M --
``mx_matmul_rw``, ``matmul_silu_mul_rw``, ``matmul_silu_mul_quantize_rw`` (``mx_rw_route`` says which kernel serves a shape) -- with
which a layer keeps one weight copy.

The plain MXFP4 quantisers and GEMM stay in ``agemm`` (``mx_reorder_quantize_{x,w}``, ``mx_matmul``).  This module is a ctypes mirror
only: the extension module ``agemm.so`` does not bind these operators.  Validation follows the mirror's order (``agemm._need`` ...):
dtype / rank / contiguity, then the size relations, then the optional tensors, and LAST where everything lives.
"""
from __future__ import annotations

import functools

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


# ---- the MXFP4 repacked weight (include/arcq.h "MXFP4 repacked weight") and the decode GEMMs over it; also reachable as
# agemm.mx_repack_w, agemm.mx_unrepack_w, agemm.mx_repacked_supported, agemm.mx_matmul_repacked and agemm.MX_REPACKED_MAX_M.
# Layers and the harness take the repacked GEMMs for calls of at most MX_REPACKED_MAX_M tokens and ``mx_matmul`` above.  It is the
# kernel's own limit (arcq_gemm_mxfp4_repacked_supported): measured against ``mx_matmul`` the repacked kernel is ahead at every M up to
# 64 (profiles/mxfp4_repacked_decode.json), so nothing lowers it.
MX_REPACKED_MAX_M = 64
_MX_ROUND = 32          # K steps of one MRSF round: 8 waves x the 4 bytes of a dword
_MX_SF_PAD = 127        # padding bytes of a partial MRSF round: E8M0 2^0 (never multiplied)


@functools.lru_cache(maxsize=None)
def _mx_repacked_bytes(N: int, K: int):
    L = _lib.lib()
    return int(L.arcq_mx_repacked_w_bytes(N, K)), int(L.arcq_mx_repacked_sf_bytes(N, K))


def mx_repack_w(QW: torch.Tensor, SFW: torch.Tensor):
    """One-time re-layout of an MXFP4 weight for the decode path (include/arcq.h, "MXFP4 repacked weight"): returns ``(MRW, MRSF)``.
    Pure data movement with torch ops -- the codes and E8M0 bytes are those ``mx_reorder_quantize_w`` wrote:
    MRW  = [row blocks of 16][steps of 128 K][lane = 16*q + r][16 bytes], as many bytes as QW;
    MRSF = [row blocks][rounds of 32 steps][wave = t % 8][lane][u = (t / 8) % 4], the steps of a partial last round padded with 127.
    ``mx_unrepack_w`` is its inverse; both also run on CPU tensors.  N % 16 == 0, K % 128 == 0 (K is the stored Kp)."""
    _need(QW, torch.uint8, "QW", 2)            # (pure data movement: no device rule)
    _need(SFW, torch.uint8, "SFW", 2)
    N, K = QW.shape[0], QW.shape[1] * 2
    if N == 0 or K == 0 or N % 16 or K % 128:
        raise RuntimeError(f"Value error in mx_repack_w: N={N} must be a multiple of 16 and K={K} a multiple of 128")
    if tuple(SFW.shape) != (N, K // 32):
        raise RuntimeError(f"Value error in mx_repack_w: SFW must be [{N}, {K // 32}]")
    RB, T = N // 16, K // 128
    R = (T + _MX_ROUND - 1) // _MX_ROUND
    # codes: [RB, r, T, q, 16 B] -> [RB, T, q, r, 16 B]
    MRW = QW.view(RB, 16, T, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    # scales: step t = 32 round + 8 u + wave; [RB, r, round, u, wave, q] -> [RB, round, wave, q, r, u]
    sf = torch.full((RB, 16, R * _MX_ROUND, 4), _MX_SF_PAD, dtype=torch.uint8, device=QW.device)
    sf[:, :, :T] = SFW.view(RB, 16, T, 4)
    MRSF = sf.view(RB, 16, R, 4, 8, 4).permute(0, 2, 4, 5, 1, 3).contiguous().view(-1)
    assert (MRW.numel(), MRSF.numel()) == _mx_repacked_bytes(N, K)
    return MRW, MRSF


def mx_unrepack_w(MRW: torch.Tensor, MRSF: torch.Tensor, N: int, K: int):
    """The exact inverse of ``mx_repack_w`` (pure data movement with torch ops, on MRW's device): returns ``(QW u8 [N, K/2], SFW u8
    [N, K/32])`` as ``mx_reorder_quantize_w`` wrote them; the padding bytes of MRSF are dropped."""
    _need(MRW, torch.uint8, "MRW", 1)
    _need(MRSF, torch.uint8, "MRSF", 1)
    N, K = int(N), int(K)
    if N <= 0 or K <= 0 or N % 16 or K % 128 or (MRW.numel(), MRSF.numel()) != _mx_repacked_bytes(N, K):
        raise RuntimeError(f"Value error in mx_unrepack_w: MRW / MRSF do not belong to a [{N}, {K}] MXFP4 weight (N % 16 == 0, K % 128 == 0)")
    RB, T = N // 16, K // 128
    R = (T + _MX_ROUND - 1) // _MX_ROUND
    QW = MRW.view(RB, T, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K // 2)
    sf = MRSF.view(RB, R, 8, 4, 16, 4).permute(0, 4, 1, 5, 2, 3).reshape(RB, 16, R * _MX_ROUND, 4)
    return QW, sf[:, :, :T].reshape(N, K // 32)


@functools.lru_cache(maxsize=None)
def mx_repacked_supported(M: int, N: int, K: int) -> bool:
    """Whether ``mx_matmul_repacked`` can run this shape: 1 <= M <= 64, N % 16 == 0, K % 128 == 0."""
    return bool(_lib.lib().arcq_gemm_mxfp4_repacked_supported(int(M), int(N), int(K)))


def _need_mx_repacked(A, MRW, SFA, MRSF, N, who, any_m=False):
    # A / SFA are the activations of an [M, K] call, (MRW, MRSF) the repacked MXFP4 weight of N rows over this K -> (M, N, K)
    # any_m: the *_rw calls, which serve every M (the boundary bounds it as arcq_gemm_mxfp4 does)
    _need(A, torch.uint8, "A", 2)
    _need(MRW, torch.uint8, "MRW", 1)
    _need(SFA, torch.uint8, "SFA", 2)
    _need(MRSF, torch.uint8, "MRSF", 1)
    M, K, N = A.shape[0], A.shape[1] * 2, int(N)
    if K % 128:
        raise RuntimeError(f"{who}: K={K} is not a padded MXFP4 K (a multiple of 128)")
    if N <= 0 or N % 16:
        raise RuntimeError(f"{who}: N={N} must be a positive multiple of 16")
    if (MRW.numel(), MRSF.numel()) != _mx_repacked_bytes(N, K):
        raise RuntimeError(f"{who}: MRW / MRSF do not belong to a [{N}, {K}] MXFP4 weight")
    if tuple(SFA.shape) != (M, K // 32):
        raise RuntimeError(f"{who}: SFA must be [rows, K/32]")
    if not any_m and not mx_repacked_supported(M, N, K):
        raise RuntimeError(f"{who}: M={M} is outside the repacked path (1 <= M <= {MX_REPACKED_MAX_M}; see mx_repacked_supported)")
    return M, N, K


def mx_matmul_repacked(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *, bias=None, residual=None,
                       out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """``mx_matmul`` for decode shapes (1 <= M <= 64) over a weight prepared by ``mx_repack_w`` (same arguments otherwise, plus the row
    count ``N`` of the weight): every weight load is one contiguous span and the weight is read once whatever M is.  Bit for bit the
    result of ``mx_matmul`` on the un-repacked operands (the same sums in the same order)."""
    M, N, K = _need_mx_repacked(A, MRW, SFA, MRSF, N, "mx.mx_matmul_repacked")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "mx.mx_matmul_repacked")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("mx.mx_matmul_repacked", A, MRW, SFA, MRSF, alpha_dev, out, bias, residual)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_repacked(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N, K,
                                                 alpha_host, alpha_p, bias_p, residual_p, oc, _stream(A))
    _lib.check(st, "mx.mx_matmul_repacked")
    return out


def matmul_silu_mul_repacked(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *, scale_host: float = 1.0,
                             bias=None, out=None):
    """``matmul_silu_mul`` for decode shapes (1 <= M <= 64) over the gate|up weight as ``agemm.mx_repack_w`` left it (rows interleaving
    gate and up; ``N`` is its row count).  Returns ``act`` bf16 [M, N/2], bit for bit what ``matmul_silu_mul`` returns on the
    un-repacked weight."""
    M, N, K = _need_mx_repacked(A, MRW, SFA, MRSF, N, "mx.matmul_silu_mul_repacked")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, _ = _out(out, M, N // 2, torch.bfloat16, A, "mx.matmul_silu_mul_repacked")
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("mx.matmul_silu_mul_repacked", A, MRW, SFA, MRSF, alpha_dev, out, bias)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_repacked_silu_mul(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N, K,
                                                          alpha_host, alpha_p, bias_p, _stream(A))
    _lib.check(st, "mx.matmul_silu_mul_repacked")
    return out


@functools.lru_cache(maxsize=None)
def mx_rw_route(M: int, N: int, K: int) -> int:
    """Which kernel serves an ``mx_matmul_rw`` call of this shape: 1 = the decode kernels (M <= 64: the call is ``mx_matmul_repacked``), 2 =
    the tile kernel over the repacked weight, 0 = no such shape (M < 1, N % 16, K % 128)."""
    return int(_lib.lib().arcq_gemm_mxfp4_rw_route(int(M), int(N), int(K)))


def mx_matmul_rw(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *, bias=None, residual=None,
                 out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """``mx_matmul`` at EVERY M over the repacked weight alone (``mx_repack_w``; arguments as ``mx_matmul_repacked``): up to 64 rows the
    decode kernel, above it the tile kernel with its B operand staged from ``(MRW, MRSF)``.  Bit for bit the result of ``mx_matmul`` on
    the un-repacked operands, so a layer can keep this one copy of its weight."""
    M, N, K = _need_mx_repacked(A, MRW, SFA, MRSF, N, "mx.mx_matmul_rw", any_m=True)
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "mx.mx_matmul_rw")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("mx.mx_matmul_rw", A, MRW, SFA, MRSF, alpha_dev, out, bias, residual)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_rw(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N, K, alpha_host,
                                           alpha_p, bias_p, residual_p, oc, _stream(A))
    _lib.check(st, "mx.mx_matmul_rw")
    return out


def matmul_silu_mul_rw(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *, scale_host: float = 1.0,
                       bias=None, out=None):
    """``matmul_silu_mul`` at every M over the repacked gate|up weight alone (arguments as ``matmul_silu_mul_repacked``).  Returns ``act``
    bf16 [M, N/2], bit for bit what ``matmul_silu_mul`` returns on the un-repacked weight."""
    M, N, K = _need_mx_repacked(A, MRW, SFA, MRSF, N, "mx.matmul_silu_mul_rw", any_m=True)
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, _ = _out(out, M, N // 2, torch.bfloat16, A, "mx.matmul_silu_mul_rw")
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("mx.matmul_silu_mul_rw", A, MRW, SFA, MRSF, alpha_dev, out, bias)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_rw_silu_mul(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N, K,
                                                    alpha_host, alpha_p, bias_p, _stream(A))
    _lib.check(st, "mx.matmul_silu_mul_rw")
    return out


def matmul_silu_mul_quantize_rw(A: torch.Tensor, MRW: torch.Tensor, SFA: torch.Tensor, MRSF: torch.Tensor, scale, N: int, KE: int, *,
                                scale_host: float = 1.0, bias=None):
    """``matmul_silu_mul_quantize`` at every M over the repacked gate|up weight alone: ``(MRW, MRSF, N)`` in place of ``(B, SFB)``, the
    other arguments and the result -- (QX, SFX) of the down projection's input -- byte for byte the same.  N % 128 == 0, KE % 64 == 0,
    0 <= KE <= N/2 <= 32767."""
    for t, name, rank in ((A, "A", 2), (MRW, "MRW", 1), (SFA, "SFA", 2), (MRSF, "MRSF", 1)):
        _need(t, torch.uint8, name, rank)
    M, K, N, KE = A.shape[0], A.shape[1] * 2, int(N), int(KE)
    if K % 128:
        raise RuntimeError(f"mx.matmul_silu_mul_quantize_rw: K={K} is not a padded MXFP4 K (a multiple of 128)")
    if N <= 0 or N % 128:
        raise RuntimeError(f"mx.matmul_silu_mul_quantize_rw: N={N} must be a positive multiple of 128 (N/2 activations in whole pairs of 32-blocks)")
    if KE % 64 or KE < 0 or KE > N // 2 or N // 2 > 32767:
        raise RuntimeError(f"Value error in mx.matmul_silu_mul_quantize_rw: KQ={N // 2}, KE={KE} is not valid")
    if (MRW.numel(), MRSF.numel()) != _mx_repacked_bytes(N, K):
        raise RuntimeError(f"mx.matmul_silu_mul_quantize_rw: MRW / MRSF do not belong to a [{N}, {K}] MXFP4 weight")
    if tuple(SFA.shape) != (M, K // 32):
        raise RuntimeError("mx.matmul_silu_mul_quantize_rw: SFA must be [rows, K/32]")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("mx.matmul_silu_mul_quantize_rw", A, MRW, SFA, MRSF, alpha_dev, bias)
    QX, SFX = _outputs(M, N // 2, KE, A)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_rw_silu_mul_quantize(A.data_ptr(), MRW.data_ptr(), SFA.data_ptr(), MRSF.data_ptr(), QX.data_ptr(),
                                                             SFX.data_ptr(), M, N, K, alpha_host, alpha_p, bias_p, KE, _stream(A))
    _lib.check(st, "mx.matmul_silu_mul_quantize_rw")
    return QX, SFX


def matmul_silu_mul_quantize(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale, KE: int, *, scale_host: float = 1.0,
                             bias=None):
    """The gate|up GEMM that writes the down projection's quantised input: operands as ``matmul_silu_mul`` -> (QX u8 [M, Kp2/2], SFX u8
    E8M0 [M, Kp2/32]) with KQ2 = N/2 and Kp2 = mx_k_padded(KQ2 + KE), byte for byte
    ``agemm.mx_reorder_quantize_x(matmul_silu_mul(A, B, SFA, SFB, scale, ...), arange(KQ2), KE)``; the activation is never written.
    There is no reorder_index: activation j is channel j of the result, so the channel order is the order of ``B``'s row pairs
    (``gate_up_rows``).  KQ2 % 64 == 0 (N % 128 == 0), KE % 64 == 0, 0 <= KE <= KQ2 <= 32767."""
    for t, name in ((A, "A"), (B, "B"), (SFA, "SFA"), (SFB, "SFB")):
        _need(t, torch.uint8, name, 2)
    M, N, K = A.shape[0], B.shape[0], A.shape[1] * 2
    KE = int(KE)
    if B.shape[1] * 2 != K:
        raise RuntimeError(f"mx.matmul_silu_mul_quantize: A has K={K}, B has K={B.shape[1] * 2}")
    if K % 128:
        raise RuntimeError(f"mx.matmul_silu_mul_quantize: K={K} is not a padded MXFP4 K (a multiple of 128)")
    if N % 128:
        raise RuntimeError(f"mx.matmul_silu_mul_quantize: N={N} must be a multiple of 128 (N/2 activations in whole pairs of 32-blocks)")
    if KE % 64 or KE < 0 or KE > N // 2 or N // 2 > 32767:
        raise RuntimeError(f"Value error in mx.matmul_silu_mul_quantize: KQ={N // 2}, KE={KE} is not valid")
    if tuple(SFA.shape) != (M, K // 32) or tuple(SFB.shape) != (N, K // 32):
        raise RuntimeError("mx.matmul_silu_mul_quantize: SFA / SFB must be [rows, K/32]")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("mx.matmul_silu_mul_quantize", A, B, SFA, SFB, alpha_dev, bias)
    QX, SFX = _outputs(M, N // 2, KE, A)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4_silu_mul_quantize(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), QX.data_ptr(), SFX.data_ptr(),
                                                          M, N, K, alpha_host, alpha_p, bias_p, KE, _stream(A))
    _lib.check(st, "mx.matmul_silu_mul_quantize")
    return QX, SFX


# ---- the fused decode linears (include/arcq.h "MXFP4 fused decode linear"): the activation quantiser as the prologue of the repacked
# decode GEMM, one launch, bit for bit the two calls it replaces.  ``linear_fused_supported`` is also agemm.mx_linear_fused_supported.
SRC_RMSNORM, SRC_PLAIN = 1, 3
MX_LINEAR_MAX_M = 16


@functools.lru_cache(maxsize=4096)
def linear_fused_supported(kind: int, M: int, N: int, KQ: int, KE: int) -> bool:
    """Whether the fused MXFP4 decode linear can run this shape: a valid shape for ``kind`` (SRC_RMSNORM: 2048 <= KQ <= 8192; SRC_PLAIN),
    1 <= M <= 16 and an LDS image that leaves two workgroups per CU (``linear_fused_lds_bytes`` <= 81920).  Callers fall back to the
    quantiser followed by ``mx_matmul_repacked`` / ``matmul_silu_mul_repacked`` otherwise."""
    return bool(_lib.lib().arcq_mx_linear_fused_supported(int(kind), int(M), int(N), int(KQ), int(KE)))


mx_linear_fused_supported = linear_fused_supported


def linear_fused_workgroups(kind: int, N: int, KQ: int, KE: int) -> int:
    """Workgroups of a fused launch (pure host arithmetic): min(N / 16, 512); workgroup g takes the row blocks g, g + grid, ...; 0 for an
    unsupported shape."""
    return int(_lib.lib().arcq_mx_linear_fused_workgroups(int(kind), int(N), int(KQ), int(KE)))


def linear_fused_lds_bytes(kind: int, KQ: int, KE: int) -> int:
    """The LDS a fused launch of this K takes (the budget formula of include/arcq.h)."""
    return int(_lib.lib().arcq_mx_linear_fused_lds_bytes(int(kind), int(KQ), int(KE)))


def _need_mx_linear(who, kind, X, W, reorder_index, KE, MRW, MRSF, N):
    # X [M, KQ] bf16 (and the norm weight) against the repacked MXFP4 weight of N rows over Kp = mx_k_padded(KQ + KE) -> (M, N, KQ, KE)
    _need(X, torch.bfloat16, "X", 2)
    if kind == SRC_RMSNORM:
        _need(W, torch.bfloat16, "W", 1)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    _need(MRW, torch.uint8, "MRW", 1)
    _need(MRSF, torch.uint8, "MRSF", 1)
    (M, KQ), KE, N = X.shape, int(KE), int(N)
    if reorder_index.numel() != KQ or (kind == SRC_RMSNORM and W.numel() != KQ):
        raise RuntimeError(f"{who}: W / reorder_index must have X.shape[1] = {KQ} entries")
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or KQ > 32767 or (kind == SRC_RMSNORM and not (2048 <= KQ <= 8192)):
        raise RuntimeError(f"Value error in {who}: KQ={KQ}, KE={KE} is not valid" + (" (2048 <= KQ <= 8192)" if kind == SRC_RMSNORM else ""))
    if N <= 0 or N % 16:
        raise RuntimeError(f"{who}: N={N} must be a positive multiple of 16")
    if (MRW.numel(), MRSF.numel()) != _mx_repacked_bytes(N, mx_k_padded(KQ + KE)):
        raise RuntimeError(f"{who}: MRW / MRSF do not belong to a [{N}, {mx_k_padded(KQ + KE)}] MXFP4 weight")
    if not linear_fused_supported(kind, M, N, KQ, KE):
        raise RuntimeError(f"{who}: M={M}, KQ={KQ}, KE={KE} is outside the fused path (1 <= M <= {MX_LINEAR_MAX_M} and the LDS budget; see "
                           f"linear_fused_supported)")
    return M, N, KQ, KE


def linear_rmsnorm_repacked(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int, MRW: torch.Tensor,
                            MRSF: torch.Tensor, scale, N: int, *, bias=None, residual=None, out_dtype=torch.bfloat16, out=None,
                            scale_host: float = 1.0):
    """``mx_matmul_repacked(*rmsnorm_quantize_x(X, W, eps, reorder_index, KE), ...)`` in ONE launch for 1 <= M <= 16: the RMSNorm and the
    MXFP4-ARC quantiser run as the GEMM's prologue and nothing quantised is written to memory.  Bit for bit the result of the two
    calls.  ``W`` is the norm weight; ``residual`` may be ``out``."""
    who = "mx.linear_rmsnorm_repacked"
    M, N, KQ, KE = _need_mx_linear(who, SRC_RMSNORM, X, W, reorder_index, KE, MRW, MRSF, N)
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, X, who)
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device(who, X, W, reorder_index, MRW, MRSF, alpha_dev, out, bias, residual)
    with _on(X.device):
        st = _lib.lib().arcq_mx_linear_rmsnorm_repacked(X.data_ptr(), W.data_ptr(), float(eps), reorder_index.data_ptr(), MRW.data_ptr(),
                                                        MRSF.data_ptr(), out.data_ptr(), M, N, KQ, KE, alpha_host, alpha_p, bias_p, residual_p, oc,
                                                        _stream(X))
    _lib.check(st, who)
    return out


def linear_rmsnorm_silu_repacked(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int, MRW: torch.Tensor,
                                 MRSF: torch.Tensor, scale, N: int, *, bias=None, out=None, scale_host: float = 1.0):
    """``matmul_silu_mul_repacked(*rmsnorm_quantize_x(X, W, eps, reorder_index, KE), ...)`` in ONE launch for 1 <= M <= 16 (the gate|up
    weight's rows interleave gate and up).  Returns ``act`` bf16 [M, N/2], bit for bit the result of the two calls."""
    who = "mx.linear_rmsnorm_silu_repacked"
    M, N, KQ, KE = _need_mx_linear(who, SRC_RMSNORM, X, W, reorder_index, KE, MRW, MRSF, N)
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, _ = _out(out, M, N // 2, torch.bfloat16, X, who)
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device(who, X, W, reorder_index, MRW, MRSF, alpha_dev, out, bias)
    with _on(X.device):
        st = _lib.lib().arcq_mx_linear_rmsnorm_silu_repacked(X.data_ptr(), W.data_ptr(), float(eps), reorder_index.data_ptr(), MRW.data_ptr(),
                                                             MRSF.data_ptr(), out.data_ptr(), M, N, KQ, KE, alpha_host, alpha_p, bias_p, _stream(X))
    _lib.check(st, who)
    return out


def linear_quantize_repacked(X: torch.Tensor, reorder_index: torch.Tensor, KE: int, MRW: torch.Tensor, MRSF: torch.Tensor, scale, N: int, *,
                             bias=None, residual=None, out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """``mx_matmul_repacked(*agemm.mx_reorder_quantize_x(X, reorder_index, KE), ...)`` in ONE launch for 1 <= M <= 16.  Bit for bit the
    result of the two calls; ``residual`` may be ``out``."""
    who = "mx.linear_quantize_repacked"
    M, N, KQ, KE = _need_mx_linear(who, SRC_PLAIN, X, None, reorder_index, KE, MRW, MRSF, N)
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, X, who)
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device(who, X, reorder_index, MRW, MRSF, alpha_dev, out, bias, residual)
    with _on(X.device):
        st = _lib.lib().arcq_mx_linear_quantize_repacked(X.data_ptr(), reorder_index.data_ptr(), MRW.data_ptr(), MRSF.data_ptr(), out.data_ptr(), M, N,
                                                         KQ, KE, alpha_host, alpha_p, bias_p, residual_p, oc, _stream(X))
    _lib.check(st, who)
    return out


def gate_up_rows(gate_w: torch.Tensor, up_w: torch.Tensor, reorder_index=None, gate_b=None, up_b=None):
    """The gate|up weight of ``matmul_silu_mul`` / ``matmul_silu_mul_quantize`` from the two projections' [KQ2, in_features] weights: rows
    g0, u0, g1, u1, ... where pair j is channel ``reorder_index[j]`` (None: channel j).  With the consumer's reorder_index the GEMM's
    activations come out in the order that quantiser would gather them into, which is what ``matmul_silu_mul_quantize`` (identity
    gather) needs; the weight is quantised per row, so permuting rows before quantising is exact.  Returns the [2*KQ2, in_features]
    weight, or (weight, bias [2*KQ2]) when ``gate_b`` and ``up_b`` are given."""
    if gate_w.dim() != 2 or gate_w.shape != up_w.shape or gate_w.dtype != up_w.dtype:
        raise RuntimeError(f"mx.gate_up_rows: gate_w and up_w must be 2-D of one shape and dtype, got {tuple(gate_w.shape)} / {tuple(up_w.shape)}")
    if (gate_b is None) != (up_b is None):
        raise RuntimeError("mx.gate_up_rows: gate_b and up_b come together or not at all")
    KQ2 = gate_w.shape[0]
    order = None
    if reorder_index is not None:
        order = reorder_index.reshape(-1).long()
        if order.numel() != KQ2 or not torch.equal(torch.sort(order).values, torch.arange(KQ2, device=order.device)):
            raise RuntimeError(f"mx.gate_up_rows: reorder_index must be a permutation of 0 .. {KQ2 - 1}")

    def pairs(g, u):
        if order is not None:
            g, u = g[order.to(g.device)], u[order.to(u.device)]
        return torch.stack((g, u), dim=1).reshape(2 * KQ2, *g.shape[1:]).contiguous()

    w = pairs(gate_w, up_w)
    if gate_b is None:
        return w
    if gate_b.shape != (KQ2,) or up_b.shape != (KQ2,):
        raise RuntimeError(f"mx.gate_up_rows: gate_b and up_b must have shape ({KQ2},)")
    return w, pairs(gate_b, up_b)
