"""Arena tests of the MXFP4 C-ABI (``-m gpu``): the quantisers (quantize_mx.hip) and the GEMMs on the block-scaled fp4 MFMA
(gemm_mx.hip: mx_small_kernel for M <= 64, mx_tile_kernel above, mx_slice_quant_kernel for the quantising epilogue at M <= 64), every
operand inside a poisoned arena (tests/arena.py).  Bit-exact against the same call on tight allocations; MXFP4 buffers have no
don't-care bytes, so what these cases pin is the `min(., M - 1)` clamps on every A / SFA pointer, the clamped K steps of the small-M
kernels and the stores of the ragged last tile."""
import pytest
import torch

from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8, I16 = torch.bfloat16, torch.float32, torch.uint8, torch.int16
MS = [1, 17, 65, 130]          # one and two row groups of the small-M kernels; one ragged tile and two tiles of the tiled kernel


def _L():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(BF16)


def _packed(rows, Kp, g):
    """Random e2m1 codes and E8M0 scale bytes 2^-7 .. 2^6 -> In(codes [rows, Kp/2]), In(scales [rows, Kp/32])."""
    q = torch.randint(0, 256, (rows, Kp // 2), generator=g, device=DEV, dtype=U8)
    sf = torch.randint(120, 134, (rows, Kp // 32), generator=g, device=DEV, dtype=U8)
    return In(q, 16), In(sf, 4)


def _q_outs(M, KQ, KE):
    Kp = int(_L().arcq_mx_k_padded(KQ + KE))
    assert int(_L().arcq_mx_sf_bytes(M, KQ + KE)) == M * Kp // 32
    return {"Q": Out((M, Kp // 2), U8, 16), "SF": Out((M, Kp // 32), U8, 4)}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("KQ,KE", [(64, 0), (192, 64), (320, 64), (256, 256)])          # K = 64 and 384: padding blocks up to Kp
def test_mx_static_quantisers(M, KQ, KE):
    """arcq_mx_quantize_x and arcq_mx_quantize_w: every declared byte of QX / SFX is written (the padding blocks included)."""
    L, g = _L(), _gen(M + KQ)
    ins = {"X": In(_bf16((M, KQ), g, 3.0), 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}
    for fn in (L.arcq_mx_quantize_x, L.arcq_mx_quantize_w):
        def call(o):
            return fn(_p(o["X"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), M, KQ, KE, _stream())
        run_in_arenas(call, ins, _q_outs(M, KQ, KE), device=DEV)


@pytest.mark.parametrize("M", MS)
def test_mx_fused_quantisers(M):
    """arcq_mx_rmsnorm_quantize_x (2048 <= KQ) and arcq_mx_silu_mul_quantize_x (both layouts)."""
    L, g = _L(), _gen(M + 5)
    for KQ, KE in ((2048, 64), (3584, 0)):
        ins = {"X": In(_bf16((M, KQ), g, 3.0), 16), "Wn": In(_bf16((KQ,), g) * 0.1 + 1, 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}

        def call(o):
            return L.arcq_mx_rmsnorm_quantize_x(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), M, KQ, KE, _stream())
        run_in_arenas(call, ins, _q_outs(M, KQ, KE), device=DEV)
    for KQ, KE, layout in ((192, 64, 0), (320, 0, 1), (64, 64, 1)):
        ins = {"GU": In(_bf16((M, 2 * KQ), g, 3.0), 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}

        def call(o):
            return L.arcq_mx_silu_mul_quantize_x(_p(o["GU"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), M, KQ, KE, layout, _stream())
        run_in_arenas(call, ins, _q_outs(M, KQ, KE), device=DEV)


def _epi(M, N, g, residual=True):
    ins = {"bias": In(_bf16((N,), g), 2), "alpha_dev": In(torch.tensor([0.5], dtype=F32, device=DEV), 4)}       # bias, residual: 2-byte aligned (arcq.h)
    if residual:
        ins["residual"] = In(_bf16((M, N), g), 2)
    return ins


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", [(144, 128), (176, 384), (16, 1152)])          # N % 64 != 0; 1, 3 and 9 K steps over the small kernel's 8 waves
def test_gemm_mxfp4(M, N, K):
    """arcq_gemm_mxfp4: mx_small_kernel (M = 1, 17) and mx_tile_kernel (M = 65, 130), bf16 plain, fp32 and bf16 with bias + residual +
    alpha_dev, and the residual aliasing D."""
    L, g = _L(), _gen(M + N + K)
    a, sfa = _packed(M, K, g)
    b, sfb = _packed(N, K, g)
    base = {"A": a, "B": b, "SFA": sfa, "SFB": sfb}
    for out_dtype, epi, alias in ((BF16, False, False), (F32, True, False), (BF16, True, False), (BF16, True, True)):
        ins = dict(base)
        if epi:
            ins.update(_epi(M, N, g, residual=not alias))
        oc = 0 if out_dtype is BF16 else 1

        def call(o):
            res = o["D"] if alias else o.get("residual")
            return L.arcq_gemm_mxfp4(_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["D"]), M, N, K, 0.01, _p(o.get("alpha_dev")), _p(o.get("bias")),
                                     _p(res), oc, None, 0, _stream())
        run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16, init=_bf16((M, N), g) if alias else None)}, device=DEV)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", [(144, 128), (176, 384)])
def test_gemm_mxfp4_silu_mul(M, N, K):
    """arcq_gemm_mxfp4_silu_mul: ACT = bf16 [M, N/2], both kernels, with and without bias."""
    L, g = _L(), _gen(M + N + K + 1)
    a, sfa = _packed(M, K, g)
    b, sfb = _packed(N, K, g)
    for bias in (False, True):
        ins = {"A": a, "B": b, "SFA": sfa, "SFB": sfb}
        if bias:
            ins.update(_epi(M, N, g, residual=False))

        def call(o):
            return L.arcq_gemm_mxfp4_silu_mul(_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["ACT"]), M, N, K, 0.004, _p(o.get("alpha_dev")),
                                              _p(o.get("bias")), _stream())
        run_in_arenas(call, ins, {"ACT": Out((M, N // 2), BF16, 16)}, device=DEV)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,KE", [(256, 128, 64), (384, 384, 0), (256, 384, 128)])      # N = 256 is the smallest with KE = 64; KQ2 = 192: a padding block
def test_gemm_mxfp4_silu_mul_quantize(M, N, K, KE):
    """arcq_gemm_mxfp4_silu_mul_quantize: QACT / SFACT are outputs and every declared byte is written (mx_slice_quant_kernel for
    M <= 64, mx_tile_kernel's quantising epilogue above)."""
    L, g = _L(), _gen(M + N + K + 2)
    a, sfa = _packed(M, K, g)
    b, sfb = _packed(N, K, g)
    Kp2 = int(L.arcq_mx_k_padded(N // 2 + KE))
    for bias in (False, True):
        ins = {"A": a, "B": b, "SFA": sfa, "SFB": sfb}
        if bias:
            ins.update(_epi(M, N, g, residual=False))

        def call(o):
            return L.arcq_gemm_mxfp4_silu_mul_quantize(_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["QACT"]), _p(o["SFACT"]), M, N, K, 0.004,
                                                       _p(o.get("alpha_dev")), _p(o.get("bias")), KE, _stream())
        run_in_arenas(call, ins, {"QACT": Out((M, Kp2 // 2), U8, 16), "SFACT": Out((M, Kp2 // 32), U8, 4)}, device=DEV)
