"""Arena tests of the MXFP4 GEMMs that serve every batch size from the repacked weight (``-m gpu``; gemm_mx_tile_rw.hip,
gemm_mx_slice_rw.hip): arcq_gemm_mxfp4_rw, arcq_gemm_mxfp4_rw_silu_mul and arcq_gemm_mxfp4_rw_silu_mul_quantize with every operand inside
a poisoned arena (tests/arena.py), bit-exact against the same call on tight allocations.  MRSF's padding bytes (the steps of a partial
last round, include/arcq.h) are the one don't-care region: they hold the poison in the arena copy.  What the cases pin: the tile kernel's
row blocks clamped to N/16 - 1 (seven of eight at N = 16, seven of the second column tile at N = 144), its A rows clamped to M - 1, the K
steps clamped to the last one, the four MRSF dwords of a step in a partial round, the row and column guards of the stores; and the
quantising decode kernel's four row blocks, its clamped second A fragment and the padding blocks it writes."""
import pytest
import torch

from arcquant_amd import agemm
from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
# tile kernel: one step, 63 clamped rows, seven clamped row blocks; tile kernel: 33 steps = a partial second round, a second row tile of
# one row, a second column tile with one live row block; decode kernels: 33 steps, two A fragments
SHAPES = [(65, 16, 128), (129, 144, 4224), (17, 128, 4224)]


def _L():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(BF16)


def _operands(M, N, K, g):
    a = torch.randint(0, 256, (M, K // 2), generator=g, device=DEV, dtype=U8)
    sfa = torch.randint(120, 134, (M, K // 32), generator=g, device=DEV, dtype=U8)
    qw = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=U8)
    sfw = torch.randint(120, 134, (N, K // 32), generator=g, device=DEV, dtype=U8)
    mrw, mrsf = agemm.mx_repack_w(qw, sfw)
    T, R = K // 128, -(-(K // 128) // 32)
    pad = torch.ones((N // 16, R, 8, 64, 4), dtype=torch.bool)
    t = torch.arange(T)
    pad[:, t // 32, t % 8, :, (t // 8) % 4] = False
    assert int(pad.sum()) == (N // 16) * (R * 32 - T) * 64
    return {"A": In(a, 16), "MRW": In(mrw, 16), "SFA": In(sfa, 4), "MRSF": In(mrsf, 4, dont_care=pad.reshape(-1) if pad.any() else None)}


def _epi(M, N, g, residual=True):
    ins = {"bias": In(_bf16((N,), g), 2), "alpha_dev": In(torch.tensor([0.5], dtype=F32, device=DEV), 4)}       # bias, residual: 2-byte aligned (arcq.h)
    if residual:
        ins["residual"] = In(_bf16((M, N), g), 2)
    return ins


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_mxfp4_rw(M, N, K):
    """bf16 plain, fp32 and bf16 with bias + residual + alpha_dev, and the residual aliasing D."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + K)
    assert L.arcq_gemm_mxfp4_rw_route(M, N, K) == (1 if M <= 64 else 2)
    base = _operands(M, N, K, g)
    for out_dtype, epi, alias in ((BF16, False, False), (F32, True, False), (BF16, True, False), (BF16, True, True)):
        ins = dict(base)
        if epi:
            ins.update(_epi(M, N, g, residual=not alias))
        oc = 0 if out_dtype is BF16 else 1

        def call(o):
            res = o["D"] if alias else o.get("residual")
            return L.arcq_gemm_mxfp4_rw(_p(o["A"]), _p(o["MRW"]), _p(o["SFA"]), _p(o["MRSF"]), _p(o["D"]), M, N, K, 0.01, _p(o.get("alpha_dev")),
                                        _p(o.get("bias")), _p(res), oc, _stream())
        run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16, init=_bf16((M, N), g) if alias else None)}, device=DEV)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_mxfp4_rw_silu_mul(M, N, K):
    """ACT = bf16 [M, N/2], with and without bias."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + K + 1)
    base = _operands(M, N, K, g)
    for bias in (False, True):
        ins = dict(base)
        if bias:
            ins.update(_epi(M, N, g, residual=False))

        def call(o):
            return L.arcq_gemm_mxfp4_rw_silu_mul(_p(o["A"]), _p(o["MRW"]), _p(o["SFA"]), _p(o["MRSF"]), _p(o["ACT"]), M, N, K, 0.004,
                                                 _p(o.get("alpha_dev")), _p(o.get("bias")), _stream())
        run_in_arenas(call, ins, {"ACT": Out((M, N // 2), BF16, 16)}, device=DEV)


@pytest.mark.parametrize("M,N,K", [(M, -(-N // 128) * 128, K) for M, N, K in SHAPES])     # N a multiple of 128: (65, 128, 128), (129, 256, 4224), (17, 128, 4224)
def test_gemm_mxfp4_rw_silu_mul_quantize(M, N, K):
    """(QACT, SFACT) with KE = 0 and KE = 64 (residual blocks, and at N = 128 two padding blocks), with and without bias."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + K + 2)
    base = _operands(M, N, K, g)
    for KE, bias in ((0, False), (64, True)):
        ins = dict(base)
        if bias:
            ins.update(_epi(M, N, g, residual=False))
        Kp2 = (N // 2 + KE + 127) // 128 * 128

        def call(o):
            return L.arcq_gemm_mxfp4_rw_silu_mul_quantize(_p(o["A"]), _p(o["MRW"]), _p(o["SFA"]), _p(o["MRSF"]), _p(o["QACT"]), _p(o["SFACT"]), M, N, K,
                                                          0.004, _p(o.get("alpha_dev")), _p(o.get("bias")), KE, _stream())
        run_in_arenas(call, ins, {"QACT": Out((M, Kp2 // 2), U8, 16), "SFACT": Out((M, Kp2 // 32), U8, 1)}, device=DEV)
