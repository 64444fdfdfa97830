"""Arena tests of the MXFP4 decode GEMMs over the repacked weight (``-m gpu``; gemm_mx_rw.hip): arcq_gemm_mxfp4_repacked and
arcq_gemm_mxfp4_repacked_silu_mul with every operand inside a poisoned arena (tests/arena.py), bit-exact against the same call on tight
allocations.  MRSF's padding bytes (the steps of a partial last round, include/arcq.h) are the one don't-care region: they hold the
poison in the arena copy.  What the cases pin: the `min(., M - 1)` clamps on every A / SFA pointer, the K steps clamped to the last
one, the MRSF dword of a partial round and the row guards of the stores."""
import pytest
import torch

from arcquant_amd import agemm
from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
# one step and one row (seven idle waves, 15 clamped rows); 33 steps = a partial second round, two A fragments, three row blocks;
# two full rounds and four full fragments
SHAPES = [(1, 16, 128), (17, 48, 4224), (64, 32, 8192)]


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
def test_gemm_mxfp4_repacked(M, N, K):
    """bf16 plain, fp32 and bf16 with bias + residual + alpha_dev, and the residual aliasing D."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + K)
    base = _operands(M, N, K, g)
    for out_dtype, epi, alias in ((BF16, False, False), (F32, True, False), (BF16, True, False), (BF16, True, True)):
        ins = dict(base)
        if epi:
            ins.update(_epi(M, N, g, residual=not alias))
        oc = 0 if out_dtype is BF16 else 1

        def call(o):
            res = o["D"] if alias else o.get("residual")
            return L.arcq_gemm_mxfp4_repacked(_p(o["A"]), _p(o["MRW"]), _p(o["SFA"]), _p(o["MRSF"]), _p(o["D"]), M, N, K, 0.01, _p(o.get("alpha_dev")),
                                              _p(o.get("bias")), _p(res), oc, _stream())
        run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16, init=_bf16((M, N), g) if alias else None)}, device=DEV)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_mxfp4_repacked_silu_mul(M, N, K):
    """ACT = bf16 [M, N/2], with and without bias."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + K + 1)
    base = _operands(M, N, K, g)
    for bias in (False, True):
        ins = dict(base)
        if bias:
            ins.update(_epi(M, N, g, residual=False))

        def call(o):
            return L.arcq_gemm_mxfp4_repacked_silu_mul(_p(o["A"]), _p(o["MRW"]), _p(o["SFA"]), _p(o["MRSF"]), _p(o["ACT"]), M, N, K, 0.004,
                                                       _p(o.get("alpha_dev")), _p(o.get("bias")), _stream())
        run_in_arenas(call, ins, {"ACT": Out((M, N // 2), BF16, 16)}, device=DEV)
