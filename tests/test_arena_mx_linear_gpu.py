"""Arena tests of the MXFP4 fused decode linears (``-m gpu``; gemm_mx_linear_rw.hip): arcq_mx_linear_rmsnorm_repacked,
arcq_mx_linear_rmsnorm_silu_repacked and arcq_mx_linear_quantize_repacked with every operand inside a poisoned arena (tests/arena.py),
bit-exact against the same call on tight allocations.  MRSF's padding bytes (the steps of a partial last round, include/arcq.h) are the
one don't-care region: they hold the poison in the arena copy.  What the cases pin: X read for exactly M rows (rows M .. 15 of the A
fragment come from the image, clamped), the norm weight and reorder_index for exactly KQ entries, the K steps of the one-round-ahead
weight loads clamped to the last step and the last row block, the MRSF dword of a partial round and the row guards of the stores."""
import pytest
import torch

from arcquant_amd import agemm, mx
from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
# (M, N, KQ, KE): one row, one row block, 17 steps (a partial round, two padding blocks); five rows (an idle half workgroup in the last
# pass), three row blocks, 33 steps (a second round that is nearly all padding); sixteen rows
RMS_SHAPES = [(1, 16, 2048, 64), (5, 48, 4096, 128), (16, 32, 2048, 0)]
PLAIN_SHAPES = RMS_SHAPES + [(3, 16, 64, 64)]            # one step: seven idle waves


def _L():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(BF16)


def _operands(M, N, KQ, KE, g, rms):
    K = mx.mx_k_padded(KQ + KE)
    qw = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV, dtype=U8)
    sfw = torch.randint(120, 128, (N, K // 32), generator=g, device=DEV, dtype=U8)
    mrw, mrsf = agemm.mx_repack_w(qw, sfw)
    T, R = K // 128, -(-(K // 128) // 32)
    pad = torch.ones((N // 16, R, 8, 64, 4), dtype=torch.bool)
    t = torch.arange(T)
    pad[:, t // 32, t % 8, :, (t // 8) % 4] = False
    assert int(pad.sum()) == (N // 16) * (R * 32 - T) * 64
    idx = torch.randperm(KQ, generator=torch.Generator().manual_seed(KQ + KE)).to(torch.int16).to(DEV)
    ins = {"X": In(_bf16((M, KQ), g, 3.0), 16), "idx": In(idx, 16), "MRW": In(mrw, 16),
           "MRSF": In(mrsf, 4, dont_care=pad.reshape(-1) if pad.any() else None)}
    if rms:
        ins["Wn"] = In(1 + _bf16((KQ,), g, 0.2), 16)
    return ins


def _epi(M, N, g, residual=True):
    ins = {"bias": In(_bf16((N,), g), 2), "alpha_dev": In(torch.tensor([0.5], dtype=F32, device=DEV), 4)}       # bias, residual: 2-byte aligned (arcq.h)
    if residual:
        ins["residual"] = In(_bf16((M, N), g), 2)
    return ins


def _plain_epilogues(call_of, base, M, N, g):
    """bf16 plain, fp32 and bf16 with bias + residual + alpha_dev, and the residual aliasing D."""
    for out_dtype, epi, alias in ((BF16, False, False), (F32, True, False), (BF16, True, False), (BF16, True, True)):
        ins = dict(base)
        if epi:
            ins.update(_epi(M, N, g, residual=not alias))
        run_in_arenas(call_of(0 if out_dtype is BF16 else 1, alias), ins,
                      {"D": Out((M, N), out_dtype, 16, init=_bf16((M, N), g) if alias else None)}, device=DEV)


@pytest.mark.parametrize("M,N,KQ,KE", RMS_SHAPES)
def test_mx_linear_rmsnorm_repacked(M, N, KQ, KE):
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + KQ + KE)

    def call_of(oc, alias):
        def call(o):
            res = o["D"] if alias else o.get("residual")
            return L.arcq_mx_linear_rmsnorm_repacked(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["MRW"]), _p(o["MRSF"]), _p(o["D"]), M, N, KQ, KE,
                                                     0.01, _p(o.get("alpha_dev")), _p(o.get("bias")), _p(res), oc, _stream())
        return call
    _plain_epilogues(call_of, _operands(M, N, KQ, KE, g, True), M, N, g)


@pytest.mark.parametrize("M,N,KQ,KE", PLAIN_SHAPES)
def test_mx_linear_quantize_repacked(M, N, KQ, KE):
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + KQ + KE + 1)

    def call_of(oc, alias):
        def call(o):
            res = o["D"] if alias else o.get("residual")
            return L.arcq_mx_linear_quantize_repacked(_p(o["X"]), _p(o["idx"]), _p(o["MRW"]), _p(o["MRSF"]), _p(o["D"]), M, N, KQ, KE, 0.01,
                                                      _p(o.get("alpha_dev")), _p(o.get("bias")), _p(res), oc, _stream())
        return call
    _plain_epilogues(call_of, _operands(M, N, KQ, KE, g, False), M, N, g)


@pytest.mark.parametrize("M,N,KQ,KE", RMS_SHAPES)
def test_mx_linear_rmsnorm_silu_repacked(M, N, KQ, KE):
    """ACT = bf16 [M, N/2], with and without bias."""
    L, g = _L(), torch.Generator(device=DEV).manual_seed(M + N + KQ + KE + 2)
    base = _operands(M, N, KQ, KE, g, True)
    for bias in (False, True):
        ins = dict(base)
        if bias:
            ins.update(_epi(M, N, g, residual=False))

        def call(o):
            return L.arcq_mx_linear_rmsnorm_silu_repacked(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["MRW"]), _p(o["MRSF"]), _p(o["ACT"]), M, N,
                                                          KQ, KE, 0.004, _p(o.get("alpha_dev")), _p(o.get("bias")), _stream())
        run_in_arenas(call, ins, {"ACT": Out((M, N // 2), BF16, 16)}, device=DEV)
