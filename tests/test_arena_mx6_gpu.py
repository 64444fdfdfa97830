"""Arena test of the MXFP6 C-ABI (``-m gpu``): arcq_mx6_quantize_x / _w (quantize_mx6.hip) and arcq_gemm_mxfp6 (gemm_mx6.hip: mx6_small_kernel
for M <= 64, mx6_tile_kernel above), every operand inside a poisoned arena (tests/arena.py) at the alignment arcq.h promises and no more.
Bit-exact against the same call on tight allocations.  MXFP6 buffers have no don't-care bytes; what this pins is the 8-byte word copies of
the quantisers at both ends of a row, the `min(., M - 1)` / `min(., N - 1)` clamps, the clamped K steps and the ragged last tile."""
import pytest
import torch

from tests.arena import In, Out, run_in_arenas
from tests.test_arena_mx_gpu import _L, _bf16, _epi, _gen, _p, _packed, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8, I16 = torch.bfloat16, torch.float32, torch.uint8, torch.int16


@pytest.mark.parametrize("M", [17, 130])          # two row groups of the small kernel with 15 clamped rows; two tiles, the second ragged
def test_mx6_entry_points(M):
    L, g = _L(), _gen(M)
    for KQ, KE in ((64, 0), (320, 64)):                                          # K = 64 and 384: padding blocks / none
        Kp = int(L.arcq_mx_k_padded(KQ + KE))
        assert int(L.arcq_mx6_code_bytes(M, KQ + KE)) == M * 3 * Kp // 4
        ins = {"X": In(_bf16((M, KQ), g, 3.0), 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}
        for fn in (L.arcq_mx6_quantize_x, L.arcq_mx6_quantize_w):
            def call(o):
                return fn(_p(o["X"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), M, KQ, KE, _stream())
            run_in_arenas(call, ins, {"Q": Out((M, 3 * Kp // 4), U8, 16), "SF": Out((M, Kp // 32), U8, 4)}, device=DEV)
    N, K = 144, 1152                                                              # N % 64 != 0; 9 K steps over the small kernel's 8 waves
    for fmt in (0, 1):
        a6, sfa = In(torch.randint(0, 256, (M, 3 * K // 4), generator=g, device=DEV, dtype=U8), 16), _packed(M, K, g)[1]
        b4, sfb = _packed(N, K, g)
        b = b4 if fmt else In(torch.randint(0, 256, (N, 3 * K // 4), generator=g, device=DEV, dtype=U8), 16)
        for out_dtype, alias in ((F32, False), (BF16, True)):
            ins = {"A": a6, "B": b, "SFA": sfa, "SFB": sfb, **_epi(M, N, g, residual=not alias)}

            def call(o):
                res = o["D"] if alias else o["residual"]
                return L.arcq_gemm_mxfp6(_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["D"]), M, N, K, fmt, 1e-4, _p(o["alpha_dev"]),
                                         _p(o["bias"]), _p(res), 0 if out_dtype is BF16 else 1, _stream())
            run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16, init=_bf16((M, N), g) if alias else None)}, device=DEV)
