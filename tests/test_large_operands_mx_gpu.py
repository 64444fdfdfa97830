"""The MXFP4 GEMMs with an operand across the 2 GiB and 4 GiB byte marks (``-m gpu``; DESIGN.md 5.2: every index of ``gemm_mx*`` is
``size_t`` from the first multiplication on, and these runs are what holds it there; method: tests/bigmem.py).

A is banded: 7 kinds of 256 rows of outlier activations quantised by arcq_mx_quantize_x (tied to tests/mx_reference.py by
tests/test_mx_gpu.py and tests/test_large_operands_quant_gpu.py), repeated down the operand; 1792 rows are 14 of the tile kernel's 128-row
tiles.  The first period of every output is held to the project's reference for its entry point:

  arcq_gemm_mxfp4        fp64 alpha deq(A) deq(B)^T within gamma(M, Kp) * wabs (tests/test_mx_gemm_exact_gpu.py): fp32 element-wise, bf16
                         between the single roundings of the interval's ends
  _silu_mul              bit-equal to F.silu(y[:, 0::2]) * y[:, 1::2] of the plain bf16 result y (tests/test_mx_fused_gpu.py)
  _silu_mul_quantize     byte-equal to arcq_mx_quantize_x of that activation with the identity gather (tests/test_mx_quant_epilogue_gpu.py)
  _rw forms              bit-equal to their namesakes over the whole output (route 2: the tile kernel over the repacked weight)

and every later band must equal its kind's bits (bigmem.check_bands); guards unchanged, no 0xFF fill left."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import bigmem as BM
from tests.test_mx_gemm_exact_gpu import gamma
from tests.test_mx_gpu import deq_torch
from tests.util import outlier_activations, random_perm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PERIOD = BM.PERIOD
ALPHA = 0.75


@pytest.fixture(autouse=True)
def _release():
    yield
    BM.release()


def _lib():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _a_kinds(Kp):
    """7 kinds of a [256, Kp] activation: (codes [7] u8 [256, Kp/2], scale bytes [7] u8 [256, Kp/32]) on the device."""
    from arcquant_amd import agemm
    KE = 64
    KQ = Kp - KE
    idx = random_perm(KQ, 31).to(DEV)
    qs = [agemm.mx_reorder_quantize_x(outlier_activations(BM.BAND, KQ, 800 + k + Kp).to(DEV), idx, KE) for k in range(BM.KINDS)]
    assert qs[0][0].shape == (BM.BAND, Kp // 2)
    return [q for q, _ in qs], [s for _, s in qs]


@functools.lru_cache(maxsize=None)
def _weight(N, Kp):
    from arcquant_amd import agemm
    KE = 64
    KQ = Kp - KE
    w = (torch.randn(N, KQ, generator=torch.Generator().manual_seed(N + Kp)) * 0.05).to(torch.bfloat16).to(DEV)
    return agemm.mx_reorder_quantize_w(w, random_perm(KQ, 31).to(DEV), KE)


def _a(M, Kp):
    q, s = _a_kinds(Kp)
    return BM.banded_rows(q, M), BM.banded_rows(s, M)


def _check(st):
    torch.cuda.synchronize()
    assert st == 0, (st, _lib().arcq_last_error())


def _gemm(A, SFA, B, SFB, D, rw=False):
    M, N, Kp = A.shape[0], D.shape[1], A.shape[1] * 2
    oc = 0 if D.dtype == torch.bfloat16 else 1
    L = _lib()
    if rw:
        _check(L.arcq_gemm_mxfp4_rw(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), D.data_ptr(), M, N, Kp, ALPHA, None, None, None, oc, _stream()))
    else:
        _check(L.arcq_gemm_mxfp4(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), D.data_ptr(), M, N, Kp, ALPHA, None, None, None, oc, None, 0,
                                 _stream()))


def _bf16_key_of_f64(x):
    """Monotone key of the bf16 nearest to the fp64 ``x`` in ONE rounding: fp64 -> fp32 first, and where that lands exactly on a bf16 tie
    that ``x`` itself was not on, one fp32 step back towards ``x`` before the round-to-nearest-even to 16 bits."""
    f = x.float()
    b = f.view(torch.int32)
    tie = (b & 0xFFFF) == 0x8000
    fd = f.double().abs()
    b = b + (tie & (fd < x.abs())).to(torch.int32) - (tie & (fd > x.abs())).to(torch.int32)
    r = ((b.to(torch.int64) & 0xFFFFFFFF) + 0x7FFF + ((b >> 16) & 1)) >> 16
    return torch.where((r & 0x8000) != 0, -(r & 0x7FFF), r & 0x7FFF)


def _bf16_key(t):
    b = t.view(torch.int16).to(torch.int64) & 0xFFFF
    return torch.where((b & 0x8000) != 0, -(b & 0x7FFF), b & 0x7FFF)


def _check_first_period(got, A, SFA, B, SFB, M):
    """gamma(M, Kp) * wabs against fp64, as tests/test_mx_gemm_exact_gpu.py::test_gemm_elementwise."""
    Kp = A.shape[1] * 2
    a, b = deq_torch(A[:PERIOD], SFA[:PERIOD]), deq_torch(B, SFB)
    ref, wabs = ALPHA * (a @ b.T), ALPHA * (a.abs() @ b.abs().T)
    BM.assert_kinds_differ(ref)
    tol = gamma(M, Kp) * wabs
    if got.dtype == torch.float32:
        err = (got.double() - ref).abs()
        print(f"    fp32: max err / (2^-24 wabs) = {float((err / (2.0 ** -24 * wabs + 1e-300)).max()):.3f} against {gamma(M, Kp) * 2 ** 24:.0f}")
        assert bool((err <= tol).all())
    else:
        k, lo, hi = _bf16_key(got), _bf16_key_of_f64(ref - tol), _bf16_key_of_f64(ref + tol)
        assert bool((lo <= hi).all())
        bad = (k < lo) | (k > hi)
        print(f"    bf16: {int(bad.sum())} of {k.numel()} outside the interval")
        assert not bool(bad.any())


def _equal_everywhere(X, Y, what):
    step = 2 * PERIOD
    for r0 in range(0, X.shape[0], step):
        x, y = BM._as_int(X[r0:r0 + step]), BM._as_int(Y[r0:r0 + step])
        if not torch.equal(x, y):
            r, c = BM._first_diff(x, y)
            raise AssertionError(f"{what}: differs first at (row {r0 + r}, column {c}), byte offset {((r0 + r) * X.shape[1] + c) * X.element_size()}")


@pytest.mark.parametrize("M,N,Kp,dtype", [(38 * PERIOD, 32768, 128, torch.bfloat16), (19 * PERIOD, 32768, 128, torch.float32),
                                          (600 * PERIOD, 16, 8192, torch.bfloat16)])
def test_gemm_and_its_rw_form(M, N, Kp, dtype):
    """(68096, 32768, 128) bf16: 4.16 GiB of D.  (34048, 32768, 128) fp32: M N just above 2^30, 4.16 GiB.  (600 * 1792, 16, 8192): 4.1 GiB
    of A codes.  The tile kernel (M > 64); arcq_gemm_mxfp4_rw on the same shape is route 2 and must give the same bits."""
    from arcquant_amd import mx
    L = _lib()
    esz = 2 if dtype == torch.bfloat16 else 4
    a_bytes, d_bytes = M * Kp // 2, M * N * esz
    assert L.arcq_gemm_mxfp4_rw_route(M, N, Kp) == 2 and M > 64
    assert max(a_bytes, d_bytes) > 1 << 32 and (dtype != torch.float32 or M * N > 1 << 30)
    BM.need(a_bytes + 2 * d_bytes + PERIOD * N * 40 + (1 << 30))
    if d_bytes > 1 << 32:
        BM.assert_wrap_visible(BM.BAND * N * esz, d_bytes, "D")
    if a_bytes > 1 << 32:
        BM.assert_wrap_visible(BM.BAND * Kp // 2, a_bytes, "A")
    A, SFA = _a(M, Kp)
    B, SFB = _weight(N, Kp)
    buf, D = BM.guarded((M, N), dtype, DEV)
    _gemm(A, SFA, B, SFB, D)
    _check_first_period(D[:PERIOD], A, SFA, B, SFB, M)
    BM.check_bands(D, buf=buf, what=f"D [{M}, {N}] {dtype}")
    MRW, MRSF = mx.mx_repack_w(B, SFB)
    buf2, D2 = BM.guarded((M, N), dtype, DEV)
    _gemm(A, SFA, MRW, MRSF, D2, rw=True)
    _equal_everywhere(D2, D, "arcq_gemm_mxfp4_rw against arcq_gemm_mxfp4")
    BM.check_guards(buf2, "D of arcq_gemm_mxfp4_rw")


def _act_reference(A, SFA, B, SFB, N):
    """silu(gate) * up of the first period's plain bf16 result (itself within gamma * wabs of fp64)."""
    y = torch.empty((PERIOD, N), dtype=torch.bfloat16, device=DEV)
    _gemm(A[:PERIOD], SFA[:PERIOD], B, SFB, y)
    _check_first_period(y, A, SFA, B, SFB, PERIOD)
    return (F.silu(y[:, 0::2]) * y[:, 1::2]).contiguous()


@pytest.mark.parametrize("rw", [False, True])
def test_silu_mul_act_past_4gib(rw):
    """arcq_gemm_mxfp4_silu_mul / _rw_silu_mul at (68096, 65536, 128): ACT bf16 [M, N / 2] is 4.16 GiB."""
    from arcquant_amd import mx
    M, N, Kp = 38 * PERIOD, 65536, 128
    L = _lib()
    assert M * N > 1 << 32 and L.arcq_gemm_mxfp4_rw_route(M, N, Kp) == 2
    BM.assert_wrap_visible(BM.BAND * N, M * N, "ACT")
    BM.need(M * N + PERIOD * N * 40 + (1 << 30))
    A, SFA = _a(M, Kp)
    B, SFB = _weight(N, Kp)
    want = _act_reference(A, SFA, B, SFB, N)
    BM.assert_kinds_differ(want.float())
    W, SW = mx.mx_repack_w(B, SFB) if rw else (B, SFB)
    buf, ACT = BM.guarded((M, N // 2), torch.bfloat16, DEV)
    fn = L.arcq_gemm_mxfp4_rw_silu_mul if rw else L.arcq_gemm_mxfp4_silu_mul
    _check(fn(A.data_ptr(), W.data_ptr(), SFA.data_ptr(), SW.data_ptr(), ACT.data_ptr(), M, N, Kp, ALPHA, None, None, _stream()))
    assert torch.equal(ACT[:PERIOD].view(torch.int16), want.view(torch.int16)), "first period differs from silu(gate) * up of the plain result"
    BM.check_bands(ACT, buf=buf, what="ACT")


@pytest.mark.parametrize("rw", [False, True])
def test_silu_mul_quantize_qact_past_4gib(rw):
    """arcq_gemm_mxfp4_silu_mul_quantize / _rw_ at (147 * 1792, 65408, 128), KE = 64: N / 2 + KE = 32768 stored columns, 16 KiB of codes
    per row, QACT 4.02 GiB (past both marks) and SFACT 257 MiB."""
    from arcquant_amd import agemm, mx
    M, N, Kp, KE = 147 * PERIOD, 65408, 128, 64
    L = _lib()
    Kp2 = N // 2 + KE
    assert Kp2 % 128 == 0 and M * Kp2 // 2 > 1 << 32 and L.arcq_gemm_mxfp4_rw_route(M, N, Kp) == 2
    BM.assert_wrap_visible(BM.BAND * Kp2 // 2, M * Kp2 // 2, "QACT")
    BM.need(M * Kp2 // 2 + M * Kp2 // 32 + PERIOD * N * 40 + (1 << 30))
    A, SFA = _a(M, Kp)
    B, SFB = _weight(N, Kp)
    act = _act_reference(A, SFA, B, SFB, N)
    wq, ws = agemm.mx_reorder_quantize_x(act, torch.arange(N // 2, dtype=torch.int16, device=DEV), KE)
    assert wq.shape == (PERIOD, Kp2 // 2) and len(torch.unique(ws)) >= 4
    for a_ in range(BM.KINDS):
        for b_ in range(a_ + 1, BM.KINDS):
            assert not torch.equal(wq[a_ * BM.BAND:(a_ + 1) * BM.BAND], wq[b_ * BM.BAND:(b_ + 1) * BM.BAND])
    W, SW = mx.mx_repack_w(B, SFB) if rw else (B, SFB)
    qbuf, Q = BM.guarded((M, Kp2 // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((M, Kp2 // 32), torch.uint8, DEV)
    fn = L.arcq_gemm_mxfp4_rw_silu_mul_quantize if rw else L.arcq_gemm_mxfp4_silu_mul_quantize
    _check(fn(A.data_ptr(), W.data_ptr(), SFA.data_ptr(), SW.data_ptr(), Q.data_ptr(), SF.data_ptr(), M, N, Kp, ALPHA, None, None, KE, _stream()))
    assert torch.equal(Q[:PERIOD], wq), "QACT: the first period differs from arcq_mx_quantize_x of the activation"
    assert torch.equal(SF[:PERIOD], ws), "SFACT: the first period differs"
    BM.check_bands(Q, buf=qbuf, fill_check=False, what="QACT")
    BM.check_bands(SF, buf=sbuf, fill_check=False, what="SFACT")
