"""The row quantisers with an input past the 4 GiB mark (``-m gpu``; DESIGN.md 5.2: every row offset is ``(size_t)row * ld`` and
``sf_offset`` is int64, which nothing but these runs holds in place).

Shape: KQ = 8192, KE = 64, rows = 150 * 1792: 4.1 GiB of bf16 input, banded (tests/bigmem.py: 7 kinds of 256 rows).  The codes and
scale bytes of the first period must equal the oracle's (oracle/ for NVFP4, tests/mx_reference.py for MXFP4) byte for byte, and every
later band must equal its kind -- rows for the codes and the MXFP4 scale rows, whole 128-row blocks for the swizzled NVFP4 scales.
Outputs lie between 0xA5 guards and start as 0xFF.

The fused MXFP4 sources (RMSNorm; SiLU * up in both layouts, where the same 8192 columns are gate | up of KQ = 4096) are held to
tests/mx_fused_reference.py and to tests/mx_reference.py on torch's silu(gate) * up.

The dynamic quantisers take the same input with ONE larger magnitude in the LAST row, past the 4 GiB mark: ``scale_out`` must be that
value / 2688 (so the abs-max pass reads the whole input; the ``_slots`` entries are handed it as their abs-max word), and the bytes follow
from that scale: the first period equals the oracle on x / scale as torch divides, and the banding breaks in the last row alone.

One case, arcq_quantize_x at rows = 600 * 1792, takes the output CODES past 4 GiB (input 16.4 GiB)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as O
from tests import bigmem as BM
from tests import mx_reference as R
from tests.util import bits, outlier_activations, random_perm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KQ, KE = 8192, 64
K = KQ + KE
ROWS = 150 * BM.PERIOD
PERIOD = BM.PERIOD


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
def _kinds(role):
    """The 7 band kinds [256, KQ] bf16 (CPU) and the permutation."""
    if role == "x":
        kinds = [outlier_activations(BM.BAND, KQ, 600 + k) for k in range(BM.KINDS)]
    else:
        kinds = [(torch.rand(BM.BAND, KQ, generator=torch.Generator().manual_seed(700 + k)) * 3 - 1.0).to(torch.bfloat16) for k in range(BM.KINDS)]
    return kinds, random_perm(KQ, 99)


def _input(role):
    kinds, idx = _kinds(role)
    nbytes = ROWS * KQ * 2
    assert nbytes > 1 << 32
    BM.assert_wrap_visible(BM.BAND * KQ * 2, nbytes, "X")
    BM.need(nbytes + ROWS * K + (2 << 30))
    X = BM.banded_rows([k.to(DEV) for k in kinds], ROWS)
    assert X.shape == (ROWS, KQ) and X.dtype == torch.bfloat16
    return X, torch.cat(kinds), idx


def _differ(codes):
    """Vacuity: the seven kinds' reference codes differ pairwise and hold many distinct bytes."""
    bands = [codes[k * BM.BAND:(k + 1) * BM.BAND] for k in range(BM.KINDS)]
    assert all(len(np.unique(b)) >= 64 for b in bands)
    assert all(not np.array_equal(bands[a], bands[b]) for a in range(BM.KINDS) for b in range(a + 1, BM.KINDS))


def _same(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    if not torch.equal(got, want):
        r, c = BM._first_diff(got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1))
        raise AssertionError(f"{what}: the first period differs from the reference first at (row {r}, byte {c})")


@pytest.mark.parametrize("fn", ["arcq_quantize_x", "arcq_quantize_w", "arcq_rmsnorm_quantize_x"])
def test_nvfp4_quantisers_input_past_4gib(fn):
    role = "w" if fn.endswith("_w") else "x"
    X, first, idx = _input(role)
    L = _lib()
    wn = (torch.rand(KQ, generator=torch.Generator().manual_seed(5)) + 0.5).to(torch.bfloat16)
    if fn == "arcq_quantize_x":
        wq, wsf = O.quantize_x(bits(first), idx.numpy(), KE, O.G16, sf_fill=0)
    elif fn == "arcq_quantize_w":
        wq, wsf = O.quantize_w(bits(first), idx.numpy(), KE, O.G16, sf_fill=0)
    else:
        wq, wsf = O.rmsnorm_quantize_x(bits(first), bits(wn), 1e-6, idx.numpy(), KE, O.G16, sf_fill=0)
    _differ(wq)
    blk = (K // 64) * 512
    nblk = ROWS // 128
    qbuf, Q = BM.guarded((ROWS, K // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((int(L.arcq_sf_alloc_bytes(ROWS, K)),), torch.uint8, DEV)
    I, W = idx.to(DEV), wn.to(DEV)
    if fn == "arcq_rmsnorm_quantize_x":
        st = L.arcq_rmsnorm_quantize_x(X.data_ptr(), W.data_ptr(), 1e-6, I.data_ptr(), Q.data_ptr(), SF.data_ptr(), ROWS, KQ, KE, 0, _stream())
    else:
        st = getattr(L, fn)(X.data_ptr(), I.data_ptr(), Q.data_ptr(), SF.data_ptr(), ROWS, KQ, KE, 0, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _same(Q[:PERIOD], wq, f"{fn}: codes")
    _same(SF[:14 * blk].view(14, blk), wsf[:14 * blk].reshape(14, blk), f"{fn}: scale bytes (128-row blocks)")
    BM.check_bands(Q, buf=qbuf, fill_check=False, what=f"{fn}: codes")
    BM.check_bands(SF[:nblk * blk].view(nblk, blk), rows_per_band=2, buf=sbuf, fill_check=False, what=f"{fn}: scale blocks")
    assert bool((SF[nblk * blk:] == BM.FILL_BYTE).all()), "the block behind the last row's was written"


@pytest.mark.parametrize("fn", ["arcq_mx_quantize_x", "arcq_mx_quantize_w"])
def test_mxfp4_quantisers_input_past_4gib(fn):
    role = "w" if fn.endswith("_w") else "x"
    X, first, idx = _input(role)
    L = _lib()
    wq, wsf = (R.quantize_w if role == "w" else R.quantize_x)(first.float().numpy(), idx.numpy(), KE)
    _differ(wq)
    Kp = R.k_padded(K)
    qbuf, Q = BM.guarded((ROWS, Kp // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((ROWS, Kp // 32), torch.uint8, DEV)
    I = idx.to(DEV)
    st = getattr(L, fn)(X.data_ptr(), I.data_ptr(), Q.data_ptr(), SF.data_ptr(), ROWS, KQ, KE, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _same(Q[:PERIOD], wq, f"{fn}: codes")
    _same(SF[:PERIOD], wsf, f"{fn}: scale bytes")
    BM.check_bands(Q, buf=qbuf, fill_check=False, what=f"{fn}: codes")
    BM.check_bands(SF, buf=sbuf, fill_check=False, what=f"{fn}: scale bytes")


def test_nvfp4_quantiser_codes_past_4gib():
    """arcq_quantize_x at rows = 600 * 1792: 4.1 GiB of codes (and 16.4 GiB of input, 0.5 GiB of scale bytes): the store offsets
    (size_t)row * (K >> 1) and sf_offset(row, p, K) beyond 2^32."""
    rows = 600 * PERIOD
    kinds, idx = _kinds("x")
    q_bytes = rows * K // 2
    assert q_bytes > 1 << 32 and rows * KQ * 2 > 1 << 34
    BM.assert_wrap_visible(BM.BAND * K // 2, q_bytes, "QX")
    BM.assert_wrap_visible(BM.BAND * KQ * 2, rows * KQ * 2, "X")
    L = _lib()
    sf_bytes = int(L.arcq_sf_alloc_bytes(rows, K))
    BM.need(rows * KQ * 2 + q_bytes + sf_bytes + 4 * BM.GUARD)
    X = BM.banded_rows([k.to(DEV) for k in kinds], rows)
    wq, wsf = O.quantize_x(bits(torch.cat(kinds)), idx.numpy(), KE, O.G16, sf_fill=0)
    _differ(wq)
    blk, nblk = (K // 64) * 512, rows // 128
    qbuf, Q = BM.guarded((rows, K // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((sf_bytes,), torch.uint8, DEV)
    I = idx.to(DEV)
    st = L.arcq_quantize_x(X.data_ptr(), I.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, 0, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _same(Q[:PERIOD], wq, "codes")
    _same(SF[:14 * blk].view(14, blk), wsf[:14 * blk].reshape(14, blk), "scale bytes")
    BM.check_bands(Q, buf=qbuf, fill_check=False, what="arcq_quantize_x: codes past 4 GiB")
    BM.check_bands(SF[:nblk * blk].view(nblk, blk), rows_per_band=2, buf=sbuf, fill_check=False, what="arcq_quantize_x: scale blocks")


# ---- the fused MXFP4 sources ----------------------------------------------------------------------------------------------------------
def test_mxfp4_rmsnorm_quantiser_input_past_4gib():
    from tests import mx_fused_reference as FR
    X, first, idx = _input("x")
    L = _lib()
    wn = (torch.rand(KQ, generator=torch.Generator().manual_seed(6)) * 1.5 + 0.25).to(torch.bfloat16)
    wq, wsf = FR.rmsnorm_quantize_x(bits(first), bits(wn), 1e-6, idx.numpy().astype(np.int64), KE)
    _differ(wq)
    Kp = R.k_padded(K)
    qbuf, Q = BM.guarded((ROWS, Kp // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((ROWS, Kp // 32), torch.uint8, DEV)
    I, W = idx.to(DEV), wn.to(DEV)
    st = L.arcq_mx_rmsnorm_quantize_x(X.data_ptr(), W.data_ptr(), 1e-6, I.data_ptr(), Q.data_ptr(), SF.data_ptr(), ROWS, KQ, KE, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _same(Q[:PERIOD], wq, "arcq_mx_rmsnorm_quantize_x: codes")
    _same(SF[:PERIOD], wsf, "arcq_mx_rmsnorm_quantize_x: scale bytes")
    BM.check_bands(Q, buf=qbuf, fill_check=False, what="arcq_mx_rmsnorm_quantize_x: codes")
    BM.check_bands(SF, buf=sbuf, fill_check=False, what="arcq_mx_rmsnorm_quantize_x: scale bytes")


KQ2 = KQ // 2                    # the SiLU * up sources read the same 8192 columns as gate | up of KQ2 channels
K2 = KQ2 + KE


def _act(GU, layout):
    """silu(gate) * up of [rows, 2 KQ2] bf16 as torch computes it (layout 0: halves, 1: pairs)."""
    g, u = (GU[:, :KQ2], GU[:, KQ2:]) if layout == 0 else (GU[:, 0::2], GU[:, 1::2])
    return (F.silu(g) * u).contiguous()


@pytest.mark.parametrize("layout", [0, 1])
def test_mxfp4_silu_mul_quantiser_input_past_4gib(layout):
    X, first, _ = _input("x")
    L = _lib()
    idx = random_perm(KQ2, 98)
    act = _act(first.to(DEV), layout)
    wq, wsf = R.quantize_x(act.float().cpu().numpy(), idx.numpy().astype(np.int64), KE)
    _differ(wq)
    Kp = R.k_padded(K2)
    qbuf, Q = BM.guarded((ROWS, Kp // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((ROWS, Kp // 32), torch.uint8, DEV)
    I = idx.to(DEV)
    st = L.arcq_mx_silu_mul_quantize_x(X.data_ptr(), I.data_ptr(), Q.data_ptr(), SF.data_ptr(), ROWS, KQ2, KE, layout, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    _same(Q[:PERIOD], wq, "arcq_mx_silu_mul_quantize_x: codes")
    _same(SF[:PERIOD], wsf, "arcq_mx_silu_mul_quantize_x: scale bytes")
    BM.check_bands(Q, buf=qbuf, fill_check=False, what="arcq_mx_silu_mul_quantize_x: codes")
    BM.check_bands(SF, buf=sbuf, fill_check=False, what="arcq_mx_silu_mul_quantize_x: scale bytes")


# ---- the dynamic quantisers: the maximum sits in the last row --------------------------------------------------------------------------
DYNAMIC = [("arcq_quantize_x_dyn", None), ("arcq_quantize_x_dyn_slots", None), ("arcq_silu_mul_quantize_x_dyn", 0), ("arcq_silu_mul_quantize_x_dyn", 1),
           ("arcq_silu_mul_quantize_x_dyn_slots", 0), ("arcq_silu_mul_quantize_x_dyn_slots", 1)]


@pytest.mark.parametrize("fn,layout", DYNAMIC)
def test_dynamic_quantisers_find_the_maximum_past_4gib(fn, layout):
    X, first, _ = _input("x")
    L = _lib()
    silu, slots_entry = layout is not None, fn.endswith("_slots")
    kq = KQ2 if silu else KQ
    k = kq + KE
    idx = random_perm(kq, 97)
    assert (ROWS - 1) * KQ * 2 > 1 << 32
    # one magnitude above every other, in the last row: 3008 (plain; the recipe stays within 64), or gate 1024 and up -2048 (SiLU * up:
    # silu(1024) = 1024 in bf16, the product 2^21, above 64 * 64)
    if not silu:
        X[ROWS - 1, 5] = -3008.0
    else:
        X[ROWS - 1, 0] = 1024.0
        X[ROWS - 1, KQ2 if layout == 0 else 1] = -2048.0
    source = (lambda t: _act(t, layout)) if silu else (lambda t: t)
    first_src, last_src = source(first.to(DEV)), source(X[ROWS - 1:])
    amax = torch.maximum(first_src.abs().max(), last_src.abs().max())
    assert float(amax) == (2.0 ** 21 if silu else 3008.0) and float(first_src.abs().max()) < float(amax)
    # the reference's wrapper (tests/test_gpu_parity.py::test_dynamic_quantizer_equals_torch_prescale_pipeline): scale = max|x| / 2688 and
    # x / scale as torch computes them on the device, then the static quantiser -- here the oracle's
    scale = amax.float() / (448.0 * 6.0)
    wq, wsf = O.quantize_x(bits((first_src / scale).contiguous()), idx.numpy(), KE, O.G16, sf_fill=0)
    _differ(wq)
    blk, nblk = (k // 64) * 512, ROWS // 128
    qbuf, Q = BM.guarded((ROWS, k // 2), torch.uint8, DEV)
    sbuf, SF = BM.guarded((int(L.arcq_sf_alloc_bytes(ROWS, k)),), torch.uint8, DEV)
    I = idx.to(DEV)
    scale_out = torch.full((1,), float("nan"), device=DEV)
    if slots_entry:         # the abs-max words a producing kernel would leave: bf16 magnitude bits, the maximum in the last of four
        word = int(amax.view(torch.int16)) & 0x7FFF
        dyn = torch.tensor([0, word // 2, 1, word], dtype=torch.int32, device=DEV)
        extra = (dyn.data_ptr(), 4)
    else:
        dyn = torch.full((1024,), 0xFF, dtype=torch.uint8, device=DEV)
        extra = (dyn.data_ptr(),)
    tail = (0,) if not silu else (0, layout)
    st = getattr(L, fn)(X.data_ptr(), I.data_ptr(), Q.data_ptr(), SF.data_ptr(), scale_out.data_ptr(), *extra, ROWS, kq, KE, *tail, _stream())
    torch.cuda.synchronize()
    assert st == 0, (st, L.arcq_last_error())
    assert float(scale_out) == float(scale), (float(scale_out), float(scale))
    _same(Q[:PERIOD], wq, f"{fn}: codes")
    _same(SF[:14 * blk].view(14, blk), wsf[:14 * blk].reshape(14, blk), f"{fn}: scale bytes")
    # the last row differs from its kind (it holds the maximum); everything in front of it, and of its 128-row block, is banded
    assert not torch.equal(Q[ROWS - 1], Q[PERIOD - 1])
    BM.check_bands(Q[:ROWS - 1], buf=qbuf, fill_check=False, what=f"{fn}: codes")
    BM.check_bands(SF[:(nblk - 1) * blk].view(nblk - 1, blk), rows_per_band=2, buf=sbuf, fill_check=False, what=f"{fn}: scale blocks")
