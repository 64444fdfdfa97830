"""Operands past the 2 GiB and 4 GiB marks (tests/test_large_operands_*_gpu.py): how they are built and how they are checked.

A kernel that narrows an index to 32 bits, or forms a byte offset in ``int``, is right for every operand the rest of the suite uses
(the largest is about 310 MB) and wrong beyond a mark.  These helpers make such a kernel FAIL, cheaply:

**Banded operands.**  A large operand is ``KINDS`` = 7 independently seeded small operands ("band kinds") of ``BAND`` = 256 rows each,
repeated: band j holds kind j mod 7.  7 x 256 = 1792 rows is a multiple of every tile height of the library (16 .. 256 rows, the
128-row blocks of the swizzled scale layout), so the same kernel sees every period at the same tile positions and must produce the
same BITS for it: no tolerance is involved.  A period's byte length has the odd factor 7, so it divides neither 2^31 nor 2^32: an
address that wraps at either mark lands ``wrap_shift`` bytes into the period -- in a band of another kind (``assert_wrap_visible``
checks this on the CPU for every operand used).  Only the first period needs a reference: it is checked by the caller against the
project's reference for the entry point at the project's existing bound, and ``check_bands`` ties every later band to it.

**Outputs** are views into a larger byte buffer with ``GUARD`` = 2 MiB of 0xA5 before and behind (tests/arena.py: one tile of the
largest operand, the reach of an address that is wrong by up to a tile), pre-filled with 0xFF bytes: NaN as bf16 and fp32.

Everything here takes the device from its arguments, so tests/test_bigmem_selfcheck.py runs it on the CPU.
"""
from __future__ import annotations

import pytest
import torch

GiB = 1 << 30
CAP = 24 * GiB               # no test may need more than this at its peak
HEADROOM = 2 * GiB
GUARD = 2 << 20
GUARD_BYTE, FILL_BYTE = 0xA5, 0xFF
BAND, KINDS = 256, 7
PERIOD = BAND * KINDS        # 1792 rows


def need(nbytes: int, device="cuda:0"):
    """Skip (with the byte counts in the reason) unless ``nbytes`` + 2 GiB of device memory are free."""
    assert nbytes <= CAP, f"a test may need at most {CAP} bytes at its peak, this one asks for {nbytes}"
    free = torch.cuda.mem_get_info(device)[0]
    if free < nbytes + HEADROOM:
        pytest.skip(f"needs {nbytes} + {HEADROOM} bytes of free device memory, {free} are free")


def release():
    """Give cached blocks back between the cases of a file: each case is sized against ``need`` on its own."""
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(-1).view(torch.uint8)


# ---- building ----------------------------------------------------------------------------------------------------------------------
def periodic(period: torch.Tensor, total: int) -> torch.Tensor:
    """``total`` bytes that repeat the 1-D uint8 tensor ``period`` (the last repetition as a prefix), on ``period``'s device."""
    assert period.dtype == torch.uint8 and period.dim() == 1
    P = period.numel()
    out = torch.empty(total, dtype=torch.uint8, device=period.device)
    n = total // P
    if n:
        out[:n * P].view(n, P).copy_(period.unsqueeze(0).expand(n, P))
    out[n * P:].copy_(period[:total - n * P])
    return out


def banded_rows(kinds, rows: int) -> torch.Tensor:
    """``kinds``: KINDS tensors [BAND, ...] of one dtype and shape (already on the device) -> [rows, ...]: band j = kind j mod KINDS."""
    assert len(kinds) == KINDS and all(k.shape == kinds[0].shape and k.shape[0] == BAND and k.is_contiguous() for k in kinds)
    period = torch.cat([_bytes(k) for k in kinds])
    row_bytes = period.numel() // PERIOD
    return periodic(period, rows * row_bytes).view(kinds[0].dtype).view((rows,) + tuple(kinds[0].shape[1:]))


def banded_sf_nvfp4(kinds, rows: int, K: int) -> torch.Tensor:
    """``kinds``: KINDS uint8 tensors, each the swizzled scale buffer of a BAND-row operand (its first two 128-row blocks: 2 x K/64 x 512
    bytes are taken) -> the scale buffer of the banded operand of ``rows`` rows, in the reference's allocation size
    (rows / 128 + 1 blocks).  Bands are whole 128-row blocks, so kind j mod KINDS's bytes are band j's."""
    blk = (K // 64) * 512
    assert BAND % 128 == 0 and all(k.dtype == torch.uint8 and k.numel() >= 2 * blk for k in kinds)
    period = torch.cat([k.reshape(-1)[:2 * blk] for k in kinds])
    return periodic(period, (rows // 128 + 1) * blk)


def guarded(shape, dtype, device="cuda:0"):
    """-> (buf, view): ``view`` is a contiguous [shape] tensor of ``dtype`` inside the uint8 allocation ``buf``, every byte of it 0xFF,
    with GUARD bytes of 0xA5 before and behind."""
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    buf = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=device)
    buf[:GUARD] = GUARD_BYTE
    buf[GUARD:GUARD + n] = FILL_BYTE
    buf[GUARD + n:] = GUARD_BYTE
    view = buf[GUARD:GUARD + n].view(dtype).view(tuple(shape))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + GUARD and view.data_ptr() % 16 == 0
    return buf, view


def check_guards(buf: torch.Tensor, what: str = "output"):
    for side, region, base in (("head", buf[:GUARD], 0), ("tail", buf[-GUARD:], buf.numel() - GUARD)):
        bad = region != GUARD_BYTE
        if bool(bad.any()):
            idx = bad.nonzero().reshape(-1)
            raise AssertionError(f"{what}: {idx.numel()} guard byte(s) on the {side} side changed, first at byte offset "
                                 f"{base + int(idx[0]) - GUARD} relative to the operand")


# ---- the CPU statements a test makes about its operand -------------------------------------------------------------------------------
def wrap_shift(band_bytes: int, mark: int) -> int:
    """Where an address that is wrong by ``mark`` bytes lands, relative to the right one, inside the period of KINDS bands."""
    return mark % (KINDS * band_bytes)


def assert_wrap_visible(band_bytes: int, nbytes: int, what: str):
    """The period of ``what`` (KINDS bands of ``band_bytes``) divides neither mark the operand crosses: a wrapped address lands at another
    offset of the period.  Where a band is a power of two of bytes (every shape but the guard probes) that is a whole number of bands,
    1 .. 6 of them: another KIND, for every byte."""
    crossed = [m for m in (1 << 31, 1 << 32) if nbytes > m]
    assert crossed, f"{what}: {nbytes} bytes cross neither 2^31 nor 2^32"
    for mark in crossed:
        s = wrap_shift(band_bytes, mark)
        assert s != 0, f"{what}: a period of {KINDS * band_bytes} bytes divides {mark}"
        if band_bytes & (band_bytes - 1) == 0 and band_bytes <= mark:
            assert s % band_bytes == 0 and 1 <= s // band_bytes < KINDS, (what, band_bytes, mark, s)


def assert_kinds_differ(ref: torch.Tensor, axis: int = 0, min_distinct: int = 64):
    """``ref``: the reference result of the first period, bands along ``axis``.  The seven kinds differ pairwise, and each holds many
    distinct non-zero values (a banded operand of equal or constant bands would make ``check_bands`` vacuous)."""
    ref = ref.movedim(axis, 0)
    assert ref.shape[0] == PERIOD, ref.shape
    bands = [ref[k * BAND:(k + 1) * BAND] for k in range(KINDS)]
    for a in range(KINDS):
        vals = bands[a][bands[a] != 0]
        assert vals.numel() and torch.unique(vals.reshape(-1)[:1 << 20]).numel() >= min_distinct, f"kind {a}: too few distinct non-zero values"
        for b in range(a + 1, KINDS):
            assert not torch.equal(bands[a], bands[b]), f"kinds {a} and {b} have equal reference results"


# ---- checking ------------------------------------------------------------------------------------------------------------------------
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _as_int(t: torch.Tensor) -> torch.Tensor:
    return t if not t.is_floating_point() else t.view(_INT[t.element_size()])


def _first_diff(a: torch.Tensor, b: torch.Tensor):
    """(row, column) of the first differing element of two equal-shaped integer 2-D tensors."""
    rows = (a != b).any(dim=1).nonzero().reshape(-1)
    r = int(rows[0])
    c = int((a[r] != b[r]).nonzero().reshape(-1)[0])
    return r, c


def check_bands(out: torch.Tensor, rows_per_band: int = BAND, kinds: int = KINDS, *, axis: int = 0, buf: torch.Tensor | None = None,
                fill_check: bool = True, what: str = "output"):
    """``out``: a 2-D result whose bands run along ``axis`` (0: rows; 1: columns, for operands that are large along the weight rows).

    * every band j >= kinds -- the ragged last one as a prefix -- is bit-equal to band j mod kinds of the same output (compared as
      integers on the device, period by period, then band by band to name the first difference);
    * ``buf`` (the allocation of ``guarded``): both guards unchanged;
    * ``fill_check``: no element of the first period is still the 0xFF fill (with the equality above: none anywhere).  Off for byte
      outputs, where 0xFF is a legal value and the caller's reference comparison of the first period does the work.

    Raises AssertionError naming the first differing (row, column) of ``out`` and its byte offset."""
    assert out.dim() == 2
    o = _as_int(out)
    esz = out.element_size()
    n = o.shape[axis]
    period = rows_per_band * kinds
    sel = (lambda a, b: o[a:b]) if axis == 0 else (lambda a, b: o[:, a:b])
    first = sel(0, min(period, n))
    for p0 in range(period, n, period):
        p1 = min(p0 + period, n)
        got, want = sel(p0, p1), (first if p1 - p0 == period else sel(0, p1 - p0))
        if torch.equal(got, want):
            continue
        for b0 in range(p0, p1, rows_per_band):                 # which band, which element
            b1 = min(b0 + rows_per_band, p1)
            g, w = sel(b0, b1), sel(b0 - p0, b1 - p0)
            if torch.equal(g, w):
                continue
            if axis == 0:
                r, c = _first_diff(g, w)
                row, col = b0 + r, c
            else:
                c, r = _first_diff(g.T, w.T)
                row, col = r, b0 + c
            j = b0 // rows_per_band
            raise AssertionError(f"{what}: band {j} differs from band {j % kinds} (its kind) first at (row {row}, column {col}), byte offset "
                                 f"{(row * o.shape[1] + col) * esz} = {hex((row * o.shape[1] + col) * esz)} of {o.numel() * esz}")
    if fill_check:
        assert esz in (2, 4)
        left = first == -1
        if bool(left.any()):
            r, c = _first_diff(left.to(torch.uint8), torch.zeros_like(left, dtype=torch.uint8))
            raise AssertionError(f"{what}: the 0xFF fill survives at (row {r}, column {c}) of the first period, byte offset {(r * o.shape[1] + c) * esz}")
    if buf is not None:
        check_guards(buf, what)
