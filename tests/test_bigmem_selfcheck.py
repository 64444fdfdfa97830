"""tests/bigmem.py checked on the CPU: the banded builders, and that ``check_bands`` FAILS -- naming the row and the byte offset -- for
the faults the large-operand GPU tests exist to catch, modelled at a small mark: a stand-in "kernel" copies row m of a banded input to
row m of the output, once with the row's byte offset formed in full and once narrowed to WRAP bits, as a ``uint32_t`` cast of
``(size_t)m0 * p.N`` (or of ``page`` in ``kv_row``) narrows it at 2^32."""
import pytest
import torch

from tests import bigmem as BM

COLS = 16                       # int16 columns: 32 bytes per row, 8 KiB per band, 56 KiB per period
ROWS = 5 * BM.PERIOD + 77
WRAP = 1 << 17                  # the model's mark: 128 KiB


def _kinds(seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, 30000, (BM.BAND, COLS), generator=g, dtype=torch.int16) for _ in range(BM.KINDS)]


def _run(x, wrap=None, out_rows=None):
    """out[m] = x[m]; with ``wrap`` the destination byte offset of row m is taken modulo ``wrap``."""
    buf, out = BM.guarded((out_rows or x.shape[0], COLS), torch.int16, "cpu")
    per = (wrap // (COLS * 2)) if wrap else x.shape[0]
    for m0 in range(0, x.shape[0], per):         # in store order: later rows overwrite earlier ones
        n = min(per, x.shape[0] - m0)
        out[:n] = x[m0:m0 + n]
    return buf, out


def test_builders_and_a_right_kernel():
    kinds = _kinds()
    x = BM.banded_rows(kinds, ROWS)
    assert x.shape == (ROWS, COLS)
    for j in (0, 6, 7, 8, 20, 34):
        assert torch.equal(x[j * BM.BAND:(j + 1) * BM.BAND], kinds[j % BM.KINDS])
    assert torch.equal(x[35 * BM.BAND:], kinds[0][:77])
    BM.assert_kinds_differ(x[:BM.PERIOD].float())
    buf, out = _run(x)
    BM.check_bands(out, buf=buf)
    BM.check_bands(out.T.contiguous(), axis=1)
    sf = BM.banded_sf_nvfp4([torch.full((3 * 512,), k, dtype=torch.uint8) for k in range(BM.KINDS)], 128 * 17 + 5, 64)
    assert sf.numel() == 18 * 512 and sf[::512].tolist() == [k // 2 % 7 for k in range(18)]


def test_wrap_statement():
    assert BM.wrap_shift(BM.BAND * COLS * 2, WRAP) == 2 * BM.BAND * COLS * 2          # 16 bands mod 7 = 2 bands on
    BM.assert_wrap_visible(256 * 65536, 68096 * 65536, "D of (68096, 32768) bf16")
    with pytest.raises(AssertionError):
        BM.assert_wrap_visible(256 * 65536, 1 << 30, "an operand below both marks")
    assert all((1 << 32) % (BM.KINDS * b) for b in range(1, 1 << 12))          # (7 bands: no period divides a power of two)


def test_a_narrowed_offset_fails_with_row_and_byte_offset():
    """Rows at and past the mark (row 4096 = 128 KiB) are stored over rows 0 ..; rows 4096 .. keep the fill.  The first band that can be
    compared, band 7 (rows 1792 ..), then holds x[5888 ..] = band 23, kind 2, and band 0 holds x[8192 ..] = band 32, kind 4: the report
    names the band's first element."""
    x = BM.banded_rows(_kinds(), ROWS)
    buf, out = _run(x, wrap=WRAP)
    assert torch.equal(out[1792], x[5888]) and torch.equal(out[0], x[8192]) and out[1792, 0] != out[0, 0]
    with pytest.raises(AssertionError, match=r"band 7 differs from band 0 .* \(row 1792, column 0\), byte offset 57344 = 0xe000 of 289184"):
        BM.check_bands(out, buf=buf)
    # with the wrapped rows put right, what is left is the fill in the rows past the mark: named as well
    out[:WRAP // 32] = x[:WRAP // 32]
    with pytest.raises(AssertionError, match=r"band 16 differs from band 2 .* \(row 4096, column 0\), byte offset 131072 "):
        BM.check_bands(out, buf=buf)


def test_surviving_fill_and_touched_guard_fail():
    x = BM.banded_rows(_kinds(), ROWS)
    buf, out = _run(x)
    out[BM.PERIOD + 300, 5] = -1                                  # a lost store in a later band
    with pytest.raises(AssertionError, match=r"band 8 differs from band 1 .* \(row 2092, column 5\), byte offset 66954 "):
        BM.check_bands(out, buf=buf)
    buf, out = _run(x)
    out[: 6 * BM.PERIOD:BM.PERIOD][:, 3] = -1                     # the same element lost in every period
    with pytest.raises(AssertionError, match="0xFF fill survives at .row 0, column 3"):
        BM.check_bands(out, buf=buf)
    buf, out = _run(x)
    buf[BM.GUARD - 2] = 0
    with pytest.raises(AssertionError, match="guard byte.*head"):
        BM.check_bands(out, buf=buf)
    buf, out = _run(x)
    out.T[2, BM.PERIOD * 2 + 9] = 7
    with pytest.raises(AssertionError, match=r"\(row 2, column 3593\)"):
        BM.check_bands(out.T.contiguous(), axis=1)
