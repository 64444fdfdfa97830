"""CPU checks of tests/mx6_reference.py, the numpy statement of MXFP6-ARC every GPU test of the format compares with: the block rule at
its edges, the six-bit packing and the exact residual."""
import numpy as np
import pytest

from tests import mx6_reference as R6
from tests.mx_reference import bf16_bits_to_f32, bf16_round


@pytest.mark.parametrize("name", list(R6.EDGE_BLOCKS))
def test_edge_blocks(name):
    bits, want_scale, want_codes = R6.EDGE_BLOCKS[name]
    v = bf16_bits_to_f32(bits).astype(np.float64)
    codes, sc, res = R6.quantize_blocks(v[None])
    assert int(sc[0]) == want_scale
    e = want_scale - 127
    amax = np.abs(v).max()
    assert amax <= 28 * 2.0 ** e and (amax == 0 or e == -127 or amax > 28 * 2.0 ** (e - 1)), "not the smallest exponent"
    if want_codes is not None:
        assert np.array_equal(codes[0], want_codes)
    # the code is a nearest one, the residual is what is left and is a bf16
    deq = np.ldexp(R6.e3m2_value(codes[0]), e)
    assert np.all(np.abs(v - deq) <= np.abs(v[:, None] - np.ldexp(np.r_[R6.E3M2, -R6.E3M2], e)[None, :]).min(axis=1))
    assert np.array_equal(np.signbit(deq), np.signbit(v)) and np.array_equal(res[0], v - deq)
    assert np.array_equal(bf16_round(res[0].astype(np.float32)).astype(np.float64), res[0])
    q = R6.pack6(codes)
    assert q.shape == (1, 24) and np.array_equal(R6.unpack6(q), codes)


def test_exponent_clamps_and_bit_layout():
    assert list(R6.block_exponent([0.0, 28.0, 28.0 * (1 + 2.0 ** -7), 2.0 ** -140, 2.0 ** 140, 28 * 2.0 ** 127, 28 * 2.0 ** -127])) == [0, 0, 1, -127, 127, 127, -127]
    assert R6.E3M2[1] == 0.0625 and R6.E3M2[4] == 0.25 and R6.E3M2[31] == 28 and np.all(np.diff(R6.E3M2) > 0)
    codes = np.zeros(32, np.uint8)
    codes[[0, 5, 31]] = [0x3F, 0x21, 0x2A]          # element i occupies bits [6 i, 6 i + 6) of the 192-bit little-endian string
    assert int.from_bytes(R6.pack6(codes).tobytes(), "little") == 0x3F | (0x21 << 30) | (0x2A << 186)


@pytest.mark.parametrize("is_x", [True, False])
def test_augmented_k(is_x):
    rng = np.random.default_rng(3)
    KQ, KE = 128, 64                                                           # K = 192, Kp = 256: blocks 0..3, tail copies 4..5, padding 6..7
    idx = rng.permutation(KQ)
    x = np.stack([bf16_bits_to_f32(R6.edge_row(KQ, idx)), bf16_round(rng.standard_normal(KQ).astype(np.float32) * 3)])
    Q, SF = (R6.quantize_x if is_x else R6.quantize_w)(x, idx, KE)
    assert Q.shape == (2, 192) and SF.shape == (2, 8)
    d, xr = R6.dequantize(Q, SF), x[:, idx].astype(np.float64)
    assert np.all(SF[:, 6:] == 127) and np.all(Q[:, 144:] == 0) and np.all(d[:, 192:] == 0)
    if is_x:        # the residual block brings every element at least as close as the primary code alone (0 is a code)
        assert np.all(np.abs(d[:, 64:128] + d[:, 128:192] - xr[:, 64:]) <= np.abs(d[:, 64:128] - xr[:, 64:]))
        assert np.any(d[:, 128:192] != 0)
    else:
        assert np.array_equal(d[:, 128:192], d[:, 64:128]) and np.array_equal(Q[:, 96:144], Q[:, 48:96])
