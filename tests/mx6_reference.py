"""numpy restatement of MXFP6-ARC (include/arcq.h "MXFP6-ARC"): the e3m2 element, the block rule for a maximum of 28, the
six-bit packing, the quantisers and an fp64 dequantisation.  The augmented K (reordered row, residual or copy of the outlier tail, padding)
is tests/mx_reference.py's; what differs from quantize_mxfp6_tensor of the reference is what differs there for MXFP4: the exponent is exact
(frexp) instead of ceil(log2(x + 1e-9)), and ties go to the even code instead of argmin's first."""
from __future__ import annotations

import numpy as np

from tests.mx_reference import PAD_SCALE, bf16_round, k_padded

# magnitude codes 0..31: subnormals 0.0625 * m, then 2^(E - 3) * (1 + m / 4) for E = 1..7; the maximum is 28
E3M2 = np.array([m * 0.0625 for m in range(4)] + [2.0 ** (E - 3) * (1 + m / 4) for E in range(1, 8) for m in range(4)])
E3M2_MAX = 28.0


def block_exponent(amax: np.ndarray) -> np.ndarray:
    """Smallest integer e with amax <= 28 * 2^e, clamped to [-127, 127]; 0 where amax == 0.  Exact (frexp, no log)."""
    amax = np.asarray(amax, dtype=np.float64)
    f, F = np.frexp(amax)                       # amax = f * 2^F, f in [0.5, 1); 28 = 0.875 * 2^5
    e = np.clip(np.where(f <= 0.875, F - 5, F - 4), -127, 127)
    return np.where(amax == 0, 0, e).astype(np.int64)


def e3m2_rne(y: np.ndarray) -> np.ndarray:
    """|y| <= 28 -> 6-bit code, round to nearest, ties to the even code, sign of zero kept."""
    a = np.abs(y)
    lo = np.clip(np.searchsorted(E3M2, a, side="right") - 1, 0, 30)
    hi = lo + 1
    dlo, dhi = a - E3M2[lo], E3M2[hi] - a
    c = np.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo)
    return (c | np.where(np.signbit(y), 32, 0)).astype(np.uint8)


def e3m2_value(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c).astype(np.int64)
    v = E3M2[c & 31]
    return np.where(c & 32, -v, v)


def quantize_blocks(v: np.ndarray):
    """v [..., 32] (exact values) -> (codes uint8 [..., 32], scale bytes uint8 [...], residual fp64 [..., 32])."""
    v = np.asarray(v, dtype=np.float64)
    e = block_exponent(np.abs(v).max(axis=-1))
    y = np.ldexp(v, -e[..., None])
    assert np.all(np.abs(y) <= E3M2_MAX), "a code would saturate"
    codes = e3m2_rne(y)
    return codes, (e + 127).astype(np.uint8), v - np.ldexp(e3m2_value(codes), e[..., None])


def pack6(codes: np.ndarray) -> np.ndarray:
    """codes [..., n] (n % 4 == 0) -> bytes [..., 3 n / 4]: element i in bits [6 i, 6 i + 6) of the little-endian bit string."""
    bits = (codes[..., None].astype(np.uint8) >> np.arange(6, dtype=np.uint8)) & 1
    return np.packbits(bits.reshape(codes.shape[:-1] + (-1,)), axis=-1, bitorder="little")


def unpack6(q: np.ndarray) -> np.ndarray:
    bits = np.unpackbits(np.asarray(q, dtype=np.uint8), axis=-1, bitorder="little").reshape(q.shape[:-1] + (-1, 6))
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def _quantize(x: np.ndarray, idx: np.ndarray, KE: int, is_x: bool):
    """x: [rows, KQ] float32 values of bf16 inputs.  Returns (Q [rows, 3 Kp / 4], SF [rows, Kp / 32])."""
    x = np.asarray(x, dtype=np.float32)
    rows, KQ = x.shape
    assert KQ % 64 == 0 and KE % 64 == 0 and 0 <= KE <= KQ
    K, B, P = KQ + KE, KQ // 32, (KQ - KE) // 32
    Kp = k_padded(K)
    codes, sc, res = quantize_blocks(x[:, np.asarray(idx, dtype=np.int64)].astype(np.float64).reshape(rows, B, 32))
    allc = np.zeros((rows, Kp // 32, 32), dtype=np.uint8)
    alls = np.full((rows, Kp // 32), PAD_SCALE, dtype=np.uint8)
    allc[:, :B], alls[:, :B] = codes, sc
    if KE and is_x:
        r = res[:, P:]
        assert np.array_equal(bf16_round(r.astype(np.float32)).astype(np.float64), r), "residual not exact in bf16"
        allc[:, B: K // 32], alls[:, B: K // 32], _ = quantize_blocks(r)
    elif KE:
        allc[:, B: K // 32], alls[:, B: K // 32] = codes[:, P:], sc[:, P:]
    return pack6(allc.reshape(rows, Kp)), alls


def quantize_x(x, idx, KE):
    return _quantize(x, idx, KE, True)


def quantize_w(w, idx, KE):
    return _quantize(w, idx, KE, False)


def dequantize(Q: np.ndarray, SF: np.ndarray) -> np.ndarray:
    """[rows, 3 Kp / 4] codes + [rows, Kp / 32] scale bytes -> fp64 [rows, Kp]."""
    v = e3m2_value(unpack6(Q)).reshape(Q.shape[0], SF.shape[1], 32)
    return np.ldexp(v, SF.astype(np.int64)[..., None] - 127).reshape(Q.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------- edge values
def _bits(v) -> np.ndarray:
    return (bf16_round(np.asarray(v, dtype=np.float32)).view(np.uint32) >> 16).astype(np.uint16)


_TIES = np.concatenate([(E3M2[:-1] + E3M2[1:]) / 2, [E3M2_MAX]])           # the 31 midpoints of adjacent codes and one 28: e = 0
_SIGNS = np.where(np.arange(32) % 3 == 0, -1.0, 1.0)
# name -> (bf16 bits [32], scale byte, codes [32] or None where the test only needs the residual rule)
EDGE_BLOCKS = {
    "code ties": (_bits(_TIES * _SIGNS), 127, (np.r_[(np.arange(31) + 1) // 2 * 2, 31] | np.where(_SIGNS < 0, 32, 0)).astype(np.uint8)),
    "code ties at 2^-9": (_bits(_TIES * _SIGNS * 2.0 ** -9), 118, None),
    "amax = 28 * 2^3": (np.r_[np.uint16(0x4360), _bits(np.arange(31) * 5.0)], 130, None),                  # 0x4360 = 224
    "amax one ulp above 28 * 2^3": (np.r_[np.uint16(0x4361), _bits(np.arange(31) * 5.0)], 131, None),
    "all zero": (np.zeros(32, np.uint16), 127, np.zeros(32, np.uint8)),
    "negative zero": (np.full(32, 0x8000, np.uint16), 127, np.full(32, 32, np.uint8)),
    "subnormals (e clamped to -127)": ((np.arange(32) * 4 + 1).astype(np.uint16), 0, None),
    "largest finite": (np.r_[np.uint16(0x7F7F), np.uint16(0xFF00) + np.arange(31, dtype=np.uint16)], 251, None),
}


def edge_row(KQ: int, idx) -> np.ndarray:
    """bf16 bits [KQ] of a row whose REORDERED blocks cycle through EDGE_BLOCKS, starting so that the last block is the last edge block."""
    names = list(EDGE_BLOCKS)
    B = KQ // 32
    xr = np.stack([EDGE_BLOCKS[names[(b - B) % len(names)]][0] for b in range(B)]).reshape(KQ)
    x = np.empty(KQ, dtype=np.uint16)
    x[np.asarray(idx, dtype=np.int64)] = xr
    return x
