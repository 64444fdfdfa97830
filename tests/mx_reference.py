"""numpy restatement of MXFP4-ARC (include/arcq.h "MXFP4", DESIGN.md "MXFP4"): the block rule, the quantisers with their
packed layout, and an fp64 dequantised GEMM.

``fake_semantics=True`` reproduces the reference's fake path (model/quantize.py quantize_mxfp4_tensor and
fake_reorder_quantize_{x,w}(dtype='MXFP4')) instead, in its own dtype, for the fixture comparison: there the exponent is
``ceil(log2(amax/6 + 1e-9))`` evaluated in the input dtype, and argmin ties go to the lower representable value.  Those two
rules are the only places where the fake path and the packed format differ."""
from __future__ import annotations

import numpy as np

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# the fake path's table, in its order (model/quantize.py quantize_e2m1): argmin takes the FIRST of two equal distances
FAKE_VALS = np.array([-6.0, -4.0, -3.0, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
PAD_SCALE = 127


def k_padded(K: int) -> int:
    return (K + 127) // 128 * 128


def bf16_round(a) -> np.ndarray:
    """float32 -> nearest bf16 (RNE), returned as float32."""
    u = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def block_exponent(amax: np.ndarray) -> np.ndarray:
    """Smallest integer e with amax <= 6 * 2^e, clamped to [-127, 127]; 0 where amax == 0.  Exact (frexp, no log)."""
    amax = np.asarray(amax, dtype=np.float64)
    f, F = np.frexp(amax)                       # amax = f * 2^F, f in [0.5, 1)
    e = np.where(f <= 0.75, F - 3, F - 2)
    e = np.clip(e, -127, 127)
    return np.where(amax == 0, 0, e).astype(np.int64)


def e2m1_rne(y: np.ndarray) -> np.ndarray:
    """|y| <= 6 -> 4-bit code, round to nearest, ties to the even code, sign of zero kept."""
    a = np.abs(y)
    lo = np.clip(np.searchsorted(E2M1, a, side="right") - 1, 0, 6)
    hi = lo + 1
    dlo, dhi = a - E2M1[lo], E2M1[hi] - a
    c = np.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo)
    return (c | np.where(np.signbit(y), 8, 0)).astype(np.uint8)


def e2m1_value(c: np.ndarray) -> np.ndarray:
    c = np.asarray(c).astype(np.int64)
    v = E2M1[c & 7]
    return np.where(c & 8, -v, v)


def quantize_blocks(v: np.ndarray):
    """v [..., 32] (exact fp32 / fp64 values) -> (codes uint8 [..., 32], scale bytes uint8 [...], residual fp64 [..., 32])."""
    v = np.asarray(v, dtype=np.float64)
    e = block_exponent(np.abs(v).max(axis=-1))
    y = np.ldexp(v, -e[..., None])
    assert np.all(np.abs(y) <= 6.0), "a code would saturate"
    codes = e2m1_rne(y)
    res = v - np.ldexp(e2m1_value(codes), e[..., None])
    return codes, (e + 127).astype(np.uint8), res


def pack(codes: np.ndarray) -> np.ndarray:
    codes = codes.astype(np.uint8)
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def unpack(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q, dtype=np.uint8)
    out = np.empty(q.shape[:-1] + (q.shape[-1] * 2,), dtype=np.uint8)
    out[..., 0::2] = q & 15
    out[..., 1::2] = q >> 4
    return out


def _quantize(x: np.ndarray, idx: np.ndarray, KE: int, is_x: bool, check_residual: bool = True):
    """x: [rows, KQ] float32 values of bf16 inputs.  Returns (Q [rows, Kp/2], SF [rows, Kp/32])."""
    x = np.asarray(x, dtype=np.float32)
    rows, KQ = x.shape
    assert KQ % 64 == 0 and KE % 64 == 0 and 0 <= KE <= KQ
    K = KQ + KE
    Kp = k_padded(K)
    xr = x[:, np.asarray(idx, dtype=np.int64)].astype(np.float64).reshape(rows, KQ // 32, 32)
    codes, sc, res = quantize_blocks(xr)
    allc = np.zeros((rows, Kp // 32, 32), dtype=np.uint8)
    alls = np.full((rows, Kp // 32), PAD_SCALE, dtype=np.uint8)
    allc[:, : KQ // 32] = codes
    alls[:, : KQ // 32] = sc
    if KE:
        P = (KQ - KE) // 32
        if is_x:
            r = res[:, P:]
            if check_residual:
                assert np.array_equal(bf16_round(r.astype(np.float32)).astype(np.float64), r), "residual not exact in bf16"
            rc, rs, _ = quantize_blocks(r)
            allc[:, KQ // 32: K // 32] = rc
            alls[:, KQ // 32: K // 32] = rs
        else:
            allc[:, KQ // 32: K // 32] = codes[:, P:]
            alls[:, KQ // 32: K // 32] = sc[:, P:]
    return pack(allc.reshape(rows, Kp)), alls


def quantize_x(x, idx, KE):
    return _quantize(x, idx, KE, True)


def quantize_w(w, idx, KE):
    return _quantize(w, idx, KE, False)


def dequantize(Q: np.ndarray, SF: np.ndarray) -> np.ndarray:
    """[rows, Kp/2] codes + [rows, Kp/32] scale bytes -> fp64 [rows, Kp]."""
    v = e2m1_value(unpack(Q)).reshape(Q.shape[0], SF.shape[1], 32)
    return np.ldexp(v, SF.astype(np.int64)[..., None] - 127).reshape(Q.shape[0], -1)


def gemm(QA, QB, SFA, SFB, alpha=1.0) -> np.ndarray:
    """fp64 alpha * deq(A) . deq(B)^T."""
    return alpha * (dequantize(QA, SFA) @ dequantize(QB, SFB).T)


def abs_gemm(QA, QB, SFA, SFB) -> np.ndarray:
    """fp64 sum_k |deq(A)[m,k]| |deq(B)[n,k]|: the magnitude every partial sum of gemm() stays under, in any order."""
    return np.abs(dequantize(QA, SFA)) @ np.abs(dequantize(QB, SFB)).T


def bf16_rne_bits(x) -> np.ndarray:
    """fp64 -> bit pattern of the nearest bf16 (RNE) in ONE rounding (bf16_round takes fp32: from fp64 that would round twice).
    For zero and the normal range of bf16, which is all a GEMM output needs."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all((x == 0) | ((np.abs(x) >= 2.0 ** -126) & (np.abs(x) < 2.0 ** 128 * (1 - 2.0 ** -9)))), "outside the range this helper rounds exactly"
    m, e = np.frexp(x)                          # x = m * 2^e, |m| in [0.5, 1): 8 significant bits = a multiple of 2^-8
    v = np.ldexp(np.rint(m * 256.0), e - 8)     # m * 256 is exact in fp64, rint rounds half to even
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_key(b) -> np.ndarray:
    """Monotone integer key of a bf16 bit pattern (tests/test_gpu_parity.py _max_bf16_ulp_diff): a < b as values <=> key(a) < key(b),
    with -0 and +0 on the same key."""
    b = np.asarray(b).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


# ---------------------------------------------------------------------------------------------------------------- special values
BOUNDARY_BITS = (0x4040, 0x40C0, 0x4041, 0x40C1)           # 3.0, 6.0, 3.015625, 6.03125: the two with a residual come last
TIE_BITS = (0x3E80, 0x3F40, 0x3FA0, 0x3FE0, 0x4020, 0x4060, 0x40A0, 0x40C0)    # 0.25 0.75 1.25 1.75 2.5 3.5 5.0 6.0
SPECIAL_ROWS = ("zero", "negative zero", "subnormals", "smallest normals", "largest finite", "exponent boundaries", "e2m1 ties",
                "subnormal blocks beside ordinary ones")


def special_value_rows(KQ: int, idx, seed: int) -> np.ndarray:
    """bf16 bit patterns [8, KQ] (SPECIAL_ROWS) whose REORDERED rows X[:, idx] are the blocks described below, so that whatever
    the permutation every kind of block also lies in the outlier tail (the last KE reordered channels) for any KE >= 64:
      0  +0 everywhere                              1  -0.0 everywhere
      2  subnormals 0x0001..0x007F, both signs      3  the smallest normals 0x0080..0x00FF, both signs
      4  0x7F00..0x7F7F, both signs, one 0x7F7F (the largest finite bf16) per block
      5  block b is all +-BOUNDARY_BITS[b % 4]: amax on and one bf16 ulp above the exponent rule's two boundaries
      6  the eight e2m1 ties (6.0 among them, so e = 0), both signs, four times per block
      7  even blocks subnormals, odd blocks 1 <= |v| < 8 with one 7.0."""
    assert KQ % 128 == 0
    rng = np.random.default_rng(seed)
    B = KQ // 32
    sign = lambda: (rng.integers(0, 2, (B, 32)).astype(np.uint16) << 15)       # noqa: E731
    xr = np.zeros((8, B, 32), dtype=np.uint16)
    xr[1] = 0x8000
    xr[2] = rng.integers(0x0001, 0x0080, (B, 32)).astype(np.uint16) | sign()
    xr[3] = rng.integers(0x0080, 0x0100, (B, 32)).astype(np.uint16) | sign()
    big = rng.integers(0x7F00, 0x7F80, (B, 32)).astype(np.uint16)
    big[np.arange(B), rng.integers(0, 32, B)] = 0x7F7F
    xr[4] = big | sign()
    xr[5] = np.asarray(BOUNDARY_BITS, dtype=np.uint16)[np.arange(B) % 4][:, None] | sign()
    xr[6] = np.tile(np.asarray(TIE_BITS, dtype=np.uint16), 4)[rng.permuted(np.tile(np.arange(32), (B, 1)), axis=1)] | sign()
    ordinary = (bf16_round(rng.uniform(1.0, 7.9, (B, 32)).astype(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
    ordinary[np.arange(B), rng.integers(0, 32, B)] = 0x40E0                    # 7.0
    sub = rng.integers(0x0001, 0x0080, (B, 32)).astype(np.uint16)
    xr[7] = np.where((np.arange(B) % 2 == 0)[:, None], sub, ordinary) | sign()
    X = np.empty((8, KQ), dtype=np.uint16)
    X[:, np.asarray(idx, dtype=np.int64)] = xr.reshape(8, KQ)
    return X


# ---------------------------------------------------------------------------------------------------------------- fake path
def _round_to(a: np.ndarray, dtype: str) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    return bf16_round(a) if dtype == "bf16" else a


def fake_block_exponent(amax: np.ndarray, dtype: str) -> np.ndarray:
    """ceil(log2(amax/6 + 1e-9)) in the input dtype, clamped (model/quantize.py quantize_ue8m0 after scale = amax / 6,
    scale[scale == 0] = 1e-9); each torch op rounds to the dtype."""
    s = _round_to(np.asarray(amax, dtype=np.float32) / np.float32(6.0), dtype)
    s = np.where(s == 0, _round_to(np.float32(1e-9), dtype), s).astype(np.float32)
    t = _round_to(s + np.float32(1e-9), dtype)
    lg = _round_to(np.log2(t.astype(np.float64)).astype(np.float32), dtype)
    return np.clip(np.ceil(lg), -127, 127).astype(np.int64)


def fake_quantize_blocks(v: np.ndarray, dtype: str, fake_semantics: bool):
    """v [..., 32] values in the input dtype -> (dequantised values as float32 in that dtype, exponents)."""
    v = np.asarray(v, dtype=np.float32)
    if not fake_semantics:
        codes, sc, _ = quantize_blocks(v.astype(np.float64))
        e = sc.astype(np.int64) - 127
        return np.ldexp(e2m1_value(codes), e[..., None]).astype(np.float32), e
    e = fake_block_exponent(np.abs(v).max(axis=-1), dtype)
    y = _round_to(np.ldexp(v.astype(np.float64), -e[..., None]).astype(np.float32), dtype)
    d = _round_to(np.abs(y[..., None] - FAKE_VALS.astype(np.float32)), dtype)
    q = FAKE_VALS[np.argmin(d, axis=-1)]                       # first minimum = the lower value
    return _round_to(np.ldexp(q, e[..., None]).astype(np.float32), dtype), e


def fake_quantize_tensor(t: np.ndarray, dtype: str, fake_semantics: bool = True) -> np.ndarray:
    """quantize_mxfp4_tensor on [..., n], n % 32 == 0 (the dequantised tensor, float32 values of the dtype)."""
    t = np.asarray(t, dtype=np.float32)
    d, _ = fake_quantize_blocks(t.reshape(-1, 32), dtype, fake_semantics)
    return d.reshape(t.shape)


def fake_reorder_quantize(x: np.ndarray, perm: np.ndarray, KE: int, is_x: bool, dtype: str, fake_semantics: bool = True):
    """The commented-out form of model/qLinearLayer.py:58 / model/qQwenLayer.py:81-83: reorder the channels, then
    fake_reorder_quantize_{x,w}(xr, arange, KE, dtype='MXFP4') -> the dequantised concatenation [rows, KQ + KE]."""
    xr = np.asarray(x, dtype=np.float32)[:, np.asarray(perm, dtype=np.int64)]
    KQ = xr.shape[1]
    q = fake_quantize_tensor(xr, dtype, fake_semantics)
    if KE == 0:
        return q
    if is_x:
        err = _round_to(xr - q, dtype)[:, KQ - KE:]
        return np.concatenate([q, fake_quantize_tensor(err, dtype, fake_semantics)], axis=1)
    return np.concatenate([q, fake_quantize_tensor(xr[:, KQ - KE:], dtype, fake_semantics)], axis=1)
