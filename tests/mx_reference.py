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
