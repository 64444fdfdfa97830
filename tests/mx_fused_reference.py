"""numpy restatement of the row arcq_mx_rmsnorm_quantize_x quantises: the normalised row of arcq_rmsnorm_quantize_x
(oracle/arcq_oracle.c rms_sumsq + arcq_o_rmsnorm_quantize_x), followed by tests/mx_reference.py's MXFP4 quantiser on the already
reordered row.  tests/test_mx_fused_reference.py pins this restatement to the committed C oracle."""
from __future__ import annotations

import numpy as np

from tests import mx_reference as R


def rms_sumsq(x: np.ndarray) -> np.ndarray:
    """x float32 [M, KQ] (values of bf16) -> float32 [M]: the sum of squares in rms_sumsq's association order.  Virtual thread
    t < bdx = KQ/16 adds the squares of the 8-element chunks t and bdx + t sequentially; then s[t] += s[t + stride] for stride 256 and
    128 (guarded by t + stride < bdx), 64, 32, 16, ... 1.  Every operation in float32."""
    x = np.asarray(x, dtype=np.float32)
    M, KQ = x.shape
    bdx = KQ // 16
    assert KQ % 16 == 0 and 128 <= bdx <= 512
    ch = x.reshape(M, 2, bdx, 8)
    s = np.zeros((M, 1024), dtype=np.float32)
    acc = np.zeros((M, bdx), dtype=np.float32)
    for it in range(2):
        for j in range(8):
            v = ch[:, it, :, j]
            acc = (acc + (v * v).astype(np.float32)).astype(np.float32)      # v * v is exact in fp32
    s[:, :bdx] = acc
    for stride in (256, 128):
        t = np.arange(min(stride, bdx))
        t = t[t + stride < bdx]
        s[:, t] = s[:, t] + s[:, t + stride]
    for stride in (64, 32, 16, 8, 4, 2, 1):
        t = np.arange(stride)
        s[:, t] = s[:, t] + s[:, t + stride]
    return s[:, 0].copy()


def normalised_rows(x_bits: np.ndarray, w_bits: np.ndarray, eps: float, idx: np.ndarray) -> np.ndarray:
    """bf16 bit patterns X [M, KQ], norm weight [KQ] -> float32 [M, KQ]: xn[c] = bf16((x[i] * w[i]) * rstd), i = idx[c]."""
    x = R.bf16_bits_to_f32(x_bits)
    w = R.bf16_bits_to_f32(w_bits)
    KQ = x.shape[1]
    var = (rms_sumsq(x) / np.float32(KQ) + np.float32(eps)).astype(np.float32)
    rstd = (1.0 / np.sqrt(var.astype(np.float64))).astype(np.float32)
    i = np.asarray(idx, dtype=np.int64)
    v = ((x[:, i] * w[i]).astype(np.float32) * rstd[:, None]).astype(np.float32)
    return R.bf16_round(v)


def rmsnorm_quantize_x(x_bits, w_bits, eps, idx, KE):
    """-> (Q [M, Kp/2], SF [M, Kp/32]) of arcq_mx_rmsnorm_quantize_x."""
    rows = normalised_rows(x_bits, w_bits, eps, idx)
    return R.quantize_x(rows, np.arange(rows.shape[1]), KE)
