"""Rotary position embedding restated with torch eager on CPU tensors: the reference of the RoPE tests.  Test infrastructure, independent
of the library.

    rotate_half(x) = cat(-x[..., 64:], x[..., :64])           (head dimension 128)
    apply_rope(x, positions, cos, sin) = x * cos[positions] + rotate_half(x) * sin[positions]

literally as the reference's model path writes it (transformers' ``apply_rotary_pos_emb``), on tensors of the activation dtype: torch
rounds each product and the sum to that dtype.  ``apply_rope_stepwise`` spells the same out in fp32 with the three roundings explicit (what
the kernels do); tests/test_rope_reference.py pins that the two agree byte for byte.
"""
from __future__ import annotations

import torch

D = 128


def rope_tables(rope_len, theta=10000.0, dtype=torch.bfloat16):
    """(cos, sin) [rope_len, 128] as Hugging Face builds them: fp32 on the CPU, emb = cat(freqs, freqs), then ``.to(dtype)``."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    t = torch.arange(rope_len, dtype=torch.int64).float()
    freqs = torch.outer(t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def rope_tables_f64(rope_len, theta=10000.0):
    inv_freq = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    freqs = torch.outer(torch.arange(rope_len, dtype=torch.float64), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos(), emb.sin()


def rotate_half(x):
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rope(x, positions, cos, sin):
    """x [tokens, heads, 128] on the CPU, positions int [tokens] -> the rotated rows, in x's dtype, by torch eager."""
    assert x.device.type == "cpu" and x.shape[-1] == D and cos.dtype is x.dtype and sin.dtype is x.dtype
    idx = torch.as_tensor(positions, dtype=torch.int64)
    c, s = cos[idx].unsqueeze(1), sin[idx].unsqueeze(1)
    return x * c + rotate_half(x) * s


def apply_rope_stepwise(x, positions, cos, sin):
    """The same in fp32 with an explicit rounding to x's dtype after each product and after the sum."""
    T = x.dtype

    def rnd(f):
        return f.to(T).float()
    idx = torch.as_tensor(positions, dtype=torch.int64)
    c, s = cos[idx].unsqueeze(1).float(), sin[idx].unsqueeze(1).float()
    xf = x.float()
    return rnd(rnd(xf * c) + rnd(rotate_half(xf) * s)).to(T)


def apply_rope_single_rounding(x, positions, cos, sin):
    """What a kernel that rounds once would give: NOT the reference (tests pin that it differs)."""
    idx = torch.as_tensor(positions, dtype=torch.int64)
    c, s = cos[idx].unsqueeze(1).float(), sin[idx].unsqueeze(1).float()
    xf = x.float()
    return (xf * c + rotate_half(xf) * s).to(x.dtype)


def rows(ntok, heads, dtype, seed):
    """Seeded normal values times per-row magnitudes 2^-12 .. 2^4 (fp16 products then land on the subnormal grid) -> [ntok, heads, 128]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((ntok, heads, D), generator=g)
    mag = 2.0 ** torch.randint(-12, 5, (ntok, heads, 1), generator=g).float()
    return (x * mag).to(dtype)


def bits(t):
    """int16 view of a 16-bit tensor (compared as integers: -0 and +0 differ)."""
    return t.contiguous().view(torch.int16)
