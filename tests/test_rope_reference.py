"""CPU tests of the RoPE reference (tests/rope_reference.py) and of ``kvrope.rope_tables``: the torch-eager formula equals its three-rounding
fp32 restatement byte for byte (and a single-rounding form does not, so a byte-exact GPU test tells the two apart); position 0 is the
identity; in fp64 the rotated dot product depends on the distance of the positions only; the library's tables are the reference's bits."""
import pytest
import torch

from arcquant_amd import kvrope
from tests import rope_reference as RR

F16, BF16 = torch.float16, torch.bfloat16


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("theta", [1e4, 1e6])
def test_eager_equals_the_three_rounding_restatement(dtype, theta):
    n = 4096
    cos, sin = RR.rope_tables(n, theta, dtype)
    pos = torch.arange(n)
    x = RR.rows(n, 2, dtype, seed=int(theta) % 97 + (dtype is F16))
    want = RR.apply_rope(x, pos, cos, sin)
    assert want.dtype is dtype and torch.isfinite(want.float()).all()
    assert torch.equal(RR.bits(want), RR.bits(RR.apply_rope_stepwise(x, pos, cos, sin)))
    once = RR.apply_rope_single_rounding(x, pos, cos, sin)
    differ = (RR.bits(want) != RR.bits(once)).float().mean().item()
    assert differ > 0.05, f"a single rounding differs on {differ:.3f} of the elements only: a byte-exact test would not tell the forms apart"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_position_zero_is_the_identity(dtype):
    cos, sin = RR.rope_tables(8, 1e4, dtype)
    assert (cos[0] == 1).all() and (sin[0] == 0).all()
    x = RR.rows(16, 2, dtype, seed=3)
    got = RR.apply_rope(x, torch.zeros(16, dtype=torch.int64), cos, sin)
    assert torch.equal(got, x)                                # (values: x * 1 + (-0) is x, and -0 + 0 compares equal to -0)


@pytest.mark.parametrize("shift", [1, 17, 1000])
def test_rotated_dot_product_depends_on_the_distance_only(shift):
    cos, sin = RR.rope_tables_f64(2048, 1e4)
    g = torch.Generator().manual_seed(shift)
    q, k = torch.randn((8, 1, 128), generator=g, dtype=torch.float64), torch.randn((8, 1, 128), generator=g, dtype=torch.float64)
    m, n = torch.arange(8) * 97 + 5, torch.arange(8) * 31

    def dot(dm):
        return (RR.apply_rope(q, m + dm, cos, sin) * RR.apply_rope(k, n + dm, cos, sin)).sum(-1)
    a, b = dot(0), dot(shift)
    assert ((a - b).abs() <= 1e-9 * a.abs().clamp(min=1.0)).all()
    assert ((a - (q * k).sum(-1)).abs() > 1e-3).any()         # (and the rotation does something)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("theta", [1e4, 5e5, 1e6])
def test_library_tables_equal_the_reference_tables(dtype, theta):
    cos, sin = kvrope.rope_tables(1024, theta, dtype)
    rc, rs = RR.rope_tables(1024, theta, dtype)
    assert cos.dtype is dtype and tuple(cos.shape) == (1024, 128) and cos.is_contiguous() and sin.is_contiguous()
    assert torch.equal(RR.bits(cos), RR.bits(rc)) and torch.equal(RR.bits(sin), RR.bits(rs))
    assert torch.equal(cos[:, :64], cos[:, 64:])              # the Hugging Face layout: emb = cat(freqs, freqs)


def test_library_tables_defaults_and_refusals():
    cos, sin = kvrope.rope_tables(4)
    assert cos.dtype is BF16 and torch.equal(RR.bits(cos), RR.bits(RR.rope_tables(4, 10000.0, BF16)[0]))
    with pytest.raises(RuntimeError):
        kvrope.rope_tables(0)
    with pytest.raises(RuntimeError):
        kvrope.rope_tables(4, dtype=torch.float32)
