"""CPU checks of tests/mx_reference.py, the statement of MXFP4-ARC (include/arcq.h "MXFP4"): with ``fake_semantics`` it reproduces
the reference's fake MXFP4 path bit for bit (tests/golden/fake_mxfp4.npz); without it, every element that differs from the fake
path is explained by one of the two named rules; the residual is exact, no code saturates, the padding is 0 / 127, and the
ARC residual channels do what they are for."""
import numpy as np
import pytest
import torch

from tests import mx_reference as R
from tests.util import outlier_activations, random_perm

DTS = ("fp32", "bf16")


def _vals(bits_arr, dt):
    return R.bf16_bits_to_f32(bits_arr) if dt == "bf16" else np.asarray(bits_arr, dtype=np.uint32).view(np.float32)


def _bits(v, dt):
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
    return (v.view(np.uint32) >> 16).astype(np.uint16) if dt == "bf16" else v.view(np.uint32)


@pytest.mark.parametrize("dt", DTS)
def test_fake_semantics_reproduce_quantize_mxfp4_tensor(golden, dt):
    f = golden("fake_mxfp4.npz")
    got = R.fake_quantize_tensor(_vals(f[f"t_{dt}"], dt), dt, fake_semantics=True)
    want = f[f"q_{dt}"]
    # the fake path returns +0 where the format keeps the sign of zero: compare bits with zeros folded
    g, w = _bits(got, dt), np.asarray(want)
    zero = _vals(w, dt) == 0
    assert np.array_equal(np.where(zero, 0, g), np.where(zero, 0, w))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("KE", [0, 64])
@pytest.mark.parametrize("is_x", [True, False], ids=["x", "w"])
def test_fake_semantics_reproduce_fake_reorder_quantize(golden, dt, KE, is_x):
    f = golden("fake_mxfp4.npz")
    key = f"{dt}_KE{KE}"
    src = _vals(f[("x_" if is_x else "w_") + key], dt)
    got = R.fake_reorder_quantize(src, f["perm_" + key], KE, is_x, dt, fake_semantics=True)
    want = f[("qx_" if is_x else "qw_") + key]
    zero = _vals(want, dt) == 0
    assert np.array_equal(np.where(zero, 0, _bits(got, dt)), np.where(zero, 0, want))


def _rules(v, dt):
    """Per element of blocks v [..., 32]: (exponent rule differs, element is an exact e2m1 tie at the common exponent)."""
    e_fake = R.fake_block_exponent(np.abs(v).max(axis=-1), dt)
    e_fmt = R.block_exponent(np.abs(v).max(axis=-1).astype(np.float64))
    exp_rule = np.broadcast_to((e_fake != e_fmt)[..., None], v.shape)
    y = np.abs(np.ldexp(v.astype(np.float64), -e_fmt[..., None]))
    mids = (R.E2M1[:-1] + R.E2M1[1:]) / 2
    tie = np.isin(y, mids)
    return exp_rule, tie


@pytest.mark.parametrize("dt", DTS)
def test_every_difference_from_the_fake_path_has_a_named_rule(golden, dt):
    f = golden("fake_mxfp4.npz")
    t = _vals(f[f"t_{dt}"], dt)
    fmt = R.fake_quantize_tensor(t, dt, fake_semantics=False)
    fake = R.fake_quantize_tensor(t, dt, fake_semantics=True)
    diff = (fmt != fake).reshape(-1, 32)
    exp_rule, tie = _rules(t.reshape(-1, 32), dt)
    assert diff.any(), "the fixture should exercise at least one of the rules"
    assert not (diff & ~exp_rule & ~tie).any()
    for KE in (0, 64):
        for is_x in (True, False):
            key = f"{dt}_KE{KE}"
            src = _vals(f[("x_" if is_x else "w_") + key], dt)
            a = R.fake_reorder_quantize(src, f["perm_" + key], KE, is_x, dt, fake_semantics=False)
            b = R.fake_reorder_quantize(src, f["perm_" + key], KE, is_x, dt, fake_semantics=True)
            KQ = src.shape[1]
            xr = src[:, f["perm_" + key]]
            d = (a[:, :KQ] != b[:, :KQ]).reshape(xr.shape[0], -1, 32)
            er, ti = _rules(xr.reshape(xr.shape[0], -1, 32), dt)
            assert not (d & ~er & ~ti).any()
            if KE:       # a residual / duplicate block may differ only where its source block or its own block has a rule
                src_blocks = d.any(axis=-1)[:, -(KE // 32):]
                dr = (a[:, KQ:] != b[:, KQ:]).reshape(xr.shape[0], -1, 32)
                rv = (xr - a[:, :KQ])[:, KQ - KE:] if is_x else xr[:, KQ - KE:]
                er2, ti2 = _rules(rv.reshape(xr.shape[0], -1, 32).astype(np.float32), dt)
                assert not (dr & ~src_blocks[..., None] & ~er2 & ~ti2).any()


def _case(M, KQ, seed):
    x = outlier_activations(M, KQ, seed)
    return R.bf16_bits_to_f32(x.contiguous().view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize("KQ,KE", [(64, 0), (64, 64), (256, 64), (4096, 64), (3584, 256)])
def test_residual_exact_no_saturation_and_padding(KQ, KE):
    x = _case(6, KQ, KQ + KE)
    idx = random_perm(KQ, 3).numpy().astype(np.int64)
    Q, S = R.quantize_x(x, idx, KE)              # asserts: residual exact in bf16, |v * 2^-e| <= 6
    K, Kp = KQ + KE, R.k_padded(KQ + KE)
    assert Q.shape == (6, Kp // 2) and S.shape == (6, Kp // 32)
    assert np.all(Q[:, K // 2:] == 0) and np.all(S[:, K // 32:] == 127)
    assert not np.any(S == 255)
    W, SW = R.quantize_w(x, idx, KE)
    assert np.array_equal(W[:, KQ // 2: K // 2], W[:, (KQ - KE) // 2: KQ // 2])
    assert np.array_equal(SW[:, KQ // 32: K // 32], SW[:, (KQ - KE) // 32: KQ // 32])
    # the residual really is v - deq(code) * 2^e of the tail channels
    xr = x[:, idx].astype(np.float64)
    dq = R.dequantize(Q, S)
    if KE:
        res = xr[:, KQ - KE:] - dq[:, KQ - KE: KQ]
        assert np.array_equal(R.bf16_round(res.astype(np.float32)).astype(np.float64), res)


def test_block_rule_is_exact():
    amax = np.array([0.0, 6.0, 6.0 * 2 ** -3, np.nextafter(np.float32(6.0), np.float32(7.0)), 3.0, 1e-40, 3.3e38])
    e = R.block_exponent(amax)
    assert list(e) == [0, 0, -3, 1, -1, -127, 126]
    for a, ee in zip(amax[1:5], e[1:5]):
        assert a <= 6 * 2.0 ** ee and a > 6 * 2.0 ** (ee - 1)
    assert list(R.e2m1_rne(np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.0]))) == [0, 2, 2, 4, 4, 6, 6, 8]


def test_arc_residual_channels_reduce_the_error():
    """Outlier activations, identity index: the GEMM's error against x . deq(W)^T falls as KE grows."""
    M, N, KQ = 16, 64, 1024
    x = _case(M, KQ, 5)
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(N, KQ, generator=g) * 0.05).to(torch.bfloat16)
    wf = R.bf16_bits_to_f32(w.view(torch.int16).numpy().view(np.uint16))
    idx = np.arange(KQ)
    errs = []
    for KE in (0, 64, 128, 256):
        QX, SX = R.quantize_x(x, idx, KE)
        QW, SW = R.quantize_w(wf, idx, KE)
        want = x.astype(np.float64) @ R.dequantize(QW, SW)[:, :KQ].T
        got = R.gemm(QX, QW, SX, SW)
        errs.append(np.linalg.norm(got - want) / np.linalg.norm(want))
    assert all(a > b for a, b in zip(errs, errs[1:])), errs
