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


def _bits_block(b):
    return R.bf16_bits_to_f32(np.full(32, b, dtype=np.uint16)).astype(np.float64)


def test_special_blocks_by_hand():
    """The block rule at its edges, expected values written out: (bf16 bits of every element) -> scale byte, code, residual."""
    for b, byte, code, res in [
        (0x0000, 127, 0, 0.0),                     # zero block: e = 0
        (0x8000, 127, 8, 0.0),                     # -0.0: the code keeps the sign
        (0x0001, 0, 0, 2.0 ** -133),               # smallest subnormal: clamp at e = -127, y = 2^-6 -> code 0, residual = v
        (0x007F, 0, 4, -2.0 ** -133),              # largest subnormal 127 * 2^-133: y = 1.984375 -> 2.0
        (0x0080, 0, 4, 0.0),                       # smallest normal 2^-126: e would be -128, clamped: y = 2
        (0x4040, 126, 7, 0.0),                     # 3.0 = 6 * 2^-1
        (0x4041, 127, 5, 0.015625),                # 3.015625 > 6 * 2^-1: e = 0, code 3.0
        (0x40C0, 127, 7, 0.0),                     # 6.0 = 6 * 2^0
        (0x40C1, 128, 5, 0.03125),                 # 6.03125: e = 1, y = 3.015625 -> 3.0
        (0x7F7F, 253, 6, -2.0 ** 120),             # largest finite 1.9921875 * 2^127: e = 126, y = 3.984375 -> 4.0, and 4 * 2^126 = 2^128
        (0xFF7F, 253, 14, 2.0 ** 120),
    ]:
        codes, sc, r = R.quantize_blocks(_bits_block(b)[None, :])
        assert (int(sc[0]), set(codes[0]), set(r[0])) == (byte, {code}, {res}), hex(b)
    assert list(R.e2m1_rne(R.bf16_bits_to_f32(np.asarray(R.TIE_BITS, dtype=np.uint16)))) == [0, 2, 2, 4, 4, 6, 6, 7]
    assert list(R.block_exponent(np.array([2.0 ** -133, 2.0 ** -126, 1.75 * 2.0 ** -126, 2.0 ** -125, 1.5 * 2.0 ** 127]))) == [-127, -127, -127, -127, 125]


@pytest.mark.parametrize("perm", ["identity", "random"])
@pytest.mark.parametrize("KQ,KE", [(128, 0), (128, 64), (128, 128), (4096, 64)])
def test_special_value_rows(KQ, KE, perm):
    """R.special_value_rows is what its docstring says in REORDERED order for any permutation, the reference accepts it (residual exact
    in bf16, no code saturates), and its scale bytes are the hand-derived ones."""
    idx = np.arange(KQ) if perm == "identity" else random_perm(KQ, 5).numpy().astype(np.int64)
    Xb = R.special_value_rows(KQ, idx, 1)
    B = KQ // 32
    xr = Xb[:, idx].reshape(8, B, 32)
    mag = xr & 0x7FFF
    assert np.all(xr[0] == 0) and np.all(xr[1] == 0x8000)
    assert np.all((mag[2] >= 1) & (mag[2] <= 0x7F)) and np.all((mag[3] >= 0x80) & (mag[3] <= 0xFF))
    assert np.all((mag[4] >= 0x7F00) & (mag[4].max(axis=-1, keepdims=True) == 0x7F7F))
    assert np.all(mag[5] == np.asarray(R.BOUNDARY_BITS)[np.arange(B) % 4][:, None])
    assert all(sorted(blk) == sorted(R.TIE_BITS * 4) for blk in mag[6])
    for r in (2, 3, 4, 5, 6, 7):
        assert len(np.unique(xr[r] >> 15)) == 2, "both signs"
    Q, S = R.quantize_x(R.bf16_bits_to_f32(Xb), idx, KE)          # asserts: residual exact in bf16, |v * 2^-e| <= 6
    Sb = S[:, :B]
    assert np.all(Sb[0] == 127) and np.all(Sb[1] == 127) and np.all(Sb[2] == 0) and np.all(Sb[3] == 0) and np.all(Sb[4] == 253)
    assert np.array_equal(Sb[5], np.asarray([126, 127, 127, 128])[np.arange(B) % 4]) and np.all(Sb[6] == 127)
    assert np.array_equal(Sb[7], np.where(np.arange(B) % 2 == 0, 0, 128))
    if KE == 0:
        assert set(np.unique(S)) == {0, 126, 127, 128, 253}
    else:
        r5 = S[5, B:B + KE // 32]                                  # residuals 0 / 0 / 2^-6 / 2^-5 per element: e = 0 / 0 / -8 / -7
        assert np.array_equal(r5, np.asarray([127, 127, 119, 120])[np.arange(B - KE // 32, B) % 4])
        assert np.all(S[4, B:B + KE // 32] >= 127 + 116)          # |residual| <= 2^125, a multiple of 2^120
    W, SW = R.quantize_w(R.bf16_bits_to_f32(Xb), idx, KE)
    assert np.array_equal(SW[:, :B], Sb) and np.array_equal(W[:, :KQ // 2], Q[:, :KQ // 2])


def test_abs_gemm_and_bf16_helpers():
    rng = np.random.default_rng(0)
    QA, QB = rng.integers(0, 256, (3, 64), dtype=np.uint8), rng.integers(0, 256, (5, 64), dtype=np.uint8)
    sa, sb = rng.integers(120, 135, (3, 4), dtype=np.uint8), rng.integers(120, 135, (5, 4), dtype=np.uint8)
    a, b = R.dequantize(QA, sa), R.dequantize(QB, sb)
    want = np.array([[sum(abs(a[m, k]) * abs(b[n, k]) for k in range(128)) for n in range(5)] for m in range(3)])
    assert np.array_equal(R.abs_gemm(QA, QB, sa, sb), np.abs(a) @ np.abs(b).T) and np.allclose(R.abs_gemm(QA, QB, sa, sb), want, rtol=1e-14)
    assert np.all(R.abs_gemm(QA, QB, sa, sb) >= np.abs(R.gemm(QA, QB, sa, sb)))
    # one rounding from fp64: 1 + 2^-8 + 2^-40 lies above the tie and goes up; through fp32 it would first land ON the tie and go to even
    x = np.array([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0, 0.0, 2.0 ** -126, 3.3e38])
    assert list(R.bf16_rne_bits(x)) == [0x3F81, 0x3F80, 0x3F82, 0xC040, 0x0000, 0x0080, 0x7F78]
    every = np.arange(0x0080, 0x7F80, dtype=np.uint16)              # every positive normal bf16 maps to itself
    assert np.array_equal(R.bf16_rne_bits(R.bf16_bits_to_f32(every).astype(np.float64)), every)
    k = R.bf16_key(np.array([0xC040, 0x8001, 0x8000, 0x0000, 0x0001, 0x4040], dtype=np.uint16))
    assert list(k) == [-0x4040, -1, 0, 0, 1, 0x4040]


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
