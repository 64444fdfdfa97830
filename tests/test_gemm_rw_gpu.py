"""GPU tests of the one-copy weight path (``-m gpu``): ``matmul_rw`` over the repacked weight against the two calls it replaces.

Route 1 (the repacked decode kernels) must equal ``matmul_repacked`` and routes 2 / 3 (register- / LDS-tiled kernels over RW) must
equal ``matmul`` on the reference-layout weight BIT FOR BIT -- the RW instantiations stage the same bytes into the same MFMA slots in
the same order.  The only exception are the G' shapes (decode where ``matmul`` takes an LDS-transposing kernel): fp64 oracle at the
suite's 1e-3 bar.  Then the SiLU epilogue, the extension module, ``QLinearLayer(repacked_only=True)`` and the e2e toy decoder."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -7777.0


def _ag():
    from arcquant_amd import agemm
    return agemm


def _quantized(rows, KQ, KE, seed, weight):
    ag = _ag()
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, KQ, generator=g, device=DEV, dtype=torch.float32)
    if not weight:
        x[:, -16:] *= 12.0                                        # a band of outlier channels, as activations have
    x = (x * (2688.0 / float(x.abs().max()))).to(torch.bfloat16)
    idx = torch.arange(KQ, dtype=torch.int16, device=DEV)
    return (ag.reorder_quantize_w if weight else ag.reorder_quantize_x)(x, idx, KE)


def _operands(M, N, KQ, KE, seed=0):
    ag = _ag()
    A, SFA = _quantized(M, KQ, KE, 1000 + seed + M, weight=False)
    B, SFB = _quantized(N, KQ, KE, 2000 + seed + N, weight=True)
    RW, RSF = ag.repack_w(B, SFB)
    return A, SFA, B, SFB, RW, RSF


def _reference_kernel_is_lds_transposing(M, N, K):
    """Whether arcq_gemm_nvfp4 serves this shape with gemm_skinny / gemm_decode (gemm_regtile.cfg: M <= 8 on very long K or very wide
    N), i.e. whether it is a G' shape of matmul_rw -- under the tuning override ARCQ_REGTILE_CFG too."""
    if M > 16:
        return False
    ov = int(os.environ.get("ARCQ_REGTILE_CFG", "0"))
    if ov < 0:
        return True
    if ov > 0:
        return ov not in range(1, 14)
    return not (M > 8 or (N <= 16384 and K <= 8448))


def _poisoned(M, N, dtype):
    return torch.full((M, N), POISON, dtype=dtype, device=DEV)


def _check_against_twin(A, SFA, B, SFB, RW, RSF, N, alpha=0.37, **kw):
    """matmul_rw into a poisoned buffer against the call it replaces; returns the route."""
    ag = _ag()
    M, K = A.shape[0], A.shape[1] * 2
    route = ag.rw_route(M, N, K)
    assert route in (1, 2, 3), (M, N, K)
    dt = kw.pop("out_dtype", torch.bfloat16)
    got = ag.matmul_rw(A, RW, SFA, RSF, alpha, N, out=_poisoned(M, N, dt), out_dtype=dt, **kw)
    if route == 1 and not _misaligned(kw):
        want = ag.matmul_repacked(A, RW, SFA, RSF, alpha, N, out=_poisoned(M, N, dt), out_dtype=dt, **kw)
    else:
        want = ag.matmul(A, B, SFA, SFB, alpha, out=_poisoned(M, N, dt), out_dtype=dt, **kw)
    taken = 2 if (route == 1 and _misaligned(kw) and M <= 16) else route          # (a misaligned view skips route 1)
    if taken == 2 and _reference_kernel_is_lds_transposing(M, N, K):
        _check_g_prime(A, SFA, B, SFB, RW, RSF, N, alpha)
        return route
    assert torch.equal(got, want), (M, N, K, route)
    return route


def _misaligned(kw):
    return any(t is not None and t.data_ptr() % 8 for t in (kw.get("bias"), kw.get("residual")))


def _check_g_prime(A, SFA, B, SFB, RW, RSF, N, alpha):
    ag = _ag()
    M, K = A.shape[0], A.shape[1] * 2
    got = ag.matmul_rw(A, RW, SFA, RSF, alpha, N, out_dtype=torch.float32, out=_poisoned(M, N, torch.float32)).double()
    ref = ag.matmul(A, B, SFA, SFB, alpha, out_dtype=torch.float32).double()
    assert torch.isfinite(got).all()
    assert float((got - ref).norm() / ref.norm()) <= 1e-3, (M, N, K)
    if N * K <= 40_000_000:
        _, want = O.gemm(A.cpu().numpy(), B.cpu().numpy(), SFA.cpu().numpy(), SFB.cpu().numpy(), alpha)
        rel = np.linalg.norm(got.cpu().numpy() - want) / np.linalg.norm(want)
        assert rel <= 1e-3, (M, N, K, rel)


def test_route_one_equals_matmul_repacked():
    ag = _ag()
    for (M, N, KQ, KE) in [(1, 4096, 4096, 64), (4, 3584, 3584, 64), (16, 512, 4096, 64), (32, 4096, 4096, 64), (64, 1000, 2048, 64),
                           (8, 10752, 3584, 64)]:
        K = KQ + KE
        if not ag.repacked_supported(M, N, K):          # (only under a tuning override of the decode-batch kernels)
            assert M > 16 and os.environ.get("ARCQ_ROWTOK") == "0", (M, N, K)
            continue
        assert ag.rw_route(M, N, K) == 1
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE)
        g = torch.Generator(device=DEV).manual_seed(M)
        bias = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16)
        res = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
        for kw in ({}, {"bias": bias, "residual": res}, {"out_dtype": torch.float32}):
            assert _check_against_twin(A, SFA, B, SFB, RW, RSF, N, **kw) == 1


QWEN_DECODE = [(10752, 3584, 64), (3584, 3584, 64), (37888, 3584, 64), (3584, 18944, 64)]


@pytest.mark.parametrize("M", [1, 4, 16, 17, 32, 64, 128, 256, 512, 1024, 4096])
def test_every_m_matches_the_reference_layout_gemm_on_the_harness_shapes(M):
    ag = _ag()
    routes = set()
    shapes = [(4096, 4096, 64)] + QWEN_DECODE
    for i, (N, KQ, KE) in enumerate(shapes):
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=i)
        routes.add(_check_against_twin(A, SFA, B, SFB, RW, RSF, N))
        del A, SFA, B, SFB, RW, RSF
    if M >= 256:
        assert 3 in routes or 2 in routes
    assert routes <= {1, 2, 3}
    if M == 4096 and "ARCQ_REGTILE_CFG" not in os.environ:
        assert routes == {3}


def test_k_tails_ragged_n_and_epilogue_operands():
    """K % 256 in {64, 128, 192}, N not a multiple of 16 / 256, bias, residual (also aliasing D), fp32 output, device alpha."""
    ag = _ag()
    for (M, N, KQ, KE) in [(4, 100, 512, 64), (3, 777, 640, 0), (17, 1000, 704, 0), (40, 300, 576, 0), (129, 1000, 512, 64),
                           (300, 520, 1024, 64), (1024, 777, 640, 0), (2048, 1040, 1216, 64), (8, 2000, 8512, 0), (2, 300, 9024, 64)]:
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=3)
        g = torch.Generator(device=DEV).manual_seed(N)
        bias = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16)
        res = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
        dev_alpha = torch.tensor(0.25, dtype=torch.float32, device=DEV)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N, bias=bias, residual=res)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N, out_dtype=torch.float32, bias=bias)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N, alpha=dev_alpha, scale_host=1.5)
        K = KQ + KE
        if not (ag.rw_route(M, N, K) == 2 and _reference_kernel_is_lds_transposing(M, N, K)):
            # the residual aliasing D (`x + linear(x')` written in place), on both layouts
            d1, d2 = res.clone(), res.clone()
            ag.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=bias, residual=d1, out=d1)
            if ag.rw_route(M, N, K) == 1:
                ag.matmul_repacked(A, RW, SFA, RSF, 0.37, N, bias=bias, residual=d2, out=d2)
            else:
                ag.matmul(A, B, SFA, SFB, 0.37, bias=bias, residual=d2, out=d2)
            assert torch.equal(d1, d2), (M, N, K)


def test_split_k_and_misaligned_bias_views():
    ag = _ag()
    # split-K: the LDS-tiled kernel's fp32 partial planes (workspace) on both layouts
    for (M, N, KQ, KE) in [(1024, 1024, 16384, 0), (300, 256, 8192, 64)]:
        K = KQ + KE
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=5)
        if ag.rw_route(M, N, K) == 3:
            assert _lib().arcq_gemm_rw_workspace_bytes(M, N, K) == _lib().arcq_gemm_workspace_bytes(M, N, K)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N)
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N, out_dtype=torch.float32)
    if not any(v in os.environ for v in ("ARCQ_TILE_CFG", "ARCQ_TILE_SPLIT", "ARCQ_REGTILE_CFG")):      # (tuning overrides may not split)
        assert _lib().arcq_gemm_rw_workspace_bytes(1024, 1024, 16384) > 0
    # a bias view 2 bytes into its storage: route 1 is skipped (the decode kernels reject it), the tiled twin accepts it
    for (M, N, KQ, KE) in [(4, 4096, 4096, 64), (32, 1000, 2048, 64), (256, 4096, 4096, 64)]:
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=6)
        store = torch.randn(N + 8, device=DEV).to(torch.bfloat16)
        bias = store[1:N + 1]
        assert bias.data_ptr() % 8
        _check_against_twin(A, SFA, B, SFB, RW, RSF, N, bias=bias)
        with pytest.raises(RuntimeError):
            if ag.repacked_supported(M, N, KQ + KE):
                ag.matmul_repacked(A, RW, SFA, RSF, 0.37, N, bias=bias)
            else:
                raise RuntimeError("not a repacked shape")


def _lib():
    from arcquant_amd import _lib as L
    return L.lib()


def test_g_prime_shapes_match_the_oracle():
    """Decode shapes matmul serves with an LDS-transposing kernel: the register-tiled 16 x 16 configuration over RW instead."""
    ag = _ag()
    for (M, N, KQ, KE) in [(8, 3584, 18944, 64), (5, 3584, 18944, 64), (8, 256, 10240, 64), (7, 1000, 12288, 64)]:
        K = KQ + KE
        assert ag.rw_route(M, N, K) == 2
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=7)
        _check_g_prime(A, SFA, B, SFB, RW, RSF, N, 0.37)
        # bf16 with the epilogue operands: within the bar of matmul's own output
        g = torch.Generator(device=DEV).manual_seed(N)
        bias = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16)
        got = ag.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=bias, out=_poisoned(M, N, torch.bfloat16)).double()
        ref = ag.matmul(A, B, SFA, SFB, 0.37, bias=bias).double()
        assert float((got - ref).norm() / ref.norm()) <= 1e-3


def test_silu_mul_epilogue_over_rw_equals_the_reference_layout():
    ag = _ag()
    for (M, IT, KQ, KE) in [(17, 1024, 2048, 64), (64, 2560, 512, 64), (300, 1000, 1024, 0), (1024, 4096, 2048, 64)]:
        N = 2 * IT
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=8)
        g = torch.Generator(device=DEV).manual_seed(IT)
        bias = torch.randn(N, generator=g, device=DEV).to(torch.bfloat16)
        for b in (None, bias):
            act, slots = ag.matmul_rw_silu_mul(A, RW, SFA, RSF, 0.37, N, bias=b)
            act0, slots0 = ag.matmul_silu_mul(A, B, SFA, SFB, 0.37, bias=b)
            assert torch.equal(act, act0) and torch.equal(slots, slots0), (M, N)
    A, SFA, B, SFB, RW, RSF = _operands(16, 2048, 1024, 64, seed=9)
    with pytest.raises(RuntimeError):
        ag.matmul_rw_silu_mul(A, RW, SFA, RSF, 0.37, 2048)           # decode has its own repacked SiLU paths


def test_extension_module_returns_the_mirrors_bytes():
    from arcquant_amd import _build_ext
    ext = _build_ext.import_agemm_extension()
    ag = _ag()
    for (M, N, KQ, KE) in [(4, 4096, 4096, 64), (8, 3584, 18944, 64), (100, 1000, 1024, 64), (2048, 2048, 2048, 64)]:
        K = KQ + KE
        A, SFA, B, SFB, RW, RSF = _operands(M, N, KQ, KE, seed=10)
        assert ext.rw_route(M, N, K) == ag.rw_route(M, N, K)
        bias = torch.randn(N, device=DEV).to(torch.bfloat16)
        res = torch.randn(M, N, device=DEV).to(torch.bfloat16)
        assert torch.equal(ext.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=bias, residual=res),
                           ag.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=bias, residual=res))
        assert torch.equal(ext.matmul_rw(A, RW, SFA, RSF, 0.37, N, out_dtype=torch.float32),
                           ag.matmul_rw(A, RW, SFA, RSF, 0.37, N, out_dtype=torch.float32))
        QW, SFW = ext.unrepack_w(RW, RSF, N, K)
        QW2, SFW2 = ag.unrepack_w(RW, RSF, N, K)
        assert torch.equal(QW, QW2) and torch.equal(SFW, SFW2) and torch.equal(QW, B)
        used = torch.from_numpy(np.array([O.sf_offset(r, p, K) for r in range(0, N, max(1, N // 7)) for p in range(0, K // 16, 5)]))
        assert torch.equal(SFW[used.to(DEV)], SFB[used.to(DEV)])
        if M > 16 and N % 8 == 0:
            a1, s1 = ext.matmul_rw_silu_mul(A, RW, SFA, RSF, 0.37, N, bias=bias)
            a2, s2 = ag.matmul_rw_silu_mul(A, RW, SFA, RSF, 0.37, N, bias=bias)
            assert torch.equal(a1, a2) and torch.equal(s1, s2)
    # operands must share A's device: a CPU bias is refused before any launch
    with pytest.raises(RuntimeError):
        ext.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=torch.zeros(N, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError):
        ag.matmul_rw(A, RW, SFA, RSF, 0.37, N, bias=torch.zeros(N, dtype=torch.bfloat16))


def test_qlinear_layer_repacked_only_equals_the_two_copy_layer():
    from arcquant_amd import qlinear
    torch.manual_seed(0)
    lin = torch.nn.Linear(4096, 1000, bias=True).to(DEV).to(torch.bfloat16)
    idx = torch.randperm(4096)
    two = qlinear.QLinearLayer(lin, 64, idx, repack_for_decode=True)
    one = qlinear.QLinearLayer(lin, 64, idx, repacked_only=True)
    assert one.W is None and one.scale_w is None and two.W is not None
    assert torch.equal(one.RW, two.RW) and torch.equal(one.RSF, two.RSF)
    assert "W" not in {k for k, v in one.state_dict().items() if v is not None}
    for M in (1, 16, 17, 300):
        x = torch.randn(M, 4096, device=DEV).to(torch.bfloat16)
        qx, sx, s = qlinear.NVFP4_reorder_quantize_x(x, idx.to(DEV).to(torch.int16), 64)
        assert torch.equal(one((qx, sx, s, 1, M)), two((qx, sx, s, 1, M))), M
    QW, SFW = _ag().unrepack_w(one.RW, one.RSF, 1000, 4160)
    assert torch.equal(QW, two.W)


def _toy(hidden=2048, inter=4096, layers=2, heads=16):
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toy", num_layers=layers, num_heads=heads, hidden_size=hidden, intermediate_size=inter, vocab_size=512,
                                attention_bias=True, mlp_bias=True)


def test_e2e_repacked_only_decoder_equals_the_two_copy_model():
    e2e, cfg = _toy()
    ag = _ag()
    bsz, q_len = 2, 16
    h, it, ke = cfg.hidden_size, cfg.intermediate_size, cfg.select_num
    # every GEMM of this toy takes route 1, 2 or 3 with a bit-identical twin (no G' shape)
    for T in (bsz, bsz * q_len):
        for N, K in ((3 * h, h + ke), (h, h + ke), (2 * it, h + ke), (h, it + ke)):
            assert ag.rw_route(T, N, K) in (1, 2, 3) and not (ag.rw_route(T, N, K) == 2 and _reference_kernel_is_lds_transposing(T, N, K))
    tok = torch.randint(0, cfg.vocab_size, (bsz, q_len), device=DEV)
    nxt = torch.randint(0, cfg.vocab_size, (bsz, 1), device=DEV)
    with torch.no_grad():
        two = e2e.DecoderModel(cfg, bsz, 32, DEV, fused=True, attention="cache")
        one = e2e.DecoderModel(cfg, bsz, 32, DEV, fused=True, attention="cache", repacked_only=True)
        assert all(L[n].W is None and L[n].SFW is None for L in one.layers for n in ("qkv", "o", "gateup", "down"))
        assert one.weight_bytes() > 0 and one.weight_bytes() != two.weight_bytes()
        assert torch.equal(one.forward(tok, 0), two.forward(tok, 0))
        assert torch.equal(one.forward(nxt, q_len), two.forward(nxt, q_len))
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, bsz, 32, DEV, fused=False, repacked_only=True)


def test_e2e_repacked_only_decode_step_at_bs8_on_the_qwen_down_projection():
    """bs = 8, intermediate 18944: the down projection (8, 3584, 19008) is a G' shape -- the two-copy model served it from the
    reference-layout weight.  Its numerics are pinned above; here the model runs and holds no reference-layout copy."""
    e2e, cfg = _toy(hidden=3584, inter=18944, layers=1, heads=28)
    ag = _ag()
    assert ag.rw_route(8, 3584, 19008) == 2 and not ag.repacked_supported(8, 3584, 19008)
    with torch.no_grad():
        one = e2e.DecoderModel(cfg, 8, 8, DEV, fused=True, attention="cache", repacked_only=True)
        assert all(L[n].W is None for L in one.layers for n in ("qkv", "o", "gateup", "down"))
        nxt = torch.randint(0, cfg.vocab_size, (8, 1), device=DEV)
        out = one.forward(nxt, 0)
        assert out.shape == (8, cfg.vocab_size) and torch.isfinite(out.float()).all()
