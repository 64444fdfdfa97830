"""CPU tests of the one-copy weight path (include/arcq.h, "every M over the REPACKED weight"): repack_w / unrepack_w are exact
inverses, arcq_gemm_rw_route follows its documented dispatch contract, and the new entry points validate before any HIP call.
No kernel is launched."""
import pytest
import torch

from arcquant_amd import _lib, agemm

P = 4096          # a fake, 16-byte aligned device pointer: never dereferenced on these paths

# the harness's Qwen2.5-7B / Llama-3.1-8B GEMMs (KE = 64): q|k|v, o, gate|up, down
QWEN = [(3 * 3584, 3584 + 64), (3584, 3584 + 64), (2 * 18944, 3584 + 64), (3584, 18944 + 64)]
LLAMA = [(3 * 4096, 4096 + 64), (4096, 4096 + 64), (2 * 14336, 4096 + 64), (4096, 14336 + 64)]


def _random_weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    QW = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    SFW = torch.zeros(agemm.sf_buffer_bytes(N, K), dtype=torch.uint8)
    # every byte of the swizzled image of N rows random, the rest of the buffer zero (what unrepack_w rebuilds)
    off = agemm._sf_swizzle_offsets(N, K, "cpu")
    SFW[off] = torch.randint(1, 256, tuple(off.shape), generator=g, dtype=torch.uint8)
    return QW, SFW


@pytest.mark.parametrize("N,K", [(16, 256), (37, 64), (100, 320), (129, 448), (300, 704), (17, 4160), (256, 3648)])
def test_repack_unrepack_round_trip_is_byte_exact(N, K):
    QW, SFW = _random_weight(N, K, N * 7 + K)
    RW, RSF = agemm.repack_w(QW, SFW)
    assert RW.device.type == "cpu" and RW.numel() == _lib.lib().arcq_repacked_w_bytes(N, K)
    QW2, SFW2 = agemm.unrepack_w(RW, RSF, N, K)
    assert QW2.dtype == torch.uint8 and tuple(QW2.shape) == (N, K // 2) and QW2.is_contiguous()
    assert SFW2.numel() == agemm.sf_buffer_bytes(N, K)
    assert torch.equal(QW2, QW) and torch.equal(SFW2, SFW)
    # and back again: the repacked bytes are a function of the weight alone
    RW2, RSF2 = agemm.repack_w(QW2, SFW2)
    assert torch.equal(RW2, RW) and torch.equal(RSF2, RSF)


def test_round_trip_covers_ragged_n_and_every_k_tail():
    for N in (1, 15, 33):
        for tail in (64, 128, 192):
            K = 256 + tail
            QW, SFW = _random_weight(N, K, N + tail)
            QW2, SFW2 = agemm.unrepack_w(*agemm.repack_w(QW, SFW), N, K)
            assert torch.equal(QW2, QW) and torch.equal(SFW2, SFW), (N, K)


def test_unrepack_rejects_a_foreign_weight():
    RW, RSF = agemm.repack_w(*_random_weight(32, 256, 1))
    with pytest.raises(RuntimeError):
        agemm.unrepack_w(RW, RSF, 48, 256)
    with pytest.raises(RuntimeError):
        agemm.unrepack_w(RW, RSF, 32, 512)


def test_route_one_is_exactly_the_repacked_decode_path():
    L = _lib.lib()
    for N, K in QWEN + LLAMA + [(4096, 4096), (512, 4160), (10752, 3648), (37888, 3648)]:
        for M in list(range(1, 20)) + [24, 31, 32, 33, 48, 63, 64, 65, 96, 127, 128, 129, 130, 256]:
            sup = L.arcq_gemm_repacked_supported(M, N, K)
            assert (L.arcq_gemm_rw_route(M, N, K) == 1) == (sup == 1), (M, N, K)


def test_route_is_never_zero_over_the_harness_shapes():
    L = _lib.lib()
    Ms = sorted(set([1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 24, 32, 48, 64, 96, 128, 129, 192, 256, 384, 512, 768, 1024, 1536, 2048,
                     3072, 4096, 6144, 8192]))
    for N, K in QWEN + LLAMA + [(4096, 4096), (4096, 4160)]:
        for M in Ms:
            assert L.arcq_gemm_rw_route(M, N, K) in (1, 2, 3), (M, N, K)
    # the shapes the two-copy model served from the reference-layout weight at decode (ISSUE: down projection at bs = 8, the widest gate|up)
    for M in (5, 6, 7, 8):
        assert L.arcq_gemm_rw_route(M, 3584, 19008) == 2
    assert L.arcq_gemm_rw_route(64, 37888, 3648) == 2
    assert L.arcq_gemm_rw_route(129, 4096, 4160) in (2, 3)
    assert L.arcq_gemm_rw_route(4096, 3584, 3648) == 3


def test_route_zero_for_invalid_shapes():
    L = _lib.lib()
    assert L.arcq_gemm_rw_route(0, 4096, 4096) == 0
    assert L.arcq_gemm_rw_route(4, 0, 4096) == 0
    assert L.arcq_gemm_rw_route(4, 4096, 4100) == 0
    assert L.arcq_gemm_rw_workspace_bytes(0, 4096, 4096) == 0


def test_workspace_equals_the_reference_layout_call_on_the_tiled_route():
    L = _lib.lib()
    seen3 = 0
    for N, K in QWEN + LLAMA + [(4096, 4096), (4096, 4160), (1024, 16384)]:
        for M in (17, 32, 64, 129, 256, 512, 1024, 2048, 4096, 8192):
            r = L.arcq_gemm_rw_route(M, N, K)
            if r == 3:
                seen3 += 1
                assert L.arcq_gemm_rw_workspace_bytes(M, N, K) == L.arcq_gemm_workspace_bytes(M, N, K), (M, N, K)
            elif r == 2:
                assert L.arcq_gemm_rw_workspace_bytes(M, N, K) == 0
    assert seen3 > 10
    # a split-K shape: the partial planes are the same on both layouts
    assert L.arcq_gemm_rw_route(1024, 1024, 16384) == 3 and L.arcq_gemm_rw_workspace_bytes(1024, 1024, 16384) > 0
    # a route-1 shape called with a misaligned bias view takes the tiled route: the workspace covers that call too
    assert L.arcq_gemm_rw_route(32, 1000, 2112) == 1 and L.arcq_gemm_rw_workspace_bytes(32, 1000, 2112) == L.arcq_gemm_workspace_bytes(32, 1000, 2112)


def test_mirror_route_matches_the_library():
    assert agemm.rw_route(8, 3584, 19008) == 2 and agemm.rw_route(4, 4096, 4160) == 1 and agemm.rw_route(4096, 4096, 4096) == 3


def test_rw_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    f = L.arcq_gemm_nvfp4_rw
    # M = 0 / N = 0: nothing to do, even with NULL pointers
    assert f(None, None, None, None, None, 0, 4096, 4160, 1.0, None, None, None, 0, None, 0, None) == 0
    assert f(None, None, None, None, None, 4, 0, 4160, 1.0, None, None, None, 0, None, 0, None) == 0
    assert f(P, P, P, P, P, 4, 4096, 4100, 1.0, None, None, None, 0, None, 0, None) == -1 and b"K % 64" in L.arcq_last_error()
    assert f(P, P, P, P, P, 4, 4096, 4160, 1.0, None, None, None, 7, None, 0, None) == -1                    # out_dtype
    assert f(P, None, P, P, P, 4, 4096, 4160, 1.0, None, None, None, 0, None, 0, None) == -4                 # NULL RW
    assert f(P, P, P, None, P, 4, 4096, 4160, 1.0, None, None, None, 0, None, 0, None) == -4                 # NULL RSF
    assert f(P, P + 8, P, P, P, 4, 4096, 4160, 1.0, None, None, None, 0, None, 0, None) == -1 and b"16-byte" in L.arcq_last_error()
    assert f(P, P, P, P + 2, P, 4, 4096, 4160, 1.0, None, None, None, 0, None, 0, None) == -1 and b"4-byte" in L.arcq_last_error()
    s = L.arcq_gemm_nvfp4_rw_silu_mul
    assert s(None, None, None, None, None, None, 0, 8192, 4160, 1.0, None, None, None) == 0
    assert s(P, P, P, P, P, P, 16, 8192, 4160, 1.0, None, None, None) == -2 and b"M <= 16" in L.arcq_last_error()
    assert s(P, P, P, P, P, P, 1, 8192, 4160, 1.0, None, None, None) == -2
    assert s(P, P, P, P, P, P, 32, 8192, 4100, 1.0, None, None, None) == -1
    assert s(P, P, P, P, P, P, 32, 8196, 4160, 1.0, None, None, None) == -1                                 # N % 8
    assert s(P, None, P, P, P, P, 32, 8192, 4160, 1.0, None, None, None) == -4
    assert s(P, P, P, P, P, None, 32, 8192, 4160, 1.0, None, None, None) == -4                              # absmax_slots
    assert s(P, P, P, P, P + 8, P, 32, 8192, 4160, 1.0, None, None, None) == -1 and b"16-byte" in L.arcq_last_error()
    assert s(P, P, P, P, P, P + 2, 32, 8192, 4160, 1.0, None, None, None) == -1 and b"4-byte" in L.arcq_last_error()
    assert L.arcq_gemm_rw_silu_mul_slots(16, 8192, 4160) == 0
    assert L.arcq_gemm_rw_silu_mul_slots(64, 8192, 4160) == L.arcq_gemm_silu_mul_slots(64, 8192, 4160)


def test_qlinear_and_decoder_reject_what_they_cannot_do():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toy", num_layers=1, num_heads=4, hidden_size=256, intermediate_size=512, vocab_size=64)
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 1, 8, torch.device("cpu"), fused=False, repacked_only=True)
