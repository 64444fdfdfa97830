"""The MXFP4 repacked weight (include/arcq.h "MXFP4 repacked weight") on the CPU: agemm.mx_repack_w against the header's index formulas
written out as plain loops, its inverse, the two size functions and the rejections.  Random bytes: the repack is pure data movement and
must not care what the bytes mean."""
import numpy as np
import pytest
import torch

from arcquant_amd import _lib, agemm

SHAPES = [(N, K) for N in (16, 48) for K in (128, 1152, 4224)]      # 1, 9 and 33 steps: a partial MRSF round and a second round
PAD = 127                                                          # arcq.h: the padding bytes of a partial round
_cache = {}


def _weight(N, K):
    """(QW, SFW, MRW, MRSF) as numpy arrays, repacked once per shape."""
    if (N, K) not in _cache:
        rng = np.random.default_rng(N * 7 + K)
        QW = rng.integers(0, 256, (N, K // 2), dtype=np.uint8)
        SFW = rng.integers(0, 255, (N, K // 32), dtype=np.uint8)
        MRW, MRSF = agemm.mx_repack_w(torch.from_numpy(QW), torch.from_numpy(SFW))
        _cache[(N, K)] = (QW, SFW, MRW.numpy(), MRSF.numpy())
    return _cache[(N, K)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_repack_matches_the_header_formula(N, K):
    QW, SFW, MRW, MRSF = _weight(N, K)
    T = K // 128
    R = -(-T // 32)
    want_w = np.zeros(N * K // 2, dtype=np.uint8)
    want_sf = np.full((N // 16) * R * 2048, PAD, dtype=np.uint8)
    for n in range(N):
        b, r = n // 16, n % 16
        for t in range(T):
            for q in range(4):
                lane = 16 * q + r
                for j in range(16):
                    want_w[((b * T + t) * 64 + lane) * 16 + j] = QW[n, 64 * t + 16 * q + j]
                want_sf[(((b * R + t // 32) * 8 + t % 8) * 64 + lane) * 4 + (t // 8) % 4] = SFW[n, 4 * t + q]
    assert np.array_equal(MRW, want_w)
    assert np.array_equal(MRSF, want_sf)
    # the padding is exactly the steps that do not exist
    assert int((want_sf == PAD).sum()) >= (N // 16) * (R * 32 - T) * 64


@pytest.mark.parametrize("N,K", SHAPES)
def test_sizes_and_inverse(N, K):
    QW, SFW, MRW, MRSF = _weight(N, K)
    L = _lib.lib()
    assert MRW.size == N * K // 2 == L.arcq_mx_repacked_w_bytes(N, K)
    assert MRSF.size == (N // 16) * -(-K // 4096) * 2048 == L.arcq_mx_repacked_sf_bytes(N, K)
    q, s = agemm.mx_unrepack_w(torch.from_numpy(MRW), torch.from_numpy(MRSF), N, K)
    assert q.shape == (N, K // 2) and s.shape == (N, K // 32)
    assert np.array_equal(q.numpy(), QW) and np.array_equal(s.numpy(), SFW)


def test_size_functions_and_predicate_outside_the_contract():
    L = _lib.lib()
    for N, K in [(0, 128), (16, 0), (24, 128), (16, 192), (-16, 128), (16, -128)]:
        assert L.arcq_mx_repacked_w_bytes(N, K) == 0 and L.arcq_mx_repacked_sf_bytes(N, K) == 0, (N, K)
    ok = agemm.mx_repacked_supported
    assert ok(1, 16, 128) and ok(64, 48, 4224) and ok(17, 37888, 3584 + 128)
    assert not ok(0, 16, 128) and not ok(65, 16, 128) and not ok(4, 24, 128) and not ok(4, 16, 192) and not ok(-1, 16, 128)
    assert agemm.MX_REPACKED_MAX_M == 64


def test_rejections():
    QW, SFW = torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(16, 4, dtype=torch.uint8)
    MRW, MRSF = agemm.mx_repack_w(QW, SFW)
    bad = (RuntimeError, ValueError)
    with pytest.raises(bad, match="multiple of 16"):
        agemm.mx_repack_w(torch.zeros(24, 64, dtype=torch.uint8), torch.zeros(24, 4, dtype=torch.uint8))
    with pytest.raises(bad, match="multiple of 128"):
        agemm.mx_repack_w(torch.zeros(16, 96, dtype=torch.uint8), torch.zeros(16, 6, dtype=torch.uint8))
    with pytest.raises(bad, match="SFW"):
        agemm.mx_repack_w(QW, torch.zeros(16, 8, dtype=torch.uint8))
    with pytest.raises(bad, match="SFW"):
        agemm.mx_repack_w(QW, torch.zeros(8, 4, dtype=torch.uint8))
    with pytest.raises(bad, match="QW"):
        agemm.mx_repack_w(QW.to(torch.int8), SFW)
    with pytest.raises(bad, match="SFW"):
        agemm.mx_repack_w(QW, SFW.to(torch.int16))
    with pytest.raises(bad, match="QW"):
        agemm.mx_repack_w(QW.reshape(-1), SFW)
    with pytest.raises(bad, match="MRW"):
        agemm.mx_unrepack_w(MRW.to(torch.int8), MRSF, 16, 128)
    with pytest.raises(bad, match="MRSF"):
        agemm.mx_unrepack_w(MRW, MRSF.to(torch.float32), 16, 128)
    for N, K in [(24, 128), (16, 192), (32, 128), (16, 256), (0, 128)]:        # divisibility, then sizes that belong to another weight
        with pytest.raises(bad, match="do not belong"):
            agemm.mx_unrepack_w(MRW, MRSF, N, K)
    with pytest.raises(bad, match="do not belong"):
        agemm.mx_unrepack_w(MRW, MRSF[:-4].contiguous(), 16, 128)
