"""CPU checks of the MXFP6 repacked weight: the layout MRW6 byte for byte against include/arcq.h's formula, and arcq_gemm_mxfp6_repacked's
rejections with their documented status before any HIP call (without a GPU a call that got as far as HIP would return ARCQ_ERR_LAUNCH)."""
import pytest
import torch

from arcquant_amd import _lib, agemm

SHAPE, NULL = -1, -4
P = 1 << 20                 # a 16-byte aligned stand-in address; never dereferenced (every call here fails validation or is empty)


@pytest.mark.parametrize("N,Kp", [(16, 128), (32, 1152), (16, 4224)])
def test_layout(N, Kp):
    g = torch.Generator().manual_seed(N + Kp)
    QW = torch.randint(0, 256, (N, 3 * Kp // 4), dtype=torch.uint8, generator=g)
    SFW = torch.randint(0, 256, (N, Kp // 32), dtype=torch.uint8, generator=g)
    MRW, MRSF = agemm.mx6_repack_w(QW, SFW)
    L = _lib.lib()
    assert (MRW.numel(), MRSF.numel()) == (L.arcq_mx6_repacked_w_bytes(N, Kp), L.arcq_mx_repacked_sf_bytes(N, Kp)) == (QW.numel(), MRSF.numel())
    assert torch.equal(MRSF, agemm.mx_repack_w(torch.zeros(N, Kp // 2, dtype=torch.uint8), SFW)[1])
    back = agemm.mx6_unrepack_w(MRW, MRSF, N, Kp)
    assert torch.equal(back[0], QW) and torch.equal(back[1], SFW)
    T = Kp // 128
    b, t, lane = torch.meshgrid(torch.arange(N // 16), torch.arange(T), torch.arange(64), indexing="ij")
    row, col, tile = 16 * b + (lane & 15), 96 * t + 24 * (lane >> 4), (b * T + t) * 1536
    for j in range(24):          # every byte of every lane's block: 0..15 in the first 1 KB of the tile, 16..23 in its last 512 bytes
        at = tile + 16 * lane + j if j < 16 else tile + 1024 + 8 * lane + j - 16
        assert torch.equal(MRW[at], QW[row, col + j]), j


def test_sizes_of_invalid_shapes():
    L = _lib.lib()
    assert [L.arcq_mx6_repacked_w_bytes(*s) for s in ((24, 128), (16, 192), (0, 128), (16, 0), (-16, 128))] == [0] * 5
    assert [L.arcq_gemm_mxfp6_repacked_supported(*s) for s in ((1, 16, 128), (64, 16, 128), (65, 16, 128), (0, 16, 128), (4, 24, 128), (4, 16, 192))] == [1, 1, 0, 0, 0, 0]
    assert agemm.MX6_REPACKED_MAX_M <= 64 and agemm.mx6_repacked_supported(agemm.MX6_REPACKED_MAX_M, 16, 128)


def _gemm(A=P, W=P, SA=P, SW=P, D=P, M=4, N=4096, K=4224, fmt=0, bias=None, res=None, out=0):
    return _lib.lib().arcq_gemm_mxfp6_repacked(A, W, SA, SW, D, M, N, K, fmt, 1.0, None, bias, res, out, None)


@pytest.mark.parametrize("kw,status", [
    (dict(M=65), SHAPE), (dict(M=-1), SHAPE), (dict(K=4160), SHAPE), (dict(K=0), SHAPE), (dict(N=4104), SHAPE), (dict(fmt=2), SHAPE),
    (dict(fmt=-1), SHAPE), (dict(out=2), SHAPE), (dict(A=P + 8), SHAPE), (dict(W=P + 8), SHAPE), (dict(D=P + 4), SHAPE), (dict(SA=P + 2), SHAPE),
    (dict(SW=P + 2), SHAPE), (dict(bias=P + 1), SHAPE), (dict(res=P + 1), SHAPE),
    (dict(A=None), NULL), (dict(W=None), NULL), (dict(SA=None), NULL), (dict(SW=None), NULL), (dict(D=None), NULL),
    (dict(M=0), 0), (dict(N=0), 0), (dict(M=0, fmt=1), 0), (dict(M=65, fmt=1), SHAPE), (dict(K=4160, fmt=1), SHAPE), (dict(W=None, fmt=1), NULL),
])
def test_gemm_rejects_before_any_hip_call(kw, status):
    assert _gemm(**kw) == status
    if status:
        assert b"arcq_gemm_mxfp6_repacked" in _lib.lib().arcq_last_error()


def test_python_and_layer_reject():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)      # noqa: E731
    A, SA = z(4, 96), z(4, 4)
    MRW, MRSF = agemm.mx6_repack_w(z(16, 96), z(16, 4))
    for bad in (dict(MRW=MRW[:-16]), dict(MRW=agemm.mx_repack_w(z(16, 64), z(16, 4))[0]), dict(N=32), dict(N=24), dict(b_format="e4m3"), dict(A=z(65, 96), SFA=z(65, 4))):
        a = dict(A=A, MRW=MRW, SFA=SA, MRSF=MRSF, N=16, b_format="e3m2") | bad
        with pytest.raises(RuntimeError):
            agemm.mx6_matmul_repacked(a["A"], a["MRW"], a["SFA"], a["MRSF"], 1.0, a["N"], b_format=a["b_format"])
    from arcquant_amd.qlinear import QLinearLayer
    for qt in ("NVFP4", "MXFP4"):
        with pytest.raises(ValueError):
            QLinearLayer(torch.nn.Linear(128, 32), 64, torch.arange(128), quant_type=qt, mx6_repack_for_decode=True)
