"""CPU tests of tests/kv_reference.py, the restatement of the paged KV-cache format the GPU tests compare with: nibble order, the offset
formulas of page.cuh against a brute-force 6-D index, and the quantiser's edge rows, settled against torch itself."""
import numpy as np
import pytest
import torch

from arcquant_amd import kvcache
from tests import kv_reference as R


def test_pack_unpack_roundtrip_and_nibble_order():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, size=(5, 3, 128), dtype=np.uint8)
    packed = R.pack_codes(codes)
    assert packed.shape == (5, 3, 64) and np.array_equal(R.unpack_codes(packed), codes)
    one = np.zeros(128, dtype=np.uint8)
    one[6], one[7] = 3, 9                                   # byte 3: element 6 low, element 7 high
    assert R.pack_codes(one)[3] == 0x93 and R.pack_codes(one).sum() == 0x93
    # the library's torch pair agrees with the numpy one
    q = torch.from_numpy(packed)
    s, z = torch.full((5, 3, 1), 0.5, dtype=torch.float16), torch.full((5, 3, 1), 2.0, dtype=torch.float16)
    want = R.dequantize_f32(packed, torch.cat([s, z], -1).numpy())
    assert np.array_equal(kvcache.unpack_i4_and_asym_dequantize(q, s.float(), z.float()).numpy(), want)


@pytest.mark.parametrize("row", [64, 128, 2])
def test_offsets_match_a_brute_force_index(row):
    pages, L, N, P = 3, 2, 3, 5
    flat = np.arange(pages * L * 2 * N * P * row).reshape(pages, L, 2, N, P, row)
    for page in range(pages):
        for layer in range(L):
            for head in range(N):
                for e in (0, 1, P - 1):
                    for f in (0, row - 1):
                        assert R.k_elem_offset(page, head, e, f, L, layer, N, P, row) == flat[page, layer, 0, head, e, f]
                        assert R.v_elem_offset(page, head, e, f, L, layer, N, P, row) == flat[page, layer, 1, head, e, f]


def test_sequence_lengths_and_locate():
    P = 5
    indptr, indices, last = [0, 1, 3, 6], [4, 0, 2, 5, 1, 3], [5, 1, 3]
    assert R.seq_lens(indptr, last, P).tolist() == [5, 6, 13]
    assert R.locate(indptr, indices, 1, 5, P) == (2, 0) and R.locate(indptr, indices, 2, 12, P) == (3, 2) and R.locate(indptr, indices, 0, 4, P) == (4, 4)


def _edge_rows(dtype):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(64, 128, generator=g) * 3).to(dtype)
    x[0] = 1.5                                               # constant row: range 0 -> clamp
    x[1] = 0
    x[2] = torch.linspace(0, 4e-6, 128).to(dtype)            # range below 1e-5
    x[3] = 1.0
    x[3, 5] = 1.0 + (2.0 ** -10 if dtype is torch.float16 else 2.0 ** -7)       # one ulp of range
    if dtype is torch.float16:
        x[4, 3], x[5, 7] = 65504, -65504
        x[6, 1], x[6, 2] = 65504, -65504                     # the range overflows fp16: scale = inf
    return x


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantiser_edge_rows_against_torch(dtype):
    """The rule is what torch computes; the stepwise form (every operation rounded to the input dtype, the Scalar 1e-5 included) is what
    the kernel implements.  They agree byte for byte, the degenerate rows included, and so does the library's torch quantiser."""
    x = _edge_rows(dtype)
    packed, param = R.quantize_i4(x)
    packed2, param2 = R.quantize_i4_stepwise(x)
    assert torch.equal(packed, packed2)
    assert torch.equal(param.view(torch.int16), param2.view(torch.int16))
    ours, scale, zero = kvcache.asym_quantize_and_pack_i4(x)
    finite = torch.isfinite(scale[:, 0])                     # (a NaN's cast to uint8 is the platform's; the reference defines it as 0)
    assert torch.equal(ours[finite], packed[finite]) and torch.equal(torch.cat([scale, zero], -1).to(torch.float16).view(torch.int16), param.view(torch.int16))
    # constant row: the clamp decides -- scale = dtype(1e-5) / 15, every code 0
    assert packed[0].eq(0).all() and float(param[0, 0]) > 0 and float(param[0, 1]) == -1.5
    # a range below 1e-5 is quantised with the clamped scale: codes stay below 15
    assert int(R.unpack_codes(packed[2].numpy()).max()) < 15
    assert float(param[2, 0]) == float(param[0, 0])
    # an ordinary row reaches both ends
    c = R.unpack_codes(packed[10].numpy())
    assert c.min() == 0 and c.max() == 15
    # round trip error of an ordinary row: half a step
    back = R.dequantize_f32(packed[10].numpy(), param[10].numpy())
    step = float(param[10, 0])
    assert np.abs(back - x[10].float().numpy()).max() <= 0.5 * step * 1.02 + 2.0 ** -7 * float(x[10].abs().max())


def test_writers_and_attention_walk_the_tables():
    """write_rows places the last tokens of a sequence; the fp64 attention over one position returns the dequantised V row."""
    P, L, N = 5, 2, 2
    data = np.full((4, L, 2, N, P, 64), 0xEE, dtype=np.uint8)
    param = np.full((4, L, 2, N, P, 2), 7.0, dtype=np.float16)
    indptr, indices, last = np.array([0, 2, 3]), np.array([3, 1, 0]), np.array([2, 1])
    x = (torch.randn(4, N, 128) * 3).to(torch.float16)
    kq, kp = R.quantize_i4(x)
    vq, vp = R.quantize_i4(-x)
    written = R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), np.array([0, 3, 4]), 1)
    assert written == [(3, 4), (1, 0), (1, 1), (0, 0)]       # sequence 0: positions 4, 5, 6 of 7; sequence 1: position 0
    assert (data[:, 0] == 0xEE).all() and (data[2] == 0xEE).all() and (data[0, 1, :, :, 1:] == 0xEE).all()
    q = np.random.default_rng(1).standard_normal((2, 2 * N, 128))
    out, (spa, qa) = R.paged_attention_f64(q, data, param, indptr, indices, last, 1)
    want = R.dequantize_f32(vq[3].numpy(), vp[3].numpy()).astype(np.float64)
    assert np.array_equal(out[1, 0], want[0]) and np.array_equal(out[1, 1], want[0]) and np.array_equal(out[1, 3], want[1])
    assert (R.decode_bound(out, spa, qa, 2.0 ** -11) > 0).all()
