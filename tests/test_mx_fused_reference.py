"""Pins tests/mx_fused_reference.py (the yardstick of the MXFP4 RMSNorm quantiser) to the committed C oracle: the restated normalised
rows, fed through the oracle's plain NVFP4 quantiser with the identity index, must give the bytes the oracle's fused
rmsnorm_quantize_x gives on the raw input.  Both oracle paths quantise the same row with the same rule, so a difference is a wrong row.
No product code is involved."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mx_fused_reference as F
from tests import mx_reference as R
from tests.util import bits, outlier_activations, random_perm


@pytest.mark.parametrize("variant", [O.G16, O.G32], ids=["G16", "G32"])
@pytest.mark.parametrize("M,KQ,KE", [(3, 2048, 64), (2, 3584, 256), (2, 4096, 64), (1, 8192, 0)])
def test_restated_rows_equal_the_oracle(M, KQ, KE, variant):
    import torch
    x = bits(outlier_activations(M, KQ, 31 + KQ))
    g = torch.Generator().manual_seed(KQ)
    w = bits((torch.rand(KQ, generator=g) + 0.5).to(torch.bfloat16))
    idx = random_perm(KQ, KQ + 1).numpy()
    eps = 1e-6
    rows = F.normalised_rows(x, w, eps, idx)
    row_bits = (np.ascontiguousarray(rows).view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(R.bf16_bits_to_f32(row_bits), rows)                         # already bf16 values
    got_q, got_sf = O.quantize_x(row_bits, np.arange(KQ, dtype=np.int16), KE, variant, sf_fill=0)
    want_q, want_sf = O.rmsnorm_quantize_x(x, w, eps, idx, KE, variant, sf_fill=0)
    assert np.array_equal(got_sf, want_sf), "scale bytes differ: the restated row is not the oracle's"
    assert np.array_equal(got_q, want_q), "codes differ: the restated row is not the oracle's"
    F.rmsnorm_quantize_x(x, w, eps, idx, KE)                                          # mx_reference accepts the rows (residual exact)
