"""Audit of the quantising gate|up GEMM kernels (arcq_gemm_mxfp4_silu_mul_quantize) in the generated code, from one compile of gemm_mx.hip
to gfx950 assembly with the product flags: the third kEpi value of mx_tile_kernel and mx_slice_quant_kernel run without scratch and
without VGPR spills, are block-scaled fp4 MFMA kernels (v_mfma_scale_f32, no fp4 -> f16 dequantisation), and the tile variant allocates no
more LDS than the plain tile kernel: its activation image lives in the staging buffers the K loop has finished with."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

PLAIN, QUANT = "ILi0E", "ILi2E"         # the kEpi template argument in the mangled kernel names

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def kernels():
    """{mangled name: (code text, metadata directives)} of every kernel in gemm_mx.hip."""
    text = assembly("gemm_mx.hip")
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M):
        name = m.group(1)
        a = text.index("\n" + name + ":")
        out[name] = (text[a:m.start()], text[m.start():text.index(".end_amdhsa_kernel", m.start())])
    return out


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def _one(kernels, stem, tag=""):
    hit = [n for n in kernels if stem in n and tag in n]
    assert len(hit) == 1, (stem, tag, sorted(kernels))
    return hit[0]


def _new_kernels(kernels):
    return [_one(kernels, "mx_tile_kernel", QUANT), _one(kernels, "mx_slice_quant_kernel")]


def test_quantising_kernels_use_no_scratch(kernels):
    for name in _new_kernels(kernels):
        code, meta = kernels[name]
        assert _int(meta, "private_segment_fixed_size") == 0, f"{name}: scratch in use"
        assert not re.search(r"\bscratch_(load|store)", code), f"{name}: scratch access (a VGPR spill)"
        print(f"{name}: {_int(meta, 'next_free_vgpr')} VGPRs allocated, {_int(meta, 'group_segment_fixed_size')} bytes of LDS")


def test_quantising_kernels_are_scaled_mfma_kernels(kernels):
    for name in _new_kernels(kernels):
        code, _ = kernels[name]
        assert "v_mfma_scale_f32" in code, f"{name}: not on the block-scaled MFMA"
        assert "v_cvt_scalef32_pk_f16_fp4" not in code, f"{name}: dequantises its operands"


def test_tile_variant_reuses_the_staging_buffers(kernels):
    quant = _int(kernels[_one(kernels, "mx_tile_kernel", QUANT)][1], "group_segment_fixed_size")
    plain = _int(kernels[_one(kernels, "mx_tile_kernel", PLAIN)][1], "group_segment_fixed_size")
    assert 0 < quant <= plain, (quant, plain)
