"""Audit of the MXFP4 decoder-layer kernels in the generated code (one compile each of quantize_mx.hip and gemm_mx.hip to gfx950
assembly, product flags): every new kernel runs without scratch and without VGPR spills; the SiLU*up GEMM variants are the block-scaled
fp4 MFMA kernels (v_mfma_scale_f32, no fp4 -> f16 dequantisation); and the plain mx_tile_kernel / mx_small_kernel instantiations, now
one value of a template parameter, keep the occupancy they had before that parameter existed.

Occupancy classes of the plain kernels, from a compile of the commit before this one: mx_tile_kernel 77 VGPRs + 64 AGPRs (144 allocated)
= 3 waves per SIMD, mx_small_kernel 52 VGPRs = 8 waves per SIMD.  Register counts may move inside a class."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

PLAIN, SILU = "ILi0E", "ILi1E"          # the kEpi template argument in the mangled kernel names
PARENT_WAVES = {"mx_tile_kernel": 3, "mx_small_kernel": 8}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _kernels(src):
    """{mangled name: (code text, metadata directives)} of every kernel in one source file."""
    text = assembly(src)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M):
        name = m.group(1)
        a = text.index("\n" + name + ":")
        out[name] = (text[a:m.start()], text[m.start():text.index(".end_amdhsa_kernel", m.start())])
    return out


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def _no_scratch(name, code, meta):
    assert _int(meta, "private_segment_fixed_size") == 0, f"{name}: scratch in use"
    assert not re.search(r"\bscratch_(load|store)", code), f"{name}: scratch access (a VGPR spill)"


def _waves_per_simd(meta):
    alloc = (_int(meta, "next_free_vgpr") + 7) // 8 * 8      # gfx950: 512 VGPRs (arch + acc) per SIMD lane, granules of 8
    return min(8, 512 // alloc)


def _one(kernels, stem, tag=""):
    hit = [n for n in kernels if stem in n and tag in n]
    assert len(hit) == 1, (stem, tag, sorted(kernels))
    return hit[0]


def test_fused_quantiser_kernels_use_no_scratch():
    ks = _kernels("quantize_mx.hip")
    fused = [n for n in ks if "mx_fused_rows_kernel" in n]
    assert len(fused) == 5, fused           # RMSNorm; SiLU*up in two layouts, each staged and direct
    for n in fused:
        _no_scratch(n, *ks[n])
    for n in ks:
        if "mx_quantize_rows_kernel" in n:
            _no_scratch(n, *ks[n])


def test_silu_mul_gemm_variants_and_the_plain_kernels():
    ks = _kernels("gemm_mx.hip")
    for stem in ("mx_tile_kernel", "mx_small_kernel"):
        silu = _one(ks, stem, SILU)
        code, meta = ks[silu]
        _no_scratch(silu, code, meta)
        assert "v_mfma_scale_f32" in code, f"{silu}: not on the block-scaled MFMA"
        assert "v_cvt_scalef32_pk_f16_fp4" not in code, f"{silu}: dequantises its operands"
        assert "quad_perm:[1,0,3,2]" in code and "quad_perm:[2,3,0,1]" in code, f"{silu}: the gate / up exchange is not DPP"
        assert not re.search(r"global_store_short\b", code), f"{silu}: 2-byte stores"
        plain = _one(ks, stem, PLAIN)
        code, meta = ks[plain]
        _no_scratch(plain, code, meta)
        assert "quad_perm" not in code and "v_exp_f32" not in code, f"{plain}: the SiLU epilogue leaked into the plain kernel"
        waves = _waves_per_simd(meta)
        print(f"{stem}: plain {_int(meta, 'next_free_vgpr')} VGPRs allocated = {waves} waves / SIMD; "
              f"silu_mul {_int(ks[silu][1], 'next_free_vgpr')} = {_waves_per_simd(ks[silu][1])}")
        assert waves == PARENT_WAVES[stem], f"{plain}: {waves} waves per SIMD, {PARENT_WAVES[stem]} before"
