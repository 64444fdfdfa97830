"""Audit of the MXFP4 kernels that serve every batch size from the repacked weight, in the generated code (one compile each of
gemm_mx_tile_rw.hip, gemm_mx_slice_rw.hip and, for comparison, gemm_mx.hip to gfx950 assembly, product flags).

The new units hold exactly the expected kernels: mx_tile_rw_kernel<kEpi> for the three epilogues, and mx_slice_rw_quant_kernel.  The tile
kernels multiply on the scaled 32x32x64 fp4 MFMA and on nothing else, never dequantise an operand, have no fp16 MFMA and no scratch, hold
no more LDS than mx_tile_kernel's plain instantiation and sit in its occupancy class (3 waves per SIMD: 156 VGPRs allocated against 144 --
the scale gather's three further dwords and the second pair of LDS offsets).  The slice kernel multiplies on the 16x16x128 form alone,
uses no scratch, and requests MRW as 16-byte non-temporal loads (104 VGPRs: two workgroups per CU, the partial sums' 34 KB of LDS allow
four)."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

TILE_UNIT, SLICE_UNIT, REF_UNIT = "gemm_mx_tile_rw.hip", "gemm_mx_slice_rw.hip", "gemm_mx.hip"
EPILOGUES = {0: "plain", 1: "silu_mul", 2: "silu_mul_quantize"}
TILE_WAVES_PER_SIMD = 3                 # mx_tile_kernel's class (tests/test_mx_fused_isa.py)
FORBIDDEN_STEMS = ("mx_tile_kernel", "mx_small_kernel", "mx_slice_quant_kernel", "mx_rw_kernel")    # what the audits of the other units count


def _kernels(unit):
    """{mangled name: (code text, metadata directives)} of every kernel in one source file."""
    text = assembly(TILE_UNIT, SLICE_UNIT, REF_UNIT) if unit == TILE_UNIT else assembly(unit)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M):
        name = m.group(1)
        a = text.index("\n" + name + ":")
        out[name] = (text[a:m.start()], text[m.start():text.index(".end_amdhsa_kernel", m.start())])
    return out


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def _waves_per_simd(meta):
    alloc = (_int(meta, "next_free_vgpr") + 7) // 8 * 8      # gfx950: 512 VGPRs (arch + acc) per SIMD lane, granules of 8
    return min(8, 512 // alloc)


def _no_scratch(who, code, meta):
    assert _int(meta, "private_segment_fixed_size") == 0, f"{who}: scratch in use"
    assert not re.search(r"\bscratch_(load|store)", code), f"{who}: scratch access (a VGPR spill)"


def _tile_kernels():
    out = {}
    for name, km in _kernels(TILE_UNIT).items():
        k = re.search(r"mx_tile_rw_kernelILi(\d)EE", name)
        assert k, f"unexpected kernel {name} in {TILE_UNIT}"
        out[int(k.group(1))] = km
    return out


def test_the_new_units_hold_exactly_the_expected_kernels():
    assert sorted(_tile_kernels()) == sorted(EPILOGUES)
    assert len(_kernels(TILE_UNIT)) == len(EPILOGUES)
    names = list(_kernels(SLICE_UNIT))
    assert len(names) == 1 and "mx_slice_rw_quant_kernel" in names[0], names
    for name in list(_kernels(TILE_UNIT)) + names:              # the other units' audits count kernels by these stems
        assert not any(stem in name for stem in FORBIDDEN_STEMS), name


@pytest.mark.parametrize("epi", sorted(EPILOGUES))
def test_tile_kernel_is_the_scaled_fp4_mfma_kernel(epi):
    code, meta = _tile_kernels()[epi]
    who = f"mx_tile_rw_kernel<{EPILOGUES[epi]}>"
    mfma = re.findall(r"^\s*(v_mfma\w+)", code, flags=re.M)
    assert mfma and set(mfma) == {"v_mfma_scale_f32_32x32x64_f8f6f4"}, f"{who}: {sorted(set(mfma))}"
    assert "cbsz:4" in code and "blgp:4" in code, f"{who}: the operands are not declared fp4"
    # no v_cvt_scalef32 at all -- except, in the quantising kernel, the quantiser's own f32 -> fp4 conversion of its OUTPUT
    # (mx_store_x_block, the instruction arcq_mx_quantize_x writes the same bytes with): nothing converts FROM fp4 anywhere
    cvt = set(re.findall(r"^\s*(v_cvt_scalef32\w+)", code, flags=re.M))
    assert cvt == ({"v_cvt_scalef32_pk_fp4_f32"} if epi == 2 else set()), f"{who}: {sorted(cvt)}: dequantises an operand"
    assert not re.search(r"v_mfma_f32_\w*f16", code), f"{who}: an fp16 MFMA"
    _no_scratch(who, code, meta)
    if epi == 0:
        assert "quad_perm" not in code and "v_exp_f32" not in code, f"{who}: the SiLU epilogue leaked into the plain kernel"
    else:
        assert "quad_perm:[1,0,3,2]" in code and "quad_perm:[2,3,0,1]" in code, f"{who}: the gate / up exchange is not DPP"


def test_tile_kernel_lds_and_occupancy_against_the_reference_layout_kernel():
    ref = [km for name, km in _kernels(REF_UNIT).items() if "mx_tile_kernelILi0E" in name]
    assert len(ref) == 1
    ref_lds, ref_waves = _int(ref[0][1], "group_segment_fixed_size"), _waves_per_simd(ref[0][1])
    assert ref_waves == TILE_WAVES_PER_SIMD
    for epi, (code, meta) in _tile_kernels().items():
        who = f"mx_tile_rw_kernel<{EPILOGUES[epi]}>"
        lds, waves = _int(meta, "group_segment_fixed_size"), _waves_per_simd(meta)
        print(f"{who}: {_int(meta, 'next_free_vgpr')} VGPRs allocated = {waves} waves / SIMD; {lds} bytes of LDS (mx_tile_kernel: {ref_lds})")
        assert lds <= ref_lds, f"{who}: {lds} bytes of LDS, mx_tile_kernel {ref_lds}"
        assert waves == TILE_WAVES_PER_SIMD, f"{who}: {waves} waves per SIMD, mx_tile_kernel's class is {TILE_WAVES_PER_SIMD}"
        assert lds * waves <= 160 * 1024, f"{who}: LDS, not registers, bounds the occupancy"


def test_tile_kernel_fetches_whole_spans_and_gathers_the_scale_bytes():
    """Per K step a thread requests two 16-byte chunks of A, two of MRW (its wave's two 1 KB spans) and four dwords (the scale gather); the
    K loop holds one such set."""
    for epi, (code, meta) in _tile_kernels().items():
        who = f"mx_tile_rw_kernel<{EPILOGUES[epi]}>"
        x4 = len(re.findall(r"global_load_dwordx4 ", code))
        x1 = len(re.findall(r"global_load_dword ", code))
        assert x4 == 8 and x1 >= 8, f"{who}: {x4} 16-byte and {x1} dword loads (prologue + loop: 2 x 4 and 2 x 4)"
        assert not re.search(r"ds_write_b8\b", code), f"{who}: the scale bytes are scattered, not assembled"


def test_slice_kernel():
    (name, (code, meta)), = _kernels(SLICE_UNIT).items()
    who = "mx_slice_rw_quant_kernel"
    mfma = re.findall(r"^\s*(v_mfma\w+)", code, flags=re.M)
    assert mfma and set(mfma) == {"v_mfma_scale_f32_16x16x128_f8f6f4"}, f"{who}: {sorted(set(mfma))}"
    assert len(mfma) == 16, f"{who}: {len(mfma)} MFMAs for 4 steps x 4 row blocks"
    assert "cbsz:4" in code and "blgp:4" in code, f"{who}: the operands are not declared fp4"
    assert "v_cvt_scalef32_pk_f16_fp4" not in code and not re.search(r"v_mfma_f32_\w*f16", code), f"{who}: dequantises an operand"
    _no_scratch(who, code, meta)
    nt4 = re.findall(r"global_load_dwordx4 .* nt\b", code)
    nt1 = re.findall(r"global_load_dword .* nt\b", code)
    assert len(nt4) == 16 and len(nt1) == 4, f"{who}: {len(nt4)} x4 and {len(nt1)} dword non-temporal loads (4 steps x 4 row blocks; 4 MRSF dwords)"
    assert len(re.findall(r"global_load_dwordx4 ", code)) == 16 + 4, f"{who}: an A fragment is not one request per step"
    vgprs, lds = _int(meta, "next_free_vgpr"), _int(meta, "group_segment_fixed_size")
    waves = _waves_per_simd(meta)
    print(f"{who}: {vgprs} VGPRs = {waves} waves / SIMD = {waves // 2} workgroups / CU; {lds} bytes of LDS")
    assert waves >= 4, f"{who}: {vgprs} VGPRs = {waves} waves per SIMD: one workgroup per CU"
    assert lds == 8 * 4 * 64 * 16 + 16 * 80, f"{who}: {lds} bytes of LDS"       # the partial sums and the activation rows
    assert lds * (waves // 2) <= 160 * 1024, f"{who}: LDS, not registers, bounds the occupancy"
