"""Audit of the MXFP4 repacked decode kernels in the generated code (one compile of gemm_mx_rw.hip to gfx950 assembly, product flags):
every instantiation of mx_rw_kernel -- two epilogues x kF = 1 .. 4 A fragments -- multiplies on the scaled 16x16x128 fp4 MFMA, never
dequantises an operand and has no fp16 MFMA, runs without scratch or spills, loads the weight as 16-byte-per-lane non-temporal requests,
and keeps the occupancy it was written for.

Registers: 51 / 78 / 99 / 128 VGPRs for kF = 1 / 2 / 3 / 4 with either epilogue, that is 8 / 6 / 4 / 4 waves per SIMD.  A
workgroup is 8 waves = 2 per SIMD, so 4 / 3 / 2 / 2 workgroups share a CU.  kF = 4 sits exactly on the 128-register line that the
kernel's launch bound asks for (131 without it, and then one workgroup per CU).  Counts may move inside a class; the class is pinned."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

WAVES_PER_SIMD = {1: 8, 2: 6, 3: 4, 4: 4}
EPILOGUES = {0: "plain", 1: "silu_mul"}


def _kernels():
    """{(kEpi, kF): (code, metadata)} of every mx_rw_kernel instantiation."""
    text = assembly("gemm_mx_rw.hip")
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M):
        name = m.group(1)
        k = re.search(r"mx_rw_kernelILi(\d)ELi(\d)EE", name)
        assert k, f"unexpected kernel {name} in gemm_mx_rw.hip"
        a = text.index("\n" + name + ":")
        out[(int(k.group(1)), int(k.group(2)))] = (text[a:m.start()], text[m.start():text.index(".end_amdhsa_kernel", m.start())])
    return out


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def test_every_instantiation_exists_once():
    assert sorted(_kernels()) == [(e, f) for e in EPILOGUES for f in WAVES_PER_SIMD]


@pytest.mark.parametrize("epi", sorted(EPILOGUES))
def test_scaled_fp4_mfma_and_nothing_else(epi):
    for (e, f), (code, meta) in _kernels().items():
        if e != epi:
            continue
        who = f"mx_rw_kernel<{EPILOGUES[e]}, {f}>"
        mfma = re.findall(r"^\s*(v_mfma\w+)", code, flags=re.M)
        assert mfma and set(mfma) == {"v_mfma_scale_f32_16x16x128_f8f6f4"}, f"{who}: {sorted(set(mfma))}"
        assert len(mfma) == 4 * f, f"{who}: {len(mfma)} MFMAs for 4 steps x {f} fragments"
        assert "cbsz:4" in code and "blgp:4" in code, f"{who}: the operands are not declared fp4"
        assert "v_cvt_scalef32" not in code and "_fp4" not in code.replace("f8f6f4", ""), f"{who}: dequantises an operand"
        assert not re.search(r"v_mfma_f32_\w*f16", code), f"{who}: an fp16 MFMA"
        if e == 1:
            assert "quad_perm:[1,0,3,2]" in code and "quad_perm:[2,3,0,1]" in code, f"{who}: the gate / up exchange is not DPP"
            assert not re.search(r"global_store_short\b", code), f"{who}: 2-byte stores"
        else:
            assert "quad_perm" not in code and "v_exp_f32" not in code, f"{who}: the SiLU epilogue leaked into the plain kernel"


def test_no_scratch_and_the_pinned_occupancy():
    for (e, f), (code, meta) in _kernels().items():
        who = f"mx_rw_kernel<{EPILOGUES[e]}, {f}>"
        assert _int(meta, "private_segment_fixed_size") == 0, f"{who}: scratch in use"
        assert not re.search(r"\bscratch_(load|store)", code), f"{who}: scratch access (a VGPR spill)"
        vgprs = _int(meta, "next_free_vgpr")
        alloc = (vgprs + 7) // 8 * 8                         # gfx950: 512 VGPRs (arch + acc) per SIMD lane, granules of 8
        waves = min(8, 512 // alloc)
        lds = _int(meta, "group_segment_fixed_size")
        print(f"{who}: {vgprs} VGPRs = {waves} waves / SIMD = {waves // 2} workgroups / CU; {lds} bytes of LDS")
        assert "v_accvgpr" not in code, f"{who}: accumulation registers in use"
        assert waves == WAVES_PER_SIMD[f], f"{who}: {vgprs} VGPRs = {waves} waves per SIMD, written for {WAVES_PER_SIMD[f]}"
        assert lds == 8 * f * 64 * 16, f"{who}: {lds} bytes of LDS"           # the partial sums: 8 waves x kF fragments x 64 lanes x 4 floats
        assert lds * (waves // 2) <= 160 * 1024, f"{who}: LDS, not registers, bounds the occupancy"


def test_weight_loads_are_whole_non_temporal_requests():
    """Per K step a lane requests its 16 bytes of MRW once (four steps in flight) and per round its MRSF dword once, both non-temporal; an A
    fragment is one 16-byte request per step and fragment."""
    for (e, f), (code, meta) in _kernels().items():
        who = f"mx_rw_kernel<{EPILOGUES[e]}, {f}>"
        nt4 = re.findall(r"global_load_dwordx4 .* nt\b", code)
        nt1 = re.findall(r"global_load_dword .* nt\b", code)
        assert len(nt4) == 4 and len(nt1) == 1, f"{who}: {len(nt4)} x4 and {len(nt1)} dword non-temporal loads"
        assert len(re.findall(r"global_load_dwordx4 ", code)) == 4 + 4 * f, f"{who}: A fragments are not one request per step and fragment"
