"""Audit of the MXFP4 fused decode linear in the generated code (one compile of gemm_mx_linear_rw.hip to gfx950 assembly, product flags):
the three instantiations of mx_linear_kernel -- the RMSNorm source with the plain and the SiLU*up epilogue, the plain source with the
plain epilogue -- each exist once, multiply only on the scaled 16x16x128 fp4 MFMA (the conversions to fp4 are the prologue's
quantiser; nothing is converted back), run without scratch or spills, load the weight as 16-byte-per-lane non-temporal requests one
round ahead, and keep the occupancy they were written for.

Registers and LDS: 90 VGPRs in every instantiation, inside the 128-register class that the launch bound asks for:
4 waves per SIMD = two 8-wave workgroups per CU.  The LDS is dynamic (the image grows with K): 71904 bytes at the model's shape
(KQ = 3584, KE = 64, RMSNorm source, four rows staged per pass), at most 81920, so that LDS too leaves two workgroups per CU.  Counts may
move inside a class; the class is pinned."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# (kSrc, kEpi): kSrc 0 = RMSNorm, 1 = plain; kEpi 0 = plain, 1 = SiLU*up
KERNELS = {(0, 0): "rmsnorm, plain", (0, 1): "rmsnorm, silu_mul", (1, 0): "plain, plain"}
WAVES_PER_SIMD = 4


def _kernels():
    text = assembly("gemm_mx_linear_rw.hip")
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M):
        name = m.group(1)
        k = re.search(r"mx_linear_kernelILi(\d)ELi(\d)EE", name)
        assert k, f"unexpected kernel {name} in gemm_mx_linear_rw.hip"
        key = (int(k.group(1)), int(k.group(2)))
        assert key not in out, f"{name} twice"
        a = text.index("\n" + name + ":")
        out[key] = (text[a:m.start()], text[m.start():text.index(".end_amdhsa_kernel", m.start())])
    return out


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def test_every_instantiation_exists_once():
    assert sorted(_kernels()) == sorted(KERNELS)


def test_scaled_fp4_mfma_and_nothing_else():
    for key, (code, meta) in _kernels().items():
        who = f"mx_linear_kernel<{KERNELS[key]}>"
        mfma = re.findall(r"^\s*(v_mfma\w+)", code, flags=re.M)
        assert mfma and set(mfma) == {"v_mfma_scale_f32_16x16x128_f8f6f4"}, f"{who}: {sorted(set(mfma))}"
        assert len(mfma) == 4, f"{who}: {len(mfma)} MFMAs for the 4 steps of a round"
        assert "cbsz:4" in code and "blgp:4" in code, f"{who}: the operands are not declared fp4"
        assert "v_cvt_scalef32_pk_fp4_f32" in code, f"{who}: the prologue does not quantise with the fp4 conversion"
        assert "v_cvt_scalef32_pk_f32_fp4" not in code, f"{who}: dequantises an operand"
        assert not re.search(r"v_mfma_f32_\w*f16", code), f"{who}: an fp16 MFMA"
        if key[1] == 1:
            assert "quad_perm:[1,0,3,2]" in code and "quad_perm:[2,3,0,1]" in code, f"{who}: the gate / up exchange is not DPP"
            assert not re.search(r"global_store_short\b", code), f"{who}: 2-byte stores"
        else:
            assert "quad_perm" not in code and "v_exp_f32" not in code, f"{who}: the SiLU epilogue leaked into the plain kernel"
        assert ("v_rsq_f64" in code or "v_sqrt_f64" in code) == (key[0] == 0), f"{who}: rstd belongs to the RMSNorm source alone"


def test_no_scratch_and_the_pinned_occupancy():
    for key, (code, meta) in _kernels().items():
        who = f"mx_linear_kernel<{KERNELS[key]}>"
        assert _int(meta, "private_segment_fixed_size") == 0, f"{who}: scratch in use"
        assert not re.search(r"\bscratch_(load|store)", code), f"{who}: scratch access (a VGPR spill)"
        vgprs = _int(meta, "next_free_vgpr")
        alloc = (vgprs + 7) // 8 * 8                         # gfx950: 512 VGPRs (arch + acc) per SIMD lane, granules of 8
        waves = min(8, 512 // alloc)
        print(f"{who}: {vgprs} VGPRs = {waves} waves / SIMD")
        assert "v_accvgpr" not in code, f"{who}: accumulation registers in use"
        assert vgprs <= 128 and waves >= WAVES_PER_SIMD, f"{who}: {vgprs} VGPRs = {waves} waves per SIMD, written for {WAVES_PER_SIMD}"
        assert _int(meta, "group_segment_fixed_size") == 0, f"{who}: static LDS beside the dynamic image (the budget formula does not count it)"


def test_lds_budget_leaves_two_workgroups_per_cu():
    """The dynamic LDS of a launch is the library's own formula (include/arcq.h); pinned at the model's shapes."""
    from arcquant_amd import mx
    assert mx.linear_fused_lds_bytes(mx.SRC_RMSNORM, 3584, 64) == 29 * 1088 + 32 + 5 * 8064 == 71904     # q|k|v, gate|up: four rows a pass
    assert mx.linear_fused_lds_bytes(mx.SRC_PLAIN, 3584, 64) == 29 * 1088 + 32 + 4 * 8064 == 63840       # o
    assert mx.linear_fused_lds_bytes(mx.SRC_RMSNORM, 4096, 128) == 33 * 1088 + 32 + 3 * 9216 == 63584    # two rows a pass
    assert mx.linear_fused_lds_bytes(mx.SRC_PLAIN, 64, 0) == 1088 + 32 + 16384                           # the partial sums bound it
    for kind in (mx.SRC_RMSNORM, mx.SRC_PLAIN):
        for KQ in range(2048, 8192 + 64, 64):
            if mx.linear_fused_supported(kind, 4, 16, KQ, 64):
                assert 2 * mx.linear_fused_lds_bytes(kind, KQ, 64) <= 160 * 1024, (kind, KQ)


def test_weight_loads_are_whole_non_temporal_requests():
    """Per K step a lane requests its 16 bytes of MRW once and per round its MRSF dword once, both non-temporal; the loads appear twice in
    the text: the first round ahead of the prologue, and one round ahead inside the K loop."""
    for key, (code, meta) in _kernels().items():
        who = f"mx_linear_kernel<{KERNELS[key]}>"
        nt4 = re.findall(r"global_load_dwordx4 .* nt\b", code)
        nt1 = re.findall(r"global_load_dword .* nt\b", code)
        assert len(nt4) == 8 and len(nt1) == 2, f"{who}: {len(nt4)} x4 and {len(nt1)} dword non-temporal loads"
        first_mfma = code.index("v_mfma_scale")
        assert len(re.findall(r"ds_read_b128|ds_read2_b64", code[code.rindex("s_barrier", 0, first_mfma):])) >= 4, f"{who}: the A fragments do not come from LDS"
