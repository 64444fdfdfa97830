"""Audit of the tile GEMM's operand staging in the generated code (arcquant_amd/csrc/gemm_tile.hip and gemm_tile_rw.hip, as tests/isa.py
compiles them: gfx950 assembly, product flags; the two compiles run side by side).

The K loop of the 256 x 256 8-wave tile is bound by vector-instruction issue, so it must hold no vector instruction the result does not
need.  A staging address is [tile origin, workgroup-uniform] + [lane offset, fixed for the launch] + [byte offset of the K step,
uniform]: only the last term moves, and it belongs on the scalar unit.  The two scale bytes of a staging unit become one packed fp16
pair in at most 3 vector instructions.  In the innermost loop (two K steps) of the headline instantiation
gemm_tile_kernel<256, 256, 2, 4, false, kEpiPlain, false, true> and of the same over the repacked weight (kBRepacked):
  * no 64-bit vector add (v_lshl_add_u64, v_add_co*, v_addc*);
  * 8 vector-memory loads (per step a 16-byte code load and a 2-byte scale load for each operand), each with a scalar offset
    (buffer loads) or a scalar base (global loads);
  * 128 v_mfma, 64 v_cvt_scalef32_pk_f16_fp4 and 64 v_pk_mul_f16: the dequantisation is what it was;
  * at most 12 other vector-ALU instructions (3 per staging unit and step);
and the kernels use at most 235 VGPRs and no scratch."""
import os
import re

import pytest

from tests.isa import HIPCC, _innermost_loop, assembly, kernel

KERNEL = "_ZN4arcq16gemm_tile_kernelILi256ELi256ELi2ELi4ELb0ELi0ELb0ELb1ELi%dEEEvNS_10TileParamsE"      # %d: kBLayout
UNITS = [("gemm_tile.hip", KERNEL % 0), ("gemm_tile_rw.hip", KERNEL % 1)]
MAX_OTHER_VALU = 12


@pytest.fixture(scope="module")
def kernels():
    """(code, metadata) of the two kernels."""
    assembly(*[src for src, _ in UNITS])
    return {src: kernel(src, name) for src, name in UNITS}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", [u[0] for u in UNITS])
def test_k_loop_forms_no_address_on_the_vector_unit(kernels, src):
    code, meta = kernels[src]
    loop = _innermost_loop(code)
    ops = [t.split()[0] for t in loop]

    wide_adds = [t for t, o in zip(loop, ops) if o.startswith(("v_lshl_add_u64", "v_add_co", "v_addc"))]
    assert not wide_adds, f"64-bit vector adds in the K loop: {wide_adds[:4]}"

    loads = [t for t, o in zip(loop, ops) if re.match(r"(buffer|global|flat|scratch)_load", o)]
    assert len(loads) == 8, loads
    for t in loads:
        args = [a.strip() for a in t.split(None, 1)[1].split(",")]
        if t.startswith("buffer_load"):             # vdata, vaddr, srsrc, soffset [modifiers]
            scalar = re.match(r"s\d+\b", args[3]) is not None
        else:                                       # vdata, vaddr, saddr | off
            scalar = t.startswith("global_load") and re.match(r"s\[\d+:\d+\]", args[2]) is not None
        assert scalar, f"a staging load without a scalar offset or base: {t}"

    count = lambda prefix: sum(o.startswith(prefix) for o in ops)
    mfma, cvt, mul = count("v_mfma"), count("v_cvt_scalef32_pk_f16_fp4"), count("v_pk_mul_f16")
    other = [t for t, o in zip(loop, ops) if o.startswith("v_") and not o.startswith(("v_mfma", "v_cvt_scalef32_pk_f16_fp4", "v_pk_mul_f16"))]
    print(f"{src}: K loop of {len(loop)} instructions: {mfma} v_mfma, {cvt} conversions, {mul} packed multiplies, {len(other)} other vector-ALU: "
          f"{sorted(set(t.split()[0] for t in other))}")
    assert (mfma, cvt, mul) == (128, 64, 64), (mfma, cvt, mul)
    assert len(other) <= MAX_OTHER_VALU, other

    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    print(f"{src}: {vgprs} VGPRs")
    assert vgprs <= 235, vgprs
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    assert not re.search(r"^\s*scratch_", code, re.M), "scratch instructions in the kernel"
