"""Audit of the tile GEMM's quad operand loads in the generated code (arcquant_amd/csrc/gemm_tile_ql.hip as tests/isa.py compiles it: gfx950
assembly, product flags).

gemm_tile_ql_kernel<256, 256, 2, 4, kEpiPlain, kBRef, 0> (no bias, no residual) is the paired-load kernel whose loop iteration is FOUR K
steps: step 0 requests the code bytes of A's four following atoms of a row back to back, step 2 those of B's, and both operands got
quads (not A alone).  In the generated code:
  * the innermost loop holds 256 v_mfma, 128 v_cvt_scalef32_pk_f16_fp4, 128 v_pk_mul_f16 and 4 s_barrier (four K steps, the audited work);
  * it holds 16 buffer_load, 8 of them 16-byte code loads (dwordx4) and 8 scale loads;
  * the code loads are two runs of FOUR consecutive instructions, a run through one descriptor and one lane offset (one row's atoms
    kt + 2 .. kt + 5), the two runs through different descriptors (A and B) and in different steps (a barrier between them);
  * at most 256 VGPRs (two waves per SIMD), no scratch -- in every instantiation of the unit."""
import os
import re

import pytest

from tests.isa import HIPCC, _innermost_loop, assembly, kernel

SIBLING = "_ZN4arcq19gemm_tile_ql_kernelILi256ELi256ELi2ELi4ELi0ELi0ELi0EEEvNS_10TileParamsE"


@pytest.fixture(scope="module")
def sibling():
    """(instructions and labels of the kernel, its metadata)"""
    return kernel("gemm_tile_ql.hip", SIBLING)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_loop_work_and_registers(sibling):
    code, meta = sibling
    ops = [t.split()[0] for t in _innermost_loop(code)]
    count = lambda prefix: sum(o.startswith(prefix) for o in ops)
    got = (count("v_mfma"), count("v_cvt_scalef32_pk_f16_fp4"), count("v_pk_mul_f16"), count("s_barrier"))
    print(f"K loop of {len(ops)} instructions: v_mfma, conversions, packed multiplies, s_barrier = {got}; {count('v_mov_b')} v_mov")
    assert got == (256, 128, 128, 4), got

    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    print(f"{vgprs} VGPRs")
    assert vgprs <= 256, vgprs
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    assert not re.search(r"^\s*scratch_", code, re.M), "scratch instructions in the kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_instantiation_of_the_unit_spills():
    text = assembly("gemm_tile_ql.hip")
    sizes = re.findall(r"\.amdhsa_private_segment_fixed_size (\d+)", text)
    vgprs = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr (\d+)", text)]
    print(f"private segment sizes {sizes}, VGPRs {vgprs}")
    assert len(sizes) == 4 and set(sizes) == {"0"}, sizes
    assert max(vgprs) <= 256, vgprs
    assert not re.search(r"^\s*scratch_", text, re.M), "scratch instructions in the unit"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_code_loads_of_the_loop_are_two_runs_of_four(sibling):
    code, _ = sibling
    loop = _innermost_loop(code)
    ops = [t.split()[0] for t in loop]
    loads = [i for i, o in enumerate(ops) if o.startswith("buffer_load")]
    barriers = [i for i, o in enumerate(ops) if o == "s_barrier"]
    print(f"buffer_load at {loads}, s_barrier at {barriers} of {len(ops)}")
    assert len(loads) == 16, loads

    def operands(i):                         # buffer_load_dwordx4 vDST, vOFF, s[DESC], sOFF offen -> (lane offset, descriptor)
        m = re.match(r"buffer_load_\w+\s+\S+,\s*(v\d+),\s*(s\[\d+:\d+\]),", loop[i])
        assert m, loop[i]
        return m.group(1), m.group(2)

    wide = [i for i in loads if ops[i] == "buffer_load_dwordx4"]
    assert len(wide) == 8, [loop[i] for i in loads]
    runs = [wide[:4], wide[4:]]
    for run in runs:
        assert run == list(range(run[0], run[0] + 4)), wide                       # four consecutive instructions
        assert len({operands(i) for i in run}) == 1, [loop[i] for i in run]       # one descriptor, one lane offset
    assert operands(runs[0][0])[1] != operands(runs[1][0])[1], [loop[i] for i in wide]   # one run per operand
    assert sum(runs[0][0] < b < runs[1][0] for b in barriers) == 2, (wide, barriers)     # two steps apart
