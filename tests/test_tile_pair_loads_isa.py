"""Audit of the tile GEMM's paired operand loads in the generated code (arcquant_amd/csrc/gemm_tile_pl.hip as tests/isa.py compiles it: gfx950 assembly,
product flags).

gemm_tile_pl_kernel<256, 256, 2, 4, kEpiPlain, kBRef, 0> (no bias, no residual) is the overlapped-tail kernel whose even K step requests
the code bytes of both following atoms of a row back to back and whose odd K step requests nothing.  In the generated code:
  * the innermost loop holds 128 v_mfma, 64 v_cvt_scalef32_pk_f16_fp4, 64 v_pk_mul_f16 and 2 s_barrier (two K steps, the audited work);
  * it holds 8 buffer_load, every one ahead of its first s_barrier (the even step's);
  * its four 16-byte code loads are two pairs of CONSECUTIVE instructions, a pair through one descriptor and one lane offset (one row's
    atoms kt + 2 and kt + 3), the two pairs through different descriptors (A and B) -- so each A code load that opens a pair is followed
    at once by a load through its own descriptor; the four scale loads come behind them (the pairs and the scale loads are spread over
    the even step's blocks: one burst of eight loads at its top measured slower);
  * at most 246 VGPRs, no scratch."""
import os
import re

import pytest

from tests.isa import HIPCC, _innermost_loop, kernel

SIBLING = "_ZN4arcq19gemm_tile_pl_kernelILi256ELi256ELi2ELi4ELi0ELi0ELi0EEEvNS_10TileParamsE"


@pytest.fixture(scope="module")
def sibling():
    """(instructions and labels of the kernel, its metadata)"""
    return kernel("gemm_tile_pl.hip", SIBLING)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_loop_work_and_registers(sibling):
    code, meta = sibling
    ops = [t.split()[0] for t in _innermost_loop(code)]
    count = lambda prefix: sum(o.startswith(prefix) for o in ops)
    got = (count("v_mfma"), count("v_cvt_scalef32_pk_f16_fp4"), count("v_pk_mul_f16"), count("s_barrier"))
    print(f"K loop of {len(ops)} instructions: v_mfma, conversions, packed multiplies, s_barrier = {got}; {count('v_mov_b')} v_mov")
    assert got == (128, 64, 64, 2), got

    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    print(f"{vgprs} VGPRs")
    assert vgprs <= 246, vgprs
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    assert not re.search(r"^\s*scratch_", code, re.M), "scratch instructions in the kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_loads_of_the_loop_are_paired_and_ahead_of_the_even_steps_barrier(sibling):
    code, _ = sibling
    loop = _innermost_loop(code)
    ops = [t.split()[0] for t in loop]
    loads = [i for i, o in enumerate(ops) if o.startswith("buffer_load")]
    first_barrier = ops.index("s_barrier")
    print(f"buffer_load at {loads}, first s_barrier at {first_barrier} of {len(ops)}")
    assert len(loads) == 8, loads
    assert all(i < first_barrier for i in loads), (loads, first_barrier)

    def operands(i):                         # buffer_load_dwordx4 vDST, vOFF, s[DESC], sOFF offen -> (lane offset, descriptor)
        m = re.match(r"buffer_load_\w+\s+\S+,\s*(v\d+),\s*(s\[\d+:\d+\]),", loop[i])
        assert m, loop[i]
        return m.group(1), m.group(2)

    wide = [i for i in loads if ops[i] == "buffer_load_dwordx4"]
    assert len(wide) == 4 and wide == loads[:4], [loop[i] for i in loads]
    assert wide[1] == wide[0] + 1 and wide[3] == wide[2] + 1, wide               # each pair: consecutive instructions
    assert operands(wide[0]) == operands(wide[1]) and operands(wide[2]) == operands(wide[3]), [loop[i] for i in wide]
    assert operands(wide[0])[1] != operands(wide[2])[1], [loop[i] for i in wide]   # one pair per operand
