"""Audit of the tile GEMM's overlapped tail in the generated code (arcquant_amd/csrc/gemm_tile_ot.hip as tests/isa.py compiles it: gfx950 assembly,
product flags).

gemm_tile_ot_kernel<256, 256, 2, 4, kEpiPlain, kBRef, 0> (no bias, no residual) is the headline kernel with another tail: the K loop is the audited one, the last
K step of the range is multiplied without staging anything, and output stores leave under its MFMAs.  In the generated code:
  * the innermost loop holds 128 v_mfma, 64 v_cvt_scalef32_pk_f16_fp4, 64 v_pk_mul_f16 and 2 s_barrier (two unchanged K steps);
  * behind the loop there is a branch-free block with the 64 v_mfma of a K step and no buffer_load, no ds_write and no s_barrier,
    and at least one global_store_dwordx4 ahead of its last v_mfma;
  * the 128 v_mov_b32 that zero the accumulators precede the first s_waitcnt that names vmcnt (they are issued while the prologue's
    loads are in flight);
  * at most 235 VGPRs, no scratch."""
import os
import re

import pytest

from tests.isa import HIPCC, _innermost_loop, kernel

SIBLING = "_ZN4arcq19gemm_tile_ot_kernelILi256ELi256ELi2ELi4ELi0ELi0ELi0EEEvNS_10TileParamsE"
ACC_REGISTERS = 128                 # 8 x 4 MFMA tiles of 16 x 16: four fp32 per lane each


@pytest.fixture(scope="module")
def sibling():
    """(instructions and labels of the kernel, its metadata)"""
    return kernel("gemm_tile_ot.hip", SIBLING)


def _blocks(code):
    """Branch-free runs of instructions (cut at labels and branches), in program order."""
    runs, cur = [], []
    for line in code.split("\n"):
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        if t.endswith(":") or t.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            if cur:
                runs.append(cur)
            cur = []
        else:
            cur.append(t)
    if cur:
        runs.append(cur)
    return runs


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_k_loop_is_the_audited_one(sibling):
    code, meta = sibling
    ops = [t.split()[0] for t in _innermost_loop(code)]
    count = lambda prefix: sum(o.startswith(prefix) for o in ops)
    got = (count("v_mfma"), count("v_cvt_scalef32_pk_f16_fp4"), count("v_pk_mul_f16"), count("s_barrier"))
    print(f"K loop of {len(ops)} instructions: v_mfma, conversions, packed multiplies, s_barrier = {got}")
    assert got == (128, 64, 64, 2), got

    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    print(f"{vgprs} VGPRs")
    assert vgprs <= 235, vgprs
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    assert not re.search(r"^\s*scratch_", code, re.M), "scratch instructions in the kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_final_step_stages_nothing_and_stores_under_its_mfmas(sibling):
    code, _ = sibling
    loop = _innermost_loop(code)
    runs = _blocks(code)
    # the blocks behind the loop: those that start after the loop's last instruction
    flat = [t for r in runs for t in r]
    last_loop = next(i for i in range(len(flat) - len(loop) + 1) if flat[i:i + len(loop)] == loop) + len(loop)
    found = []
    pos = 0
    for r in runs:
        pos += len(r)
        if pos - len(r) < last_loop:
            continue
        ops = [t.split()[0] for t in r]
        mfma = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
        if len(mfma) != 64 or any(o.startswith(("buffer_load", "ds_write")) or o == "s_barrier" for o in ops):
            continue
        early = sum(o == "global_store_dwordx4" for o in ops[:mfma[-1]])
        found.append((len(r), early, sum(o == "global_store_dwordx4" for o in ops)))
    print(f"final-step blocks behind the loop (instructions, global_store_dwordx4 ahead of the last v_mfma, all): {found}")
    assert found, "no branch-free block of 64 v_mfma without buffer_load, ds_write and s_barrier behind the K loop"
    assert all(early >= 1 for _, early, _ in found), found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_accumulators_are_zeroed_ahead_of_the_first_wait_for_a_load(sibling):
    code, _ = sibling
    flat = [t for r in _blocks(code) for t in r]
    first_wait = next(i for i, t in enumerate(flat) if t.startswith("s_waitcnt") and "vmcnt" in t)
    # (the zero is an inline constant or a scalar register pair; hipcc writes two accumulator registers per v_mov_b64 where it can)
    head = [t.split()[0] for t in flat[:first_wait]]
    loads = [i for i, o in enumerate(head) if o.startswith("buffer_load")]
    assert len(loads) == 8, loads                    # both K steps of the prologue are requested by then
    shadow = head[loads[-1] + 1:]                    # between the last request and the first wait: while the loads are in flight
    movs = sum(o.startswith("v_mov_b32") for o in shadow)
    wide = sum(o.startswith("v_mov_b64") for o in shadow)
    print(f"{movs} v_mov_b32 and {wide} v_mov_b64 between the prologue's last buffer_load and the first s_waitcnt vmcnt")
    assert movs + 2 * wide >= ACC_REGISTERS, (movs, wide)
