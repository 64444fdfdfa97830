"""Audit of the tile GEMM's K loop in the generated code (arcquant_amd/csrc/gemm_tile.hip as tests/isa.py compiles it: gfx950 assembly,
product flags).

The headline instantiation, gemm_tile_kernel<256, 256, 2, 4, false, kEpiPlain, false, true>, runs its K loop unrolled by two steps (one per
LDS buffer).  All eight waves of a workgroup leave a barrier together, so whatever follows it runs on every SIMD at once with no partner
wave to cover it: it must be MFMAs whose operands are already in registers.  In the innermost loop of the kernel:
  * exactly one s_barrier per K step (two per unrolled iteration);
  * between each s_barrier and the next v_mfma (around the back-edge, should the barrier close the iteration): no ds_read* and no
    s_waitcnt that names lgkmcnt;
  * 64 v_mfma per step;
and the kernel uses no scratch."""
import os
import re

import pytest

from tests.isa import HIPCC, _innermost_loop, kernel

HEADLINE = "_ZN4arcq16gemm_tile_kernelILi256ELi256ELi2ELi4ELb0ELi0ELb0ELb1ELi0EEEvNS_10TileParamsE"
MFMA_PER_STEP = 64                  # 8 x 4 MFMA tiles of 16 x 16, two K halves of 32
STEPS_PER_ITERATION = 2


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_headline_k_loop_has_mfmas_behind_its_barrier():
    code, meta = kernel("gemm_tile.hip", HEADLINE)

    loop = _innermost_loop(code)
    ops = [t.split()[0] for t in loop]
    barriers = [i for i, o in enumerate(ops) if o == "s_barrier"]
    mfmas = sum(o.startswith("v_mfma") for o in ops)
    print(f"K loop: {len(loop)} instructions, {mfmas} v_mfma, {len(barriers)} s_barrier")
    assert mfmas == MFMA_PER_STEP * STEPS_PER_ITERATION, mfmas
    assert len(barriers) == STEPS_PER_ITERATION, barriers

    for b in barriers:
        between = []
        for k in range(1, len(loop) + 1):              # around the back-edge if need be
            t = loop[(b + k) % len(loop)]
            if t.startswith("v_mfma"):
                break
            between.append(t)
        bad = [t for t in between if t.startswith("ds_read") or (t.startswith("s_waitcnt") and "lgkmcnt" in t)]
        assert not bad, f"between an s_barrier and the next v_mfma: {bad}"

    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    assert not re.search(r"^\s*scratch_", code, re.M), "scratch instructions in the kernel"
