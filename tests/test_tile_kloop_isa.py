"""Audit of the tile GEMM's K loop in the generated code (arcquant_amd/csrc/gemm_tile.hip, one compile to gfx950 assembly, product flags:
the compile line of tests/test_tile_epilogue_isa.py).

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
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arcquant_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HEADLINE = "_ZN4arcq16gemm_tile_kernelILi256ELi256ELi2ELi4ELb0ELi0ELb0ELb1ELi0EEEvNS_10TileParamsE"
MFMA_PER_STEP = 64                  # 8 x 4 MFMA tiles of 16 x 16, two K halves of 32
STEPS_PER_ITERATION = 2


def _innermost_loop(code):
    """Instructions of the loop (label .. backward conditional branch to it) that holds the most v_mfma and no other loop."""
    lines = []
    for line in code.split("\n"):
        t = line.split(";")[0].strip()
        if t and (t.endswith(":") or not t.startswith(".")):
            lines.append(t)
    labels = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
    loops = []
    for i, t in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", t)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    assert loops, "no loop in the kernel"
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    a, b = max(inner, key=lambda ab: sum(t.startswith("v_mfma") for t in lines[ab[0]:ab[1]]))
    return [t for t in lines[a:b] if not t.endswith(":")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_headline_k_loop_has_mfmas_behind_its_barrier(tmp_path):
    asm = tmp_path / "gemm_tile.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-I", CSRC, os.path.join(CSRC, "gemm_tile.hip"), "-o", str(asm)], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    a = text.index("\n" + HEADLINE + ":")
    body = text[a:text.index(".end_amdhsa_kernel", a)]
    meta = body[body.rindex(".amdhsa_kernel"):]
    code = body[:body.rindex(".amdhsa_kernel")]

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
