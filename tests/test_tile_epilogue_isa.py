"""Audit of the tile GEMM's interior-tile epilogue in the generated code (arcquant_amd/csrc/gemm_tile.hip as tests/isa.py compiles it:
gfx950 assembly, product flags).

The headline instantiation, gemm_tile_kernel<256, 256, 2, 4, false, kEpiPlain, false, true> (bench.py's 4096 x 4096 x 4160), holds 8 x 4
MFMA tiles = 32 output quads per lane.  After its last v_mfma there must be a BRANCH-FREE run of instructions that
  * contains all of a wave's output stores (32 global_store_dwordx2, or 16 global_store_dwordx4),
  * contains no vector-memory load,
  * spends at most 8 instructions per output quad in total (needed: 2 multiplies, 2 conversions, 1 store, at most 1 swap and a share
    of one row-address add -- 6 or fewer; 8 leaves room for the compiler's moves and waits);
alpha_dev is not fetched with a vector-memory load after the last v_mfma (it is a scalar load ahead of the K loop: no single-dword
vector load is left behind the loop -- every other epilogue load is an 8-byte operand quad or a 2-byte element); the kernel uses no
scratch and at most 235 VGPRs (what the K loop was tuned with)."""
import collections
import os
import re

import pytest

from tests.isa import HIPCC, kernel

HEADLINE = "_ZN4arcq16gemm_tile_kernelILi256ELi256ELi2ELi4ELb0ELi0ELb0ELb1ELi0EEEvNS_10TileParamsE"
QUADS = 32                          # 8 x 4 MFMA tiles of 16 x 16 per wave, 4 columns per lane each
MAX_PER_QUAD = 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_headline_has_a_straight_line_interior_epilogue():
    code, meta = kernel("gemm_tile.hip", HEADLINE)

    # instruction stream with block boundaries (labels, branches) kept as None
    stream = []
    for line in code.split("\n"):
        t = line.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":"):
            stream.append(None)
        elif t.startswith("."):
            continue
        elif t.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            stream.append(None)
        else:
            stream.append(t)
    last_mfma = max(i for i, t in enumerate(stream) if t and t.startswith("v_mfma"))
    tail = stream[last_mfma + 1:]

    # no vector-memory load of alpha_dev behind the K loop
    lone = [t for t in tail if t and re.match(r"(global|flat|buffer)_load_dword\s", t)]
    assert not lone, f"single-dword vector load after the last v_mfma (alpha_dev?): {lone[:3]}"

    runs, cur = [], []
    for t in tail:
        if t is None:
            if cur:
                runs.append(cur)
            cur = []
        else:
            cur.append(t)
    if cur:
        runs.append(cur)
    found = []
    for r in runs:
        ops = collections.Counter(t.split()[0] for t in r)
        if any(re.match(r"(global|flat|buffer|scratch)_load", o) for o in ops):
            continue
        stores = {o: n for o, n in ops.items() if re.match(r"(global|flat|buffer)_store", o)}
        if stores == {"global_store_dwordx2": QUADS} or stores == {"global_store_dwordx4": QUADS // 2}:
            found.append((len(r), stores))
    assert found, "no branch-free, load-free run holding all of a wave's output stores after the last v_mfma"
    n = min(f[0] for f in found)
    print(f"interior epilogue: {n} instructions for {QUADS} output quads = {n / QUADS:.2f} per quad")
    assert n <= MAX_PER_QUAD * QUADS, f"{n} instructions for {QUADS} quads: more than {MAX_PER_QUAD} per quad"

    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", meta), "scratch in use"
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1))
    assert vgprs <= 235, vgprs
