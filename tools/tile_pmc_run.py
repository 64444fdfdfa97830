#!/usr/bin/env python3
"""Workload of a rocprofv3 --pmc pass over the tile GEMM's headline launch (bench.py's problem: M = N = 4096, KQ = 4096, KE = 64): N
back-to-back launches through agemm.matmul (reference layout) or, with `rw`, agemm.matmul_rw (repacked weight).  ARCQ_HIP_LIB selects
the library, ARCQ_AB_PAIR_LOADS / ARCQ_AB_QUAD_LOADS = 0|1 call arcq_debug_set_tile_pair_loads / arcq_debug_set_tile_quad_loads first.  usage: rocprofv3 --pmc <counters> --kernel-trace ... -- python3 tools/tile_pmc_run.py [ref|rw] [launches]
(tools/pmc_summarize.py <dir> gemm_tile <launches> then gives the per-launch means)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arcquant_amd import agemm  # noqa: E402
from bench import make_problem  # noqa: E402

route = sys.argv[1] if len(sys.argv) > 1 else "ref"
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 40
if os.environ.get("ARCQ_AB_PAIR_LOADS"):
    agemm._debug_set_tile_pair_loads(int(os.environ["ARCQ_AB_PAIR_LOADS"]))
if os.environ.get("ARCQ_AB_QUAD_LOADS"):
    agemm._debug_set_tile_quad_loads(int(os.environ["ARCQ_AB_QUAD_LOADS"]))
dev = torch.device("cuda:0")
M, N, KQ, KE = 4096, 4096, 4096, 64
p = make_problem(M, N, KQ, KE, dev)
out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
if route == "rw":
    rw, rsf = agemm.repack_w(p["qw"], p["sfw"])
    f = lambda: agemm.matmul_rw(p["qx"], rw, p["sfx"], rsf, p["alpha"], N, out=out)
else:
    f = lambda: agemm.matmul(p["qx"], p["qw"], p["sfx"], p["sfw"], p["alpha"], out=out)
for _ in range(launches):
    f()
torch.cuda.synchronize()
