#!/usr/bin/env python3
"""In-kernel clock and phases of the tile GEMM (MI355X_MICROARCH.md "DVFS give-back" item 6): DIAGNOSTIC library only
(make -C arcquant_amd/csrc diag), >= 2 s of back-to-back launches on random data, then per workgroup the five stamps of
gemm_tile_body.inc (kernel entry, K loop starts, K loop ends, first output store issued, last output store issued; s_memtime and
s_memrealtime each): delta s_memtime / delta s_memrealtime x 100 MHz over the K loop = the shader clock, and the phases in
microseconds of the 100 MHz counter, median / p10 / p90 over the workgroups of the stamped launches.  The fp16 library GEMM cannot be
stamped; its clock is read from GRBM_GUI_ACTIVE in a separate rocprofv3 pass (profiles/).
usage: ARCQ_HIP_LIB=$PWD/arcquant_amd/lib/libarcq_hip_diag.so python tools/tile_clock.py [label]"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arcquant_amd import _lib, agemm  # noqa: E402
from bench import make_problem  # noqa: E402

STAMPS = 5                                   # kTileStamps of gemm_tile_common.hpp
PHASES = {"entry_to_k_loop": (0, 1), "k_loop": (1, 2), "k_loop_end_to_first_store": (2, 3), "first_to_last_store": (3, 4),
          "epilogue_k_loop_end_to_last_store": (2, 4), "entry_to_last_store": (0, 4)}
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("ARCQ_HIP_LIB", "diag"))
dev = torch.device("cuda:0")
setter = ctypes.CDLL(_lib.LIB_PATH).arcq_debug_set_tile_stamps
setter.argtypes = [ctypes.c_void_p]
for (M, N, KQ, silu) in ((4096, 4096, 4096, 0), (8192, 8192, 8192, 0), (4096, 37888, 3584, 1)):
    q = make_problem(M, N, KQ, 64, dev)
    if silu:
        def f():
            agemm.matmul_silu_mul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"])
    else:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)

        def f():
            agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], out=out)
    stamps = torch.zeros((4096 * 2 * STAMPS,), dtype=torch.int64, device=dev)
    setter(None)
    t0 = time.time()
    n = 0
    while time.time() - t0 < 2.5:                         # >= 2 s of continuous load before the stamped launches
        for _ in range(50 if silu else 200):
            f()
        n += 50 if silu else 200
        torch.cuda.synchronize()
    setter(stamps.data_ptr())
    for _ in range(50):
        f()
    torch.cuda.synchronize()
    setter(None)
    t = stamps.cpu().numpy().reshape(-1, STAMPS, 2)
    t = t[t[:, 0, 0] > 0]
    cyc, rt = (t[:, 2, 0] - t[:, 1, 0]).astype(np.float64), (t[:, 2, 1] - t[:, 1, 1]).astype(np.float64)
    ghz = cyc / rt * 0.1
    row = {"lib": label, "gemm": f"{M}x{N}x{KQ + 64}" + (" silu*up" if silu else ""), "workgroups": int(len(t)),
           "k_loop_us_median": round(float(np.median(rt)) / 100.0, 2),
           "in_kernel_clock_GHz_median": round(float(np.median(ghz)), 3), "p10": round(float(np.percentile(ghz, 10)), 3),
           "p90": round(float(np.percentile(ghz, 90)), 3), "launches_before_stamp": n, "phases_us": {}}
    for name, (a, b) in PHASES.items():
        d = (t[:, b, 1] - t[:, a, 1]).astype(np.float64) / 100.0
        row["phases_us"][name] = {"median": round(float(np.median(d)), 2), "p10": round(float(np.percentile(d, 10)), 2),
                                  "p90": round(float(np.percentile(d, 90)), 2)}
    print(json.dumps(row), flush=True)
    del q
    torch.cuda.empty_cache()
