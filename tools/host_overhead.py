#!/usr/bin/env python3
"""Host time per call of the agemm wrappers (Python + ctypes + allocations), GPU left to run asynchronously: what paces an EAGER
decode step (benchmarks/benchmark_e2e_arc.py runs eagerly).  usage: python tools/host_overhead.py [--json FILE]
--json FILE also writes {call: host microseconds per call}, so that two builds can be compared call by call."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arcquant_amd import agemm  # noqa: E402
from bench import make_problem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", metavar="FILE")
args = ap.parse_args()
dev = torch.device("cuda:0")
M, N, KQ, KE = 4, 3584, 3584, 64
q = make_problem(M, N, KQ, KE, dev)
RW, RSF = agemm.repack_w(q["qw"], q["sfw"])
wn = torch.ones(KQ, dtype=torch.bfloat16, device=dev)
res = torch.zeros((M, N), dtype=torch.bfloat16, device=dev)
calls = {
    "rmsnorm_matmul_repacked": lambda: agemm.rmsnorm_matmul_repacked(q["x"], wn, 1e-6, q["idx"], KE, RW, RSF, 1.0, N),
    "dynamic_matmul_repacked(residual)": lambda: agemm.dynamic_matmul_repacked(q["x"], q["idx"], KE, RW, RSF, 1.0, N, residual=res),
    "matmul_repacked": lambda: agemm.matmul_repacked(q["qx"], RW, q["sfx"], RSF, q["alpha"], N),
    "reorder_quantize_x_dynamic": lambda: agemm.reorder_quantize_x_dynamic(q["x"], q["idx"], KE),
    "matmul (reference layout)": lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"]),
    "torch.empty((4, 3584))": lambda: torch.empty((M, N), dtype=torch.bfloat16, device=dev),
}
try:                                                           # the pybind11 extension form of the same boundary (csrc/agemm_ext.cpp)
    from arcquant_amd import _build_ext
    ext = _build_ext.import_agemm_extension()
    xs = (q["x"] / q["sx"]).contiguous()
    qx64, sfx64 = agemm.reorder_quantize_x(xs.repeat(16, 1), q["idx"], KE)
    calls["EXT matmul (reference layout)"] = lambda: ext.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"])
    calls["EXT reorder_quantize_x"] = lambda: ext.reorder_quantize_x(xs, q["idx"], KE)
    calls["ctypes reorder_quantize_x"] = lambda: agemm.reorder_quantize_x(xs, q["idx"], KE)
    calls["EXT rmsnorm_quantize_x"] = lambda: ext.rmsnorm_quantize_x(q["x"], wn, 1e-6, q["idx"], KE)
    calls["ctypes rmsnorm_quantize_x"] = lambda: agemm.rmsnorm_quantize_x(q["x"], wn, 1e-6, q["idx"], KE)
    # the decode entry points arcquant_amd/e2e.py calls per layer, through the extension and (same arguments) through ctypes
    bias = torch.zeros(N, dtype=torch.bfloat16, device=dev)
    _, slots = agemm.rmsnorm_matmul_repacked_silu(q["x"], wn, 1e-6, q["idx"], KE, RW, RSF, 1.0, N)
    act = torch.zeros((M, KQ), dtype=torch.bfloat16, device=dev)
    for tag, mod in (("EXT", ext), ("ctypes", agemm)):
        calls[f"{tag} rmsnorm_matmul_repacked(bias)"] = lambda mod=mod: mod.rmsnorm_matmul_repacked(q["x"], wn, 1e-6, q["idx"], KE, RW, RSF, 1.0, N, bias=bias)
        calls[f"{tag} dynamic_matmul_repacked(bias, residual)"] = lambda mod=mod: mod.dynamic_matmul_repacked(q["x"], q["idx"], KE, RW, RSF, 1.0, N, bias=bias,
                                                                                                              residual=res)
        calls[f"{tag} rmsnorm_matmul_repacked_silu"] = lambda mod=mod: mod.rmsnorm_matmul_repacked_silu(q["x"], wn, 1e-6, q["idx"], KE, RW, RSF, 1.0, N)
        calls[f"{tag} reorder_quantize_x_dynamic(slots)"] = lambda mod=mod: mod.reorder_quantize_x_dynamic(act, None, KE, absmax_slots=slots)
        calls[f"{tag} matmul_repacked(device scale)"] = lambda mod=mod: mod.matmul_repacked(q["qx"], RW, q["sfx"], RSF, q["alpha"], N)
        calls[f"{tag} matmul_rw(M=64)"] = lambda mod=mod: mod.matmul_rw(qx64, RW, sfx64, RSF, q["alpha"], N)
except ImportError as e:
    print("extension not built:", e)
host_us = {}
for name, f in calls.items():
    for _ in range(200):
        f()
    torch.cuda.synchronize()
    n = 2000
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    host_us[name] = round(1e6 * (t1 - t0) / n, 3)
    print(f"{name:48s} host {host_us[name]:6.2f} us per call   (with the GPU drained: {1e6 * (t2 - t0) / n:6.2f} us)", flush=True)
if args.json:
    with open(args.json, "w") as fh:
        json.dump(host_us, fh, indent=1)
