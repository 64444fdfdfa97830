#!/usr/bin/env python3
"""MXFP4 GEMM and quantisers on the MI355X against NVFP4 (agemm.matmul) and the fp16 library GEMM (torch.matmul), in one process
and the same warm state; prints ONE JSON line (the evidence behind profiles/mxfp4_gemm.json).

    python tools/mx_bench.py [--quick] [--out FILE]

Method: bench.make_problem builds the NVFP4 operands (outlier activations, identity reorder index) and the same x / w are quantised
to MXFP4; prefill shapes are timed with bench.time_events_steady (sustained back-to-back launches, both sides alike); decode shapes
are HIP-graph replays over weight copies totalling > 320 MB (HBM-cold, as bench.py's decode figures); the quantisers' inputs rotate
through > 320 MB as well."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from bench import PEAK_F16_TFLOPS, PEAK_FP4_TFLOPS, PEAK_HBM_GBS, make_problem, time_events_steady  # noqa: E402
from arcquant_amd import agemm  # noqa: E402

KE = 64


def graph_time(launches, reps=10):
    """us per launch of zero-arg closures replayed from one HIP graph (warm ~40 ms of replays, then time >= ~10 ms)."""
    for f in launches:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for f in launches:
            f()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            for f in launches:
                f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    per_ms = max(e0.elapsed_time(e1) / 3, 1e-3)
    for _ in range(min(20000, int(40.0 / per_ms))):
        g.replay()
    reps = max(reps, min(20000, int(10.0 / per_ms)))
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(launches))


def mx_problem(q):
    qx, sx = agemm.mx_reorder_quantize_x(q["x"], q["idx"], KE)
    qw, sw = agemm.mx_reorder_quantize_w(q["w"], q["idx"], KE)
    return qx, sx, qw, sw


def mx_bytes(M, N, Kp):
    return (M + N) * Kp * (1 / 2 + 1 / 32) + 2 * M * N


def prefill(M, N, KQ, dev, iters):
    q = make_problem(M, N, KQ, KE, dev)
    qx, sx, qw, sw = mx_problem(q)
    K, Kp = KQ + KE, qx.shape[1] * 2
    o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    t_mx = time_events_steady(lambda: agemm.mx_matmul(qx, qw, sx, sw, 1.0, out=o), iters)
    t_nv = time_events_steady(lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], out=o), iters)
    a16 = torch.randn(M, K, dtype=torch.float16, device=dev)
    b16 = torch.randn(N, K, dtype=torch.float16, device=dev)
    o16 = torch.empty((M, N), dtype=torch.float16, device=dev)
    t16 = time_events_steady(lambda: torch.matmul(a16, b16.t(), out=o16), iters)
    f_mx = bench.gemm_flops(M, N, Kp)
    rec = {"M": M, "N": N, "KQ": KQ, "KE": KE, "Kp": Kp, "mxfp4_us": round(t_mx, 2), "nvfp4_us": round(t_nv, 2), "fp16_torch_matmul_us": round(t16, 2),
           "speedup_vs_nvfp4": round(t_nv / t_mx, 3), "speedup_vs_fp16": round(t16 / t_mx, 3),
           "mxfp4_TFLOPs": round(f_mx / t_mx / 1e6, 1), "frac_of_fp4_peak": round(f_mx / t_mx / 1e6 / PEAK_FP4_TFLOPS, 4),
           "nvfp4_frac_of_fp16_peak": round(bench.gemm_flops(M, N, K) / t_nv / 1e6 / PEAK_F16_TFLOPS, 4)}
    del q
    torch.cuda.empty_cache()
    return rec


def decode(M, N, KQ, dev):
    q = make_problem(M, N, KQ, KE, dev)
    qx, sx, qw, sw = mx_problem(q)
    K, Kp = KQ + KE, qx.shape[1] * 2
    o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    ws = [(qw.clone(), sw.clone()) for _ in range(rot)]
    t_mx = graph_time([(lambda i=i: agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0, out=o)) for i in range(rot)])
    del ws
    rot = max(2, int(320e6 // (N * K * 9 / 16)) + 1)
    nws = [(q["qw"].clone(), q["sfw"].clone()) for _ in range(rot)]
    t_nv = graph_time([(lambda i=i: agemm.matmul(q["qx"], nws[i][0], q["sfx"], nws[i][1], q["alpha"], out=o)) for i in range(rot)])
    del nws, q
    torch.cuda.empty_cache()
    gb = mx_bytes(M, N, Kp)
    return {"M": M, "N": N, "KQ": KQ, "mxfp4_us": round(t_mx, 2), "nvfp4_us": round(t_nv, 2), "speedup_vs_nvfp4": round(t_nv / t_mx, 3),
            "mxfp4_GBps": round(gb / t_mx / 1e3, 1), "mxfp4_frac_hbm_peak": round(gb / t_mx / 1e3 / PEAK_HBM_GBS, 4)}


def quantisers(S, dev):
    idx = torch.arange(S, dtype=torch.int16, device=dev)
    rot = max(2, int(320e6 // (S * S * 2)) + 1)
    xs = [bench.outlier_activations(S, S, dev, seed=i) for i in range(rot)]
    Kp = agemm.mx_k_padded(S + KE)
    gb = S * S * 2 + S * Kp * (1 / 2 + 1 / 32)
    rec = {}
    for name, fn in (("x", agemm.mx_reorder_quantize_x), ("w", agemm.mx_reorder_quantize_w)):
        t = graph_time([(lambda i=i: fn(xs[i], idx, KE)) for i in range(rot)])
        rec[f"mx_quantize_{name}_us"] = round(t, 2)
        rec[f"mx_quantize_{name}_GBps"] = round(gb / t / 1e3, 1)
    t = graph_time([(lambda i=i: agemm.reorder_quantize_x(xs[i], idx, KE)) for i in range(rot)])
    rec["nvfp4_quantize_x_us"] = round(t, 2)
    del xs
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="headline shape only")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "peak_fp4_TFLOPs": PEAK_FP4_TFLOPS, "peak_f16_TFLOPs": PEAK_F16_TFLOPS,
           "headline": prefill(4096, 4096, 4096, dev, a.iters)}
    if not a.quick:
        res["gemm_8192"] = prefill(8192, 8192, 8192, dev, a.iters)
        res["qwen_prefill_M4096"] = [prefill(4096, n, kq, dev, a.iters) for n, kq in ((10752, 3584), (3584, 3584), (37888, 3584), (3584, 18944))]
        res["decode_hbm_cold"] = [decode(m, n, kq, dev) for m, n, kq in ((1, 4096, 4096), (4, 4096, 4096), (16, 4096, 4096), (4, 3584, 3584),
                                                                       (4, 10752, 3584), (4, 37888, 3584), (4, 3584, 18944))]
        res["quantisers"] = {f"S{S}": quantisers(S, dev) for S in (4096, 8192)}
    res["note"] = ("prefill: sustained back-to-back launches (bench.time_events_steady), MXFP4 / NVFP4 / fp16 library GEMM in the same process; "
                   "frac_of_fp4_peak = 2*M*N*Kp / time over the 10 PFLOP/s dense fp4 MFMA roof; decode: HIP-graph replay over weight copies "
                   "> 320 MB (HBM-cold), GBps = algorithmic bytes (codes + scales of both operands + bf16 D) / time; quantisers: inputs rotated "
                   "through > 320 MB, GBps = bf16 input + codes + scales")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
