#!/usr/bin/env python3
"""agemm.mx6_matmul with an e3m2 weight (MXFP6) and with an e2m1 weight (W4A6) against agemm.mx_matmul (MXFP4) on the same shapes, in the
same run, on the MI355X; writes profiles/mxfp6_gemm.json.

    python tools/mx6_bench.py [--rounds R] [--out FILE]
    python tools/mx6_bench.py --table repacked [--rounds R] [--out FILE]

--table repacked: the decode GEMM over the repacked weight (agemm.mx6_matmul_repacked) against agemm.mx6_matmul for both weight formats,
agemm.mx_matmul_repacked beside them, at M = 1, 16, 32, 64 on the same five shapes; writes profiles/mxfp6_repacked_decode.json.

Shapes: M = 1, 16, 64, 512, 4096 on N = KQ = 4096 and on the four Qwen2.5-7B linears, KE = 64, bf16 output, no epilogue operands.

Method (tools/mx_repacked_bench.py's, as tools/mx_rw_bench.py uses it): every call is replayed from a HIP graph over weight copies rotated
through > 320 MB (HBM-cold weights), warmed for ~40 ms and timed for >= 10 ms; the three calls of one shape ALTERNATE for `--rounds` rounds
in one process; a record holds each call's median over the rounds and its band (max - min).  A ratio is called a difference only where the
medians differ by more than twice the larger band; nothing here is a pass condition."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from arcquant_amd import agemm  # noqa: E402
from mx_repacked_bench import alternate  # noqa: E402

KE = 64
SHAPES = [("4096x4096", 4096, 4096), ("qkv", 4608, 3584), ("o", 3584, 3584), ("gate_up", 37888, 3584), ("down", 3584, 18944)]
MS = (1, 16, 64, 512, 4096)


def shape(name, M, N, KQ, dev, rounds):
    q = bench.make_problem(M, N, KQ, KE, dev)
    x4, s4 = agemm.mx_reorder_quantize_x(q["x"], q["idx"], KE)
    x6, s6 = agemm.mx6_reorder_quantize_x(q["x"], q["idx"], KE)
    w4, sw4 = agemm.mx_reorder_quantize_w(q["w"], q["idx"], KE)
    w6, sw6 = agemm.mx6_reorder_quantize_w(q["w"], q["idx"], KE)
    Kp = s4.shape[1] * 32
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    c4 = [(w4.clone(), sw4.clone()) for _ in range(rot)]
    c6 = [(w6.clone(), sw6.clone()) for _ in range(rot)]
    o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    calls = {"mxfp4": lambda i: agemm.mx_matmul(x4, c4[i][0], s4, c4[i][1], 1.0, out=o),
             "mxfp6": lambda i: agemm.mx6_matmul(x6, c6[i][0], s6, c6[i][1], 1.0, out=o),
             "w4a6": lambda i: agemm.mx6_matmul(x6, c4[i][0], s6, c4[i][1], 1.0, b_format="e2m1", out=o)}
    t = alternate({k: [(lambda i=i, f=f: f(i)) for i in range(rot)] for k, f in calls.items()}, rounds)
    rec = {"shape": name, "M": M, "N": N, "KQ": KQ, "Kp": Kp, "kernel": "small" if M <= 64 else "tile"}
    for k in calls:
        rec[k + "_us"], rec[k + "_band_us"] = round(t[k][0], 2), round(t[k][1], 2)
    for k, wbytes in (("mxfp6", 25 / 32), ("w4a6", 17 / 32)):
        bar = 2 * max(t[k][1], t["mxfp4"][1])
        rec[k + "_over_mxfp4"] = round(t[k][0] / t["mxfp4"][0], 3)
        rec[k + "_verdict"] = "slower" if t[k][0] - t["mxfp4"][0] > bar else "faster" if t["mxfp4"][0] - t[k][0] > bar else "no difference beyond the bands"
        rec[k + "_GBps"] = round((N * Kp * wbytes + M * Kp * 25 / 32 + M * N * 2) / t[k][0] / 1e3, 1)
        rec[k + "_TFLOPs"] = round(2.0 * M * N * Kp / t[k][0] / 1e6, 1)
    del c4, c6, q
    torch.cuda.empty_cache()
    return rec


REPACKED_MS = (1, 16, 32, 64)


def repacked_shape(name, M, N, KQ, dev, rounds):
    """--table repacked: agemm.mx6_matmul_repacked against agemm.mx6_matmul (the reference-layout kernel of the same library) for both weight
    formats, with agemm.mx_matmul_repacked (MXFP4) beside them for scale; five calls alternating."""
    q = bench.make_problem(M, N, KQ, KE, dev)
    x4, s4 = agemm.mx_reorder_quantize_x(q["x"], q["idx"], KE)
    x6, s6 = agemm.mx6_reorder_quantize_x(q["x"], q["idx"], KE)
    w4, sw4 = agemm.mx_reorder_quantize_w(q["w"], q["idx"], KE)
    w6, sw6 = agemm.mx6_reorder_quantize_w(q["w"], q["idx"], KE)
    Kp = s4.shape[1] * 32
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    c4 = [(w4.clone(), sw4.clone()) for _ in range(rot)]
    c6 = [(w6.clone(), sw6.clone()) for _ in range(rot)]
    r4 = [tuple(t.clone() for t in agemm.mx_repack_w(w4, sw4)) for _ in range(rot)]
    r6 = [tuple(t.clone() for t in agemm.mx6_repack_w(w6, sw6)) for _ in range(rot)]
    o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    calls = {"mxfp4_repacked": lambda i: agemm.mx_matmul_repacked(x4, r4[i][0], s4, r4[i][1], 1.0, N, out=o),
             "mxfp6": lambda i: agemm.mx6_matmul(x6, c6[i][0], s6, c6[i][1], 1.0, out=o),
             "mxfp6_repacked": lambda i: agemm.mx6_matmul_repacked(x6, r6[i][0], s6, r6[i][1], 1.0, N, out=o),
             "w4a6": lambda i: agemm.mx6_matmul(x6, c4[i][0], s6, c4[i][1], 1.0, b_format="e2m1", out=o),
             "w4a6_repacked": lambda i: agemm.mx6_matmul_repacked(x6, r4[i][0], s6, r4[i][1], 1.0, N, b_format="e2m1", out=o)}
    # before anything is timed: W4A6 bit for bit; MXFP6 (the same products in another grouping) within a bf16 rounding, or, where the
    # sum cancels, within 1e-4 of the largest output (tests/test_mx6_repacked_gpu.py holds the element-wise bound)
    assert torch.equal(calls["w4a6"](0).clone(), calls["w4a6_repacked"](0)), f"{name} M={M}: W4A6 layouts disagree: nothing to time"
    a, b = calls["mxfp6"](0).float().clone(), calls["mxfp6_repacked"](0).float()
    assert ((a - b).abs() <= 2.0 ** -7 * a.abs() + 1e-4 * a.abs().max()).all(), f"{name} M={M}: MXFP6 layouts disagree: nothing to time"
    t = alternate({k: [(lambda i=i, f=f: f(i)) for i in range(rot)] for k, f in calls.items()}, rounds)
    rec = {"shape": name, "M": M, "N": N, "KQ": KQ, "Kp": Kp}
    for k in calls:
        rec[k + "_us"], rec[k + "_band_us"] = round(t[k][0], 2), round(t[k][1], 2)
    for k, wbytes in (("mxfp6", 25 / 32), ("w4a6", 17 / 32)):
        (r_us, r_band), (p_us, p_band) = t[k], t[k + "_repacked"]
        bar = 2 * max(r_band, p_band)
        rec[k + "_speedup"] = round(r_us / p_us, 3)
        rec[k + "_verdict"] = "repacked faster" if r_us - p_us > bar else "reference layout faster" if p_us - r_us > bar else "no difference beyond the bands"
        rec[k + "_repacked_GBps"] = round((N * Kp * wbytes + M * Kp * 25 / 32 + M * N * 2) / p_us / 1e3, 1)
    rec["mxfp6_repacked_over_mxfp4_repacked"] = round(t["mxfp6_repacked"][0] / t["mxfp4_repacked"][0], 3)
    rec["w4a6_repacked_over_mxfp4_repacked"] = round(t["w4a6_repacked"][0] / t["mxfp4_repacked"][0], 3)
    del c4, c6, r4, r6, q
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table", choices=("gemm", "repacked"), default="gemm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx6_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    if a.table == "repacked":
        res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
               "shapes": [repacked_shape(n, M, N, KQ, dev, a.rounds) for n, N, KQ in SHAPES for M in REPACKED_MS],
               "note": ("us per call, HIP-graph replay over weight copies rotated through > 320 MB (HBM-cold); the five calls alternate in one "
                        "process; *_us = median of the rounds, *_band_us = max - min; *_speedup = mx6_matmul_us / mx6_matmul_repacked_us for that "
                        "weight format; a verdict other than 'no difference' needs the medians to differ by more than twice the larger band; "
                        "*_repacked_GBps = codes + scales of both operands + the bf16 output over the repacked time")}
        a.out = a.out or os.path.join(ROOT, "profiles", "mxfp6_repacked_decode.json")
        line = json.dumps(res, indent=1)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "mxfp6_gemm.json")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "shapes": [shape(n, M, N, KQ, dev, a.rounds) for n, N, KQ in SHAPES for M in MS],
           "note": ("us per call, HIP-graph replay over weight copies rotated through > 320 MB (HBM-cold); the three calls alternate in one process; "
                    "*_us = median of the rounds, *_band_us = max - min; *_over_mxfp4 = time ratio against mx_matmul (> 1: slower); a verdict other "
                    "than 'no difference' needs the medians to differ by more than twice the larger band; *_GBps = codes + scales of both operands "
                    "+ the bf16 output over the time")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
