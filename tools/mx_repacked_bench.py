#!/usr/bin/env python3
"""The MXFP4 decode GEMMs over the repacked weight (agemm.mx_matmul_repacked, mx.matmul_silu_mul_repacked) against the same GEMMs on the
reference-layout weight (agemm.mx_matmul, mx.matmul_silu_mul) on the MI355X, with NVFP4's agemm.matmul_repacked beside them where
agemm.repacked_supported holds; writes profiles/mxfp4_repacked_decode.json.

    python tools/mx_repacked_bench.py [--rounds R] [--out FILE]

Method (tools/mx_bench.py's): every call is replayed from a HIP graph over weight copies rotated through > 320 MB (HBM-cold weights),
warmed for ~40 ms and timed for >= 10 ms.  The calls of one shape ALTERNATE for `--rounds` rounds in one process on the same weight; a
record holds each call's median over the rounds and its band (max - min).  Before anything is timed the two MXFP4 outputs are compared
with torch.equal.  "faster" is claimed only where the medians differ by more than twice the larger band (DESIGN.md 3.2's bar); a shape
that does not clear it is reported as it came out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import bench  # noqa: E402
from arcquant_amd import agemm, mx  # noqa: E402
from mx_bench import graph_time  # noqa: E402

KE = 64
# (name, N, KQ, epilogue): the four decode linears of Qwen2.5-7B (hidden 3584, intermediate 18944; q|k|v = 3584 + 2 * 512)
QWEN = [("qkv", 4608, 3584, "bias"), ("o", 3584, 3584, "residual"), ("gate_up", 37888, 3584, "silu_mul"), ("down", 3584, 18944, "residual")]


def alternate(chains, rounds):
    """{name: [closures]} -> {name: (median us, band us)}: the chains timed in turn, `rounds` times."""
    seen = {n: [] for n in chains}
    for _ in range(rounds):
        for n, launches in chains.items():
            seen[n].append(graph_time(launches))
    return {n: (statistics.median(t), max(t) - min(t)) for n, t in seen.items()}


def shape(name, M, N, KQ, epilogue, dev, rounds):
    q = bench.make_problem(M, N, KQ, KE, dev)
    qx, sx = agemm.mx_reorder_quantize_x(q["x"], q["idx"], KE)
    qw, sw = agemm.mx_reorder_quantize_w(q["w"], q["idx"], KE)
    mrw, mrsf = agemm.mx_repack_w(qw, sw)
    K, Kp = KQ + KE, qx.shape[1] * 2
    g = torch.Generator(device=dev).manual_seed(N)
    kw = {}
    if epilogue in ("bias", "silu_mul"):
        kw["bias"] = (torch.randn(N, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    if epilogue == "residual":
        kw["residual"] = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    silu = epilogue == "silu_mul"
    o = torch.empty((M, N // 2 if silu else N), dtype=torch.bfloat16, device=dev)
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    ws = [(qw.clone(), sw.clone()) for _ in range(rot)]
    rs = [(mrw.clone(), mrsf.clone()) for _ in range(rot)]
    if silu:
        ref = lambda i: mx.matmul_silu_mul(qx, ws[i][0], sx, ws[i][1], 1.0, out=o, **kw)                          # noqa: E731
        rep = lambda i: mx.matmul_silu_mul_repacked(qx, rs[i][0], sx, rs[i][1], 1.0, N, out=o, **kw)              # noqa: E731
    else:
        ref = lambda i: agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0, out=o, **kw)                             # noqa: E731
        rep = lambda i: agemm.mx_matmul_repacked(qx, rs[i][0], sx, rs[i][1], 1.0, N, out=o, **kw)                 # noqa: E731
    a = ref(rot - 1).clone()
    b = rep(rot - 1).clone()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name} M={M}: the two layouts disagree: nothing to time"
    chains = {"mx_matmul": [(lambda i=i: ref(i)) for i in range(rot)], "mx_matmul_repacked": [(lambda i=i: rep(i)) for i in range(rot)]}
    nv = agemm.repacked_supported(M, N, K)
    if nv:                                       # NVFP4's repacked decode GEMM on the same x / w (plain epilogue on the SiLU shape)
        rw, rsf = agemm.repack_w(q["qw"], q["sfw"])
        nrot = max(2, int(320e6 // (rw.numel() + rsf.numel())) + 1)
        nws = [(rw.clone(), rsf.clone()) for _ in range(nrot)]
        on = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        nkw = {} if silu else kw
        chains["nvfp4_matmul_repacked"] = [(lambda i=i: agemm.matmul_repacked(q["qx"], nws[i][0], q["sfx"], nws[i][1], q["alpha"], N, out=on, **nkw))
                                           for i in range(nrot)]
    t = alternate(chains, rounds)
    (r_us, r_band), (p_us, p_band) = t["mx_matmul"], t["mx_matmul_repacked"]
    bar = 2 * max(r_band, p_band)
    verdict = "repacked faster" if r_us - p_us > bar else "reference layout faster" if p_us - r_us > bar else "no difference beyond the bands"
    rec = {"shape": name, "M": M, "N": N, "KQ": KQ, "Kp": Kp, "epilogue": epilogue, "outputs_equal": True}
    for n, (us, band) in t.items():
        rec[n + "_us"], rec[n + "_band_us"] = round(us, 2), round(band, 2)
    rec.update(speedup=round(r_us / p_us, 3), verdict=verdict,
               repacked_GBps=round((N * Kp * 17 / 32 + M * Kp * 17 / 32 + o.numel() * 2) / p_us / 1e3, 1))
    if nv:
        rec["repacked_vs_nvfp4"] = round(t["nvfp4_matmul_repacked"][0] / p_us, 3)
    del ws, rs, q, chains
    if nv:
        del nws
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_repacked_decode.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_repacked_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "square_4096": [shape("4096x4096", M, 4096, 4096, "plain", dev, a.rounds) for M in (1, 4, 16, 32, 64)],
           "qwen2.5-7b_decode_linears": [shape(n, M, N, KQ, epi, dev, a.rounds) for n, N, KQ, epi in QWEN for M in (4, 64)],
           "note": ("us per call, HIP-graph replay over weight copies rotated through > 320 MB (HBM-cold); mx_matmul, mx_matmul_repacked "
                    "(mx.matmul_silu_mul / _repacked on the silu_mul shape) and NVFP4's matmul_repacked alternate in one process; *_us = median "
                    "of the rounds, *_band_us = max - min; verdict: a difference counts only beyond twice the larger band; speedup = "
                    "mx_matmul_us / mx_matmul_repacked_us; repacked_GBps = codes + scales of both operands + the output over the repacked time")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
