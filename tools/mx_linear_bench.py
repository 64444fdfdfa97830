#!/usr/bin/env python3
"""The MXFP4 fused decode linears (mx.linear_rmsnorm_repacked, mx.linear_quantize_repacked, mx.linear_rmsnorm_silu_repacked) against the
two-launch chains they replace (mx.rmsnorm_quantize_x or agemm.mx_reorder_quantize_x, then mx_matmul_repacked /
mx.matmul_silu_mul_repacked) on the MI355X; writes profiles/mxfp4_linear_fused.json.

    python tools/mx_linear_bench.py [--rounds R] [--ms 1,4,8,16] [--out FILE]

Method (tools/mx_bench.py's): every call is replayed from a HIP graph over weight copies rotated through > 320 MB (HBM-cold weights),
warmed for ~40 ms and timed for >= 10 ms.  The fused call and the chain of one shape ALTERNATE for `--rounds` rounds in one process on
the same operands; a record holds each one's median over the rounds and its band (max - min).  Before anything is timed the two
outputs are compared with torch.equal.  A linear counts as WON only where the fused call is faster by more than twice the larger band;
everything else is reported as it came out.  Over a library built with `make EXTRA=-DARCQ_MX_LINEAR_GRID_KNOB`, ARCQ_MX_LINEAR_WGS=n
in the environment caps the fused launch's workgroups (the grid experiment of DESIGN.md 3.6; the product build ignores it); the record
names the workgroups each launch had."""
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

from arcquant_amd import agemm, mx  # noqa: E402
from mx_bench import graph_time  # noqa: E402

KE = 64
EPS = 1e-6
# (name, N, KQ, source, epilogue): the three decode linears of Qwen2.5-7B that can be fused (hidden 3584, intermediate 18944) and a square
SHAPES = [("qkv", 4608, 3584, "rmsnorm", "bias"), ("o", 3584, 3584, "plain", "residual"), ("gate_up", 37888, 3584, "rmsnorm", "silu_mul"),
          ("4096x4096", 4096, 4096, "rmsnorm", "plain")]


def alternate(chains, rounds):
    seen = {n: [] for n in chains}
    for _ in range(rounds):
        for n, launches in chains.items():
            seen[n].append(graph_time(launches))
    return {n: (statistics.median(t), max(t) - min(t)) for n, t in seen.items()}


def shape(name, M, N, KQ, source, epilogue, dev, rounds):
    g = torch.Generator(device=dev).manual_seed(N + KQ + M)
    Kp = mx.mx_k_padded(KQ + KE)
    x = (torch.randn(M, KQ, device=dev, generator=g) * 2).to(torch.bfloat16)
    x[:, -KE:] *= 16                                                  # the outlier channels
    wn = (1 + 0.1 * torch.randn(KQ, device=dev, generator=g)).to(torch.bfloat16)
    idx = torch.arange(KQ, dtype=torch.int16, device=dev)
    qw = torch.randint(0, 256, (N, Kp // 2), device=dev, generator=g, dtype=torch.uint8)
    sw = torch.randint(118, 124, (N, Kp // 32), device=dev, generator=g, dtype=torch.uint8)
    mrw, mrsf = agemm.mx_repack_w(qw, sw)
    del qw, sw
    kw = {}
    if epilogue in ("bias", "silu_mul"):
        kw["bias"] = (torch.randn(N, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    if epilogue == "residual":
        kw["residual"] = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    silu, rms = epilogue == "silu_mul", source == "rmsnorm"
    o = torch.empty((M, N // 2 if silu else N), dtype=torch.bfloat16, device=dev)
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    rs = [(mrw.clone(), mrsf.clone()) for _ in range(rot)]

    def chain(i):
        a, sfa = mx.rmsnorm_quantize_x(x, wn, EPS, idx, KE) if rms else agemm.mx_reorder_quantize_x(x, idx, KE)
        if silu:
            return mx.matmul_silu_mul_repacked(a, rs[i][0], sfa, rs[i][1], 1.0, N, out=o, **kw)
        return mx.mx_matmul_repacked(a, rs[i][0], sfa, rs[i][1], 1.0, N, out=o, **kw)

    def fused(i):
        if silu:
            return mx.linear_rmsnorm_silu_repacked(x, wn, EPS, idx, KE, rs[i][0], rs[i][1], 1.0, N, out=o, **kw)
        if rms:
            return mx.linear_rmsnorm_repacked(x, wn, EPS, idx, KE, rs[i][0], rs[i][1], 1.0, N, out=o, **kw)
        return mx.linear_quantize_repacked(x, idx, KE, rs[i][0], rs[i][1], 1.0, N, out=o, **kw)

    kind = mx.SRC_RMSNORM if rms else mx.SRC_PLAIN
    assert mx.linear_fused_supported(kind, M, N, KQ, KE), f"{name} M={M}: no fused kernel for this shape"
    a = chain(rot - 1).clone()
    b = fused(rot - 1).clone()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a, b), f"{name} M={M}: fused and chain disagree: nothing to time"
    # (a launch of the chain is two kernels: graph_time divides by the closures, so a closure is one whole chain)
    t = alternate({"chain": [(lambda i=i: chain(i)) for i in range(rot)], "fused": [(lambda i=i: fused(i)) for i in range(rot)]}, rounds)
    (c_us, c_band), (f_us, f_band) = t["chain"], t["fused"]
    bar = 2 * max(c_band, f_band)
    verdict = "fused won" if c_us - f_us > bar else "chain won" if f_us - c_us > bar else "no difference beyond the bands"
    rec = {"shape": name, "M": M, "N": N, "KQ": KQ, "KE": KE, "Kp": Kp, "source": source, "epilogue": epilogue, "outputs_equal": True,
           "workgroups": mx.linear_fused_workgroups(kind, N, KQ, KE), "lds_bytes": mx.linear_fused_lds_bytes(kind, KQ, KE),
           "chain_us": round(c_us, 2), "chain_band_us": round(c_band, 2), "fused_us": round(f_us, 2), "fused_band_us": round(f_band, 2),
           "fused_minus_chain_us": round(f_us - c_us, 2), "speedup": round(c_us / f_us, 3), "verdict": verdict}
    del rs
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ms", default="1,4,8,16")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_linear_fused.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_linear_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    ms, names = [int(m) for m in a.ms.split(",")], a.shapes.split(",")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "ARCQ_MX_LINEAR_WGS": os.environ.get("ARCQ_MX_LINEAR_WGS"),
           "linears": [shape(n, M, N, KQ, src, epi, dev, a.rounds) for n, N, KQ, src, epi in SHAPES if n in names for M in ms],
           "note": ("us per linear, HIP-graph replay over weight copies rotated through > 320 MB (HBM-cold); chain = the activation quantiser "
                    "and the repacked GEMM as two launches, fused = one launch; they alternate in one process on the same operands after their "
                    "outputs compared equal; *_us = median of the rounds, *_band_us = max - min; verdict: a difference counts only beyond "
                    "twice the larger band")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
