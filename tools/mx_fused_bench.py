#!/usr/bin/env python3
"""The MXFP4 decoder-layer operators (arcquant_amd/mx.py) on the MI355X, each against the chain of launches that gave the same result
before it existed, and the NVFP4 counterparts, in one process; prints ONE JSON line (the evidence behind
profiles/mxfp4_fused_ops.json).

    python tools/mx_fused_bench.py [--rounds R] [--table {all,fused,quant_epilogue}] [--out FILE]

Method (tools/mx_bench.py's): every chain is replayed from a HIP graph over inputs / weight copies rotated through > 320 MB (HBM-cold
weights at decode sizes), warmed for ~40 ms and timed for >= 10 ms.  The chains of one shape ALTERNATE for `--rounds` rounds in the same
warm state; a record holds the best round of each chain and `round_spread`, the largest (max - min) / min any chain of the record showed
between rounds -- ratios closer to 1 than that are not a difference.  Run the command twice to see the run-to-run spread.

  rmsnorm   torch's RMSNorm ops (Qwen2RMSNorm) + mx_reorder_quantize_x      against  mx.rmsnorm_quantize_x
  gate|up   mx_matmul + F.silu * up + mx_reorder_quantize_x                  against  mx.matmul_silu_mul + mx_reorder_quantize_x  (epilogue)
                                                                             and      mx_matmul + mx.silu_mul_quantize_x(GU_PAIRS) (quantiser)

Second table (--table quant_epilogue, the evidence behind profiles/mxfp4_quant_epilogue.json), the same protocol at M = 4, 16, 64, 4096:
  gate|up   mx.matmul_silu_mul + mx_reorder_quantize_x (the chain above)     against  mx.matmul_silu_mul_quantize  (one launch)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from arcquant_amd import agemm, mx  # noqa: E402
from mx_bench import graph_time  # noqa: E402

KE, EPS = 64, 1e-6


def alternate(chains, rounds):
    """{name: [closures]} -> ({name: best us}, spread): the chains timed in turn, `rounds` times."""
    seen = {n: [] for n in chains}
    for _ in range(rounds):
        for n, launches in chains.items():
            seen[n].append(graph_time(launches))
    return {n + "_us": round(min(t), 2) for n, t in seen.items()}, round(max((max(t) - min(t)) / min(t) for t in seen.values()), 3)


def torch_rmsnorm(x, w):
    """Qwen2RMSNorm.forward: fp32 statistics, bf16 before the weight multiply."""
    xf = x.float()
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)).to(torch.bfloat16)


def rmsnorm(M, KQ, dev, rounds):
    rot = max(2, min(16, int(320e6 // (M * KQ * 2)) + 1))
    xs = [bench.outlier_activations(M, KQ, dev, seed=i) for i in range(rot)]
    w = (torch.rand(KQ, device=dev) + 0.5).to(torch.bfloat16)
    idx = torch.arange(KQ, dtype=torch.int16, device=dev)
    chains = {
        "torch_rmsnorm_then_mx_quantize": [(lambda i=i: agemm.mx_reorder_quantize_x(torch_rmsnorm(xs[i], w), idx, KE)) for i in range(rot)],
        "mx_rmsnorm_quantize": [(lambda i=i: mx.rmsnorm_quantize_x(xs[i], w, EPS, idx, KE)) for i in range(rot)],
        "nvfp4_rmsnorm_quantize": [(lambda i=i: agemm.rmsnorm_quantize_x(xs[i], w, EPS, idx, KE)) for i in range(rot)],
    }
    t, spread = alternate(chains, rounds)
    rec = {"M": M, "KQ": KQ, **t, "round_spread": spread,
           "fused_speedup": round(t["torch_rmsnorm_then_mx_quantize_us"] / t["mx_rmsnorm_quantize_us"], 3),
           "vs_nvfp4": round(t["nvfp4_rmsnorm_quantize_us"] / t["mx_rmsnorm_quantize_us"], 3)}
    del xs
    torch.cuda.empty_cache()
    return rec


def gate_up(M, dev, rounds, KQ=3584, inter=18944):
    N = 2 * inter
    from arcquant_amd import qlinear
    x = bench.outlier_activations(M, KQ, dev)
    w = (torch.randn(N, KQ, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.05).to(torch.bfloat16)   # rows: g0, u0, g1, u1, ...
    idx = torch.arange(KQ, dtype=torch.int16, device=dev)
    idx_i = torch.arange(inter, dtype=torch.int16, device=dev)
    qx, sx = agemm.mx_reorder_quantize_x(x, idx, KE)
    qw, sw = agemm.mx_reorder_quantize_w(w, idx, KE)
    q = {}
    q["qw"], q["sfw"], s_w = qlinear.NVFP4_reorder_quantize_w(w, idx, KE)
    q["qx"], q["sfx"], s_x = qlinear.NVFP4_reorder_quantize_x(x, idx, KE)
    q["alpha"] = (s_x * s_w).reshape(1)
    del w
    Kp, K = qx.shape[1] * 2, KQ + KE
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    ws = [(qw.clone(), sw.clone()) for _ in range(rot)]
    nws = [(q["qw"].clone(), q["sfw"].clone()) for _ in range(max(2, int(320e6 // (N * K * 9 / 16)) + 1))]

    def unfused(i):
        y = agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0)
        return agemm.mx_reorder_quantize_x(F.silu(y[:, 0::2]) * y[:, 1::2], idx_i, KE)

    def nvfp4(i):
        act, slots = agemm.matmul_silu_mul(q["qx"], nws[i][0], q["sfx"], nws[i][1], q["alpha"])
        return agemm.reorder_quantize_x_dynamic(act, idx_i, KE, absmax_slots=slots)

    chains = {
        "mx_matmul_torch_silu_mul_quantize": [(lambda i=i: unfused(i)) for i in range(rot)],
        "epilogue_gemm_then_quantize": [(lambda i=i: agemm.mx_reorder_quantize_x(mx.matmul_silu_mul(qx, ws[i][0], sx, ws[i][1], 1.0), idx_i, KE))
                                        for i in range(rot)],
        "mx_matmul_then_silu_quantiser": [(lambda i=i: mx.silu_mul_quantize_x(agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0), idx_i, KE,
                                                                              layout=agemm.GU_PAIRS)) for i in range(rot)],
        "mx_matmul_alone": [(lambda i=i: agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0)) for i in range(rot)],
        "nvfp4_epilogue_gemm_then_dynamic_quantize": [(lambda i=i: nvfp4(i)) for i in range(len(nws))],
    }
    t, spread = alternate(chains, rounds)
    base = t["mx_matmul_torch_silu_mul_quantize_us"]
    rec = {"M": M, "N": N, "KQ": KQ, **t, "round_spread": spread,
           "epilogue_speedup": round(base / t["epilogue_gemm_then_quantize_us"], 3),
           "silu_quantiser_speedup": round(base / t["mx_matmul_then_silu_quantiser_us"], 3),
           "epilogue_vs_nvfp4": round(t["nvfp4_epilogue_gemm_then_dynamic_quantize_us"] / t["epilogue_gemm_then_quantize_us"], 3)}
    del ws, nws, q
    torch.cuda.empty_cache()
    return rec


def quant_epilogue(M, dev, rounds, KQ=3584, inter=18944):
    """The two launches from packed operands to the down projection's (QX, SFX) against the one that replaces them."""
    N = 2 * inter
    x = bench.outlier_activations(M, KQ, dev)
    w = (torch.randn(N, KQ, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 0.05).to(torch.bfloat16)   # rows: g0, u0, g1, u1, ...
    idx = torch.arange(KQ, dtype=torch.int16, device=dev)
    idx_i = torch.arange(inter, dtype=torch.int16, device=dev)
    qx, sx = agemm.mx_reorder_quantize_x(x, idx, KE)
    qw, sw = agemm.mx_reorder_quantize_w(w, idx, KE)
    del w
    Kp = qx.shape[1] * 2
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    ws = [(qw.clone(), sw.clone()) for _ in range(rot)]
    a, b = agemm.mx_reorder_quantize_x(mx.matmul_silu_mul(qx, ws[0][0], sx, ws[0][1], 1.0), idx_i, KE), mx.matmul_silu_mul_quantize(qx, ws[0][0], sx, ws[0][1], 1.0, KE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the two forms disagree: nothing to time"
    chains = {
        "epilogue_gemm_then_quantize": [(lambda i=i: agemm.mx_reorder_quantize_x(mx.matmul_silu_mul(qx, ws[i][0], sx, ws[i][1], 1.0), idx_i, KE))
                                        for i in range(rot)],
        "quantising_epilogue_gemm": [(lambda i=i: mx.matmul_silu_mul_quantize(qx, ws[i][0], sx, ws[i][1], 1.0, KE)) for i in range(rot)],
    }
    t, spread = alternate(chains, rounds)
    rec = {"M": M, "N": N, "KQ": KQ, "KE": KE, **t, "round_spread": spread,
           "one_launch_speedup": round(t["epilogue_gemm_then_quantize_us"] / t["quantising_epilogue_gemm_us"], 3)}
    del ws, a, b
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--table", choices=("all", "fused", "quant_epilogue"), default="all")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_fused_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0)}
    if a.table in ("all", "fused"):
        res["rmsnorm_quantize"] = [rmsnorm(M, KQ, dev, a.rounds) for M in (4, 4096) for KQ in (3584, 4096)]
        res["gate_up_qwen2.5-7b"] = [gate_up(M, dev, a.rounds) for M in (4, 64, 4096)]
    if a.table in ("all", "quant_epilogue"):
        res["gate_up_quant_epilogue_qwen2.5-7b"] = [quant_epilogue(M, dev, a.rounds) for M in (4, 16, 64, 4096)]
    res["note"] = ("us per chain, HIP-graph replay over inputs / weights rotated through > 320 MB; best of the alternating rounds; "
                    "round_spread = largest (max - min) / min of a chain between rounds; *_speedup = the parent chain's time over the "
                    "fused form's")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
