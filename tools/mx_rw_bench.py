#!/usr/bin/env python3
"""The MXFP4 GEMMs that serve every batch size from the repacked weight (agemm.mx_matmul_rw, mx.matmul_silu_mul_rw,
mx.matmul_silu_mul_quantize_rw) against the same GEMMs on the reference-layout weight (agemm.mx_matmul, mx.matmul_silu_mul,
mx.matmul_silu_mul_quantize) on the MI355X; writes profiles/mxfp4_rw.json.

    python tools/mx_rw_bench.py [--rounds R] [--out FILE]

Shapes: the tile kernel over the repacked weight at M = 128, 512, 4096 on the four Qwen2.5-7B linears (q|k|v with bias, o and down with
the residual, gate|up with SiLU*up and with the quantising epilogue) and at 4096 x 4096; the quantising decode kernel at M = 4, 16, 64 on the
gate|up shape.

Method (tools/mx_repacked_bench.py's): every call is replayed from a HIP graph over weight copies rotated through > 320 MB (HBM-cold
weights), warmed for ~40 ms and timed for >= 10 ms.  The two calls of one shape ALTERNATE for `--rounds` rounds in one process on the same
weight; a record holds each call's median over the rounds and its band (max - min).  Before anything is timed the two outputs are compared
with torch.equal.  "faster" is claimed only where the medians differ by more than twice the larger band (DESIGN.md 3.2's bar); a shape
that does not clear it is reported as it came out."""
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
from arcquant_amd import agemm, mx  # noqa: E402
from mx_repacked_bench import alternate  # noqa: E402

KE = 64
# (name, N, KQ, epilogues): the four linears of Qwen2.5-7B (hidden 3584, intermediate 18944; q|k|v = 3584 + 2 * 512)
QWEN = [("qkv", 4608, 3584, ("bias",)), ("o", 3584, 3584, ("residual",)), ("gate_up", 37888, 3584, ("silu_mul", "silu_mul_quantize")),
        ("down", 3584, 18944, ("residual",))]


def shape(name, M, N, KQ, epilogue, dev, rounds):
    q = bench.make_problem(M, N, KQ, KE, dev)
    qx, sx = agemm.mx_reorder_quantize_x(q["x"], q["idx"], KE)
    qw, sw = agemm.mx_reorder_quantize_w(q["w"], q["idx"], KE)
    mrw, mrsf = agemm.mx_repack_w(qw, sw)
    Kp = qx.shape[1] * 2
    g = torch.Generator(device=dev).manual_seed(N)
    kw = {}
    if epilogue in ("bias", "silu_mul", "silu_mul_quantize"):
        kw["bias"] = (torch.randn(N, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    if epilogue == "residual":
        kw["residual"] = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    rot = max(2, int(320e6 // (N * Kp * 17 / 32)) + 1)
    ws = [(qw.clone(), sw.clone()) for _ in range(rot)]
    rs = [(mrw.clone(), mrsf.clone()) for _ in range(rot)]
    if epilogue == "silu_mul_quantize":
        names = ("matmul_silu_mul_quantize", "matmul_silu_mul_quantize_rw")
        out_bytes = M * ((N // 2 + KE + 127) // 128 * 128) * 17 // 32
        ref = lambda i: mx.matmul_silu_mul_quantize(qx, ws[i][0], sx, ws[i][1], 1.0, KE, **kw)                      # noqa: E731
        rep = lambda i: mx.matmul_silu_mul_quantize_rw(qx, rs[i][0], sx, rs[i][1], 1.0, N, KE, **kw)                # noqa: E731
        same = all(torch.equal(a, b) for a, b in zip(ref(rot - 1), rep(rot - 1)))
    else:
        silu = epilogue == "silu_mul"
        names = ("matmul_silu_mul", "matmul_silu_mul_rw") if silu else ("mx_matmul", "mx_matmul_rw")
        o = torch.empty((M, N // 2 if silu else N), dtype=torch.bfloat16, device=dev)
        out_bytes = o.numel() * 2
        if silu:
            ref = lambda i: mx.matmul_silu_mul(qx, ws[i][0], sx, ws[i][1], 1.0, out=o, **kw)                        # noqa: E731
            rep = lambda i: mx.matmul_silu_mul_rw(qx, rs[i][0], sx, rs[i][1], 1.0, N, out=o, **kw)                  # noqa: E731
        else:
            ref = lambda i: agemm.mx_matmul(qx, ws[i][0], sx, ws[i][1], 1.0, out=o, **kw)                           # noqa: E731
            rep = lambda i: agemm.mx_matmul_rw(qx, rs[i][0], sx, rs[i][1], 1.0, N, out=o, **kw)                     # noqa: E731
        a = ref(rot - 1).clone()
        same = torch.equal(a.view(torch.int16), rep(rot - 1).view(torch.int16))
    assert same, f"{name} M={M} {epilogue}: the two layouts disagree: nothing to time"
    chains = {names[0]: [(lambda i=i: ref(i)) for i in range(rot)], names[1]: [(lambda i=i: rep(i)) for i in range(rot)]}
    t = alternate(chains, rounds)
    (r_us, r_band), (p_us, p_band) = t[names[0]], t[names[1]]
    bar = 2 * max(r_band, p_band)
    verdict = "repacked faster" if r_us - p_us > bar else "reference layout faster" if p_us - r_us > bar else "no difference beyond the bands"
    rec = {"shape": name, "M": M, "N": N, "KQ": KQ, "Kp": Kp, "epilogue": epilogue, "route": agemm.mx_rw_route(M, N, Kp), "outputs_equal": True,
           "reference": names[0], "repacked": names[1], "reference_us": round(r_us, 2), "reference_band_us": round(r_band, 2),
           "repacked_us": round(p_us, 2), "repacked_band_us": round(p_band, 2), "speedup": round(r_us / p_us, 3), "verdict": verdict,
           "repacked_TFLOPs": round(2.0 * M * N * Kp / p_us / 1e6, 1),
           "repacked_GBps": round((N * Kp * 17 / 32 + M * Kp * 17 / 32 + out_bytes) / p_us / 1e3, 1)}
    del ws, rs, q, chains
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_rw.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_rw_bench: needs a GPU (there is no CPU measurement)")
    dev = "cuda:0"
    big = (128, 512, 4096)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "square_4096": [shape("4096x4096", M, 4096, 4096, "plain", dev, a.rounds) for M in big],
           "qwen2.5-7b_linears": [shape(n, M, N, KQ, epi, dev, a.rounds) for n, N, KQ, epis in QWEN for epi in epis for M in big],
           "qwen2.5-7b_gate_up_quantising_decode": [shape("gate_up", M, 37888, 3584, "silu_mul_quantize", dev, a.rounds) for M in (4, 16, 64)],
           "note": ("us per call, HIP-graph replay over weight copies rotated through > 320 MB (HBM-cold); the reference-layout call and the call "
                    "over the repacked weight alternate in one process; *_us = median of the rounds, *_band_us = max - min; verdict: a difference "
                    "counts only beyond twice the larger band; speedup = reference_us / repacked_us; route 2 = the tile kernel over MRW, 1 = the "
                    "decode kernels; repacked_GBps = codes + scales of both operands + the output over the repacked time")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
