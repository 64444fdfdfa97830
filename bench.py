#!/usr/bin/env python3
"""bench.py -- the ARC-NVFP4 GEMM benchmark of BASELINE.json on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot-path GEMM (`agemm.matmul`) over one batch of synthetic, already-quantised
input: M=4096 tokens, N=KQ=4096, KE=64 residual channels (K_aug=4160), the shape BASELINE.json's
TFLOP/s metric and its >=70 %-of-fp4-peak target are quoted on.  This follows the reference's own
kernel benchmark, which times the GEMM only (kernels/bench.py:33-43).  Inputs are resident in HBM before
the timed region.  With N > 1 ranks every rank owns one column shard (its own 4096 output columns of a
4096*N-wide layer: column-parallel, no data-path collective), so scaling is "weak".

Rank 0 prints ONE JSON line.  Besides the contract fields it carries
  roofline      -- the dominant kernel against the MFMA roof it actually runs on (fp16/bf16 dense) plus the
                   fraction of the fp4 roof the north star asks about
and, with --full only (a plain run measures the headline and nothing else):
  cpu_baseline  -- oracle/fake_quant.py (our port of the reference's CPU fake-quant path) on host cores
  extra         -- decode-shape (M=1, config[1]) GEMM vs the HBM roof, 8192^2 GEMM, equal-shape fp16
                   rocBLAS GEMM, quantiser timings, Qwen2.5-7B-shape decode tok/s, row-parallel + RCCL timing

--dump-outputs DIR writes what the last timed step computed (the bf16 GEMM output, a fixed sample of its rows, as float32)
to DIR/<name>.npy, so that two builds can be compared output for output on identical, seeded inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0      # MI355X dense bf16/fp16 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_FP4_TFLOPS = 10000.0     # MI355X dense fp4 MFMA (north-star denominator)
PEAK_HBM_GBS = 8000.0         # HBM3E spec (6.3 TB/s achievable)


def outlier_activations(M, K, device, seed=45510):
    """kernels/main.py:13-19 recipe (uniform*3 with x3+3 / x8+8 / x32+32 outlier bands, random signs)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ks, ko = K * 384 // 4096, K * 128 // 4096
    signs = torch.randint(0, 2, (M, K), generator=g).to(torch.bfloat16) * 2 - 1
    x = torch.rand(M, K, generator=g).to(torch.bfloat16) * 3
    x[:, -ks:] = torch.rand(M, ks, generator=g).to(torch.bfloat16) * 3 + 3
    x[:, -ko:] = torch.rand(M, ko, generator=g).to(torch.bfloat16) * 8 + 8
    x[:, -16:] = torch.rand(M, 16, generator=g).to(torch.bfloat16) * 32 + 32
    return (x * signs).to(device)


def make_problem(M, N, KQ, KE, device, seed=45510):
    from arcquant_amd import qlinear
    x = outlier_activations(M, KQ, device, seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    w = (torch.rand(N, KQ, generator=g) * 3).to(torch.bfloat16).to(device)
    idx = torch.arange(KQ, dtype=torch.int16, device=device)
    qw, sfw, sw = qlinear.NVFP4_reorder_quantize_w(w, idx, KE)
    qx, sfx, sx = qlinear.NVFP4_reorder_quantize_x(x, idx, KE)
    return dict(x=x, w=w, idx=idx, qx=qx, sfx=sfx, sx=sx, qw=qw, sfw=sfw, sw=sw, alpha=(sx * sw).reshape(1))


def dequant_fp16(Q, SF, rows, K):
    """Format-spec dequantisation of a packed operand (e2m1 codes, swizzled ue4m3 scales) to fp16 [rows, K] with torch ops: the
    values the GEMM kernels contract (exact in fp16).  Comparator data only."""
    dev = Q.device
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float32, device=dev)
    codes = torch.stack([Q & 15, Q >> 4], dim=-1).reshape(rows, K).long()
    r = torch.arange(rows, device=dev).unsqueeze(1)
    g = torch.arange(K // 16, device=dev).unsqueeze(0)
    off = ((r // 128) * (K // 64) + g // 4) * 512 + (r % 32) * 16 + ((r // 32) % 4) * 4 + g % 4
    sc = SF[off].view(torch.float8_e4m3fn).float()
    return (lut[codes] * sc.repeat_interleave(16, dim=1)).to(torch.float16)


def time_events(fn, iters, warmup):
    """Average device time of fn() in microseconds, HIP events on torch's current stream (the stream the
    C-ABI launches on)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def time_events_steady(fn, iters, warm_ms=60.0):
    """time_events after `warm_ms` of back-to-back launches: from idle the GPU's power management first lowers and then
    raises the clocks, and a compute-bound kernel only reaches its sustained duration after ~30 ms of continuous load
    (tools/clock_transient.py: the 4096^2 GEMM runs 152 -> 116 -> 112 -> 107 -> 105 -> 103 us per launch over its first 300
    launches, the fp16 library GEMM 113 -> 99).  Used for both sides of every comparison."""
    done_ms, chunk, t = 0.0, 20, 1.0
    while done_ms < warm_ms:                       # chunks timed by events: a cold first call cannot shorten the warm-up
        t = time_events(fn, chunk, 0)
        done_ms += t * chunk / 1e3
        chunk = min(chunk * 2, 400)
    # time at least ~30 ms: the clocks keep breathing by several percent over a few milliseconds even in the sustained state
    return time_events(fn, max(iters, min(2000, int(30e3 / max(t, 1.0)))), 5)


def gemm_flops(M, N, K):
    return 2.0 * M * N * K


def gemm_bytes(M, N, K):
    """Algorithmic HBM bytes of one ARC-NVFP4 GEMM launch: packed B + its scales, packed A
    + its scales, bf16 D."""
    return N * K * 9 / 16 + M * K * 9 / 16 + 2 * M * N


def dump_output(dirname, name, t, rows):
    """Write `rows` rows of the 2-D output `t` (all of them if it has fewer), chosen by a fixed seed, to dirname/name.npy as float32.
    bf16 -> float32 is exact; the sample keeps the files small (the full 4096 x 4096 output is 64 MB in float32)."""
    import numpy as np
    if t.shape[0] > rows:
        sel = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:rows].sort().values
        t = t[sel.to(t.device)]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, name + ".npy"), t.float().cpu().numpy())


def bench_extra(args, device, rank):
    from arcquant_amd import agemm
    extra = {}

    def graph_time(launches, reps=10):
        """us per launch of a list of zero-arg launch closures replayed from ONE HIP graph (host launch overhead
        of the Python shim does not pace the GPU; the inter-kernel gap of ~1.5-2 us is included)."""
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
        # warm for ~40 ms of replays (the clock ramp after idle, see time_events_steady), then time >= reps replays / ~10 ms
        per_replay_ms = max(e0.elapsed_time(e1) / 3, 1e-3)
        for _ in range(min(20000, int(40.0 / per_replay_ms))):
            g.replay()
        reps = max(reps, min(20000, int(10.0 / per_replay_ms)))
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (reps * len(launches))

    # ---- decode shapes (BASELINE config[1] = M=1, N=KQ=4096, KE=64; config[2] Llama-3-8B linears; config[3] Qwen2.5-7B decode):
    #      weights rotated through > 320 MB so that they stream from HBM, not from the Infinity Cache.  Per shape: the GEMM on
    #      the reference layout (agemm.matmul), on the repacked decode copy (agemm.matmul_repacked), and the equal-shape fp16
    #      library GEMM (torch.matmul = hipBLASLt / rocBLAS, 3.6x the operand bytes) -- the regime where north_star's
    #      ">= 3.5x fp16 rocBLAS" is physically reachable.
    KE = 64
    for (m, n, kq) in [(1, 4096, 4096), (4, 4096, 4096), (16, 4096, 4096), (1, 14336, 4096), (1, 4096, 14336), (1, 1024, 4096),
                       (4, 3584, 3584), (4, 10752, 3584), (4, 37888, 3584), (4, 3584, 18944),
                       # config[4], one rank of Llama-3-70B TP=8 at bs=4: q|k|v and gate|up column shards (N = 10240/8, 57344/8),
                       # o / down row shards (the largest K slice of tp.k_slices: 1088 and 3648 of K_aug = 8256 / 28736)
                       (4, 1280, 8192), (4, 7168, 8192), (4, 8192, 1024), (4, 8192, 3584)]:
        q = make_problem(m, n, kq, KE, device)
        K = kq + KE
        rot = max(2, int(320e6 // (n * K * 9 / 16)) + 1)
        o = torch.empty((m, n), dtype=torch.bfloat16, device=device)
        gb = gemm_bytes(m, n, K)
        rec = {}
        qws = [q["qw"].clone() for _ in range(rot)]
        sfws = [q["sfw"].clone() for _ in range(rot)]
        t_ref = graph_time([(lambda i=i: agemm.matmul(q["qx"], qws[i], q["sfx"], sfws[i], q["alpha"], out=o)) for i in range(rot)])
        rec["reference_layout_us"] = round(t_ref, 3)
        del qws, sfws
        best = t_ref
        if agemm.repacked_supported(m, n, K):
            rps = [agemm.repack_w(q["qw"].clone(), q["sfw"].clone()) for _ in range(rot)]
            t_rp = graph_time([(lambda i=i: agemm.matmul_repacked(q["qx"], rps[i][0], q["sfx"], rps[i][1], q["alpha"], n, out=o)) for i in range(rot)])
            rec["repacked_us"] = round(t_rp, 3)
            best = min(best, t_rp)
            del rps
        rot16 = max(2, int(320e6 // (n * K * 2)) + 1)
        a16 = torch.randn(m, K, dtype=torch.float16, device=device)
        b16 = [torch.randn(n, K, dtype=torch.float16, device=device) for _ in range(rot16)]
        o16 = torch.empty((m, n), dtype=torch.float16, device=device)
        t16 = graph_time([(lambda i=i: torch.matmul(a16, b16[i].t(), out=o16)) for i in range(rot16)])
        # torch.matmul at M = 1 is a weak GEMV (1.6 TB/s at N = K = 4096): the other library entry points for the same product,
        # same protocol; the fastest one is the comparator the speed-up is quoted against
        alts = {"torch.matmul": t16}
        try:
            alts["F.linear"] = graph_time([(lambda i=i: torch.nn.functional.linear(a16, b16[i])) for i in range(rot16)])
            if m == 1:
                v16, ov = a16[0].contiguous(), torch.empty((n,), dtype=torch.float16, device=device)
                alts["torch.mv"] = graph_time([(lambda i=i: torch.mv(b16[i], v16, out=ov)) for i in range(rot16)])
            bias16 = torch.zeros((n,), dtype=torch.float16, device=device)
            alts["torch.addmm"] = graph_time([(lambda i=i: torch.addmm(bias16, a16, b16[i].t(), out=o16)) for i in range(rot16)])
        except Exception as e:
            alts["error"] = repr(e)[:120]
        times = {k: v for k, v in alts.items() if isinstance(v, float)}
        best16_name = min(times, key=times.get)
        best16 = times[best16_name]
        del b16
        rec.update({"us_per_launch_graph": round(best, 3), "GBps": round(gb / best / 1e3, 1), "frac_hbm_peak": round(gb / best / 1e3 / PEAK_HBM_GBS, 4),
                    "fp16_rocblas_us": round(t16, 3), "speedup_vs_fp16_rocblas": round(t16 / best, 2),
                    "fp16_best_us": round(best16, 3), "fp16_best_call": best16_name, "fp16_best_GBps": round(n * K * 2 / best16 / 1e3, 1),
                    "speedup_vs_fp16_best": round(best16 / best, 2),
                    "fp16_calls_us": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in alts.items()}})
        extra[f"decode_gemm_M{m}_N{n}_KQ{kq}"] = rec
        del q
        torch.cuda.empty_cache()
    extra["decode_note"] = ("HIP-graph replay over weight copies totalling > 320 MB (ours and the fp16 library GEMM alike); per-launch time includes "
                            "the inter-kernel gap; us_per_launch_graph / GBps are the faster of the two layouts; a read-only kernel for 9.6 MB "
                            "takes 3.3 us back to back (tools/probe_stream.hip), a dependent no-op graph node 1.7 us")

    # ---- 8192^2 GEMM and the equal-shape fp16 library GEMM (hipBLASLt/rocBLAS through torch.matmul)
    for S in (4096, 8192):
        q = make_problem(S, S, S, 64, device)
        Kq = S + 64
        # two sustained windows each, the faster one reported: the first window of a kernel that has not run yet can still
        # sit in the power-management ramp after 60 ms (observed on the library GEMM: 117 us, then 96-97 us ever after)
        t = min(time_events_steady(lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"]), 50) for _ in range(2))
        a16 = torch.randn(S, Kq, dtype=torch.float16, device=device)
        b16 = torch.randn(S, Kq, dtype=torch.float16, device=device)
        t16 = min(time_events_steady(lambda: torch.matmul(a16, b16.t()), 50) for _ in range(2))
        # ... and the library GEMM on the SAME operand values (the dequantised NVFP4 operands: <= 6 significant bits each, exact in fp16).
        # The matrix pipe is power-limited and its clock depends on the operands' bit density: on these values the library runs 15-20 %
        # faster than on randn data (tools/mfma_dtype_power_probe.py) -- this, not the randn figure, is the like-for-like comparator
        a16.copy_(dequant_fp16(q["qx"], q["sfx"], S, Kq))
        b16.copy_(dequant_fp16(q["qw"], q["sfw"], S, Kq))
        t16s = min(time_events_steady(lambda: torch.matmul(a16, b16.t()), 50) for _ in range(2))
        extra[f"gemm_{S}"] = {"us": round(t, 2), "TFLOPs": round(gemm_flops(S, S, Kq) / t / 1e6, 1),
                              "fp16_rocblas_us": round(t16, 2), "fp16_rocblas_TFLOPs": round(gemm_flops(S, S, Kq) / t16 / 1e6, 1),
                              "speedup_vs_fp16_rocblas": round(t16 / t, 3),
                              "fp16_rocblas_same_values_us": round(t16s, 2), "fp16_rocblas_same_values_TFLOPs": round(gemm_flops(S, S, Kq) / t16s / 1e6, 1),
                              "speedup_vs_fp16_rocblas_same_values": round(t16s / t, 3),
                              "note": "fp16_rocblas = torch.matmul (hipBLASLt) on randn fp16 operands; _same_values = the same call on the dequantised NVFP4 "
                                      "operands of this problem (no dequantisation inside it: what the in-loop conversion of the fused kernel costs)"}
        # activation quantiser on the same shape (HBM-bound: 2 B in, 9/16 B out per element)
        xs = (q["x"] / q["sx"]).contiguous()
        tq = time_events_steady(lambda: agemm.reorder_quantize_x(xs, q["idx"], 64), 50, 20.0)
        tqg = graph_time([lambda: agemm.reorder_quantize_x(xs, q["idx"], 64)] * 8)      # device time: the eager call is partly host-paced
        # ... and with inputs rotated through > 320 MB, so that the 33.5 MB input of the 4096^2 case is not served from the Infinity
        # Cache launch after launch (tools/quant_cold_probe.py: 12.0 -> 14.5 us); `us` / `GBps` are this HBM-cold figure
        rot = max(2, int(320e6 // (S * S * 2)) + 1)
        xr = [xs] + [xs.clone() for _ in range(rot - 1)]
        tqc = graph_time([(lambda i=i: agemm.reorder_quantize_x(xr[i], q["idx"], 64)) for i in range(rot)])
        qbytes = S * S * 2 + S * Kq * 9 / 16
        extra[f"quantize_x_{S}"] = {"us": round(tqc, 2), "GBps": round(qbytes / tqc / 1e3, 1), "us_same_input": round(tqg, 2),
                                    "GBps_same_input": round(qbytes / tqg / 1e3, 1), "us_eager_python": round(tq, 2)}
        del q, a16, b16, xs, xr
    torch.cuda.empty_cache()
    # ---- SURVEY 8-d sweep: token counts at N=KQ=4096 KE=64, plus KE=0 and the reference bench's K=5888 (bench_nvfp4.cu:25)
    sweep = {}
    for (m, n, kq, ke) in [(128, 4096, 4096, 64), (1024, 4096, 4096, 64), (8192, 4096, 4096, 64), (4096, 4096, 4096, 0),
                           (4096, 4096, 5888, 0)]:
        q = make_problem(m, n, kq, ke, device)
        t = time_events_steady(lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"]), 50)
        sweep[f"M{m}_N{n}_KQ{kq}_KE{ke}"] = {"us": round(t, 2), "TFLOPs": round(gemm_flops(m, n, kq + ke) / t / 1e6, 1)}
        del q
    extra["gemm_sweep"] = sweep
    # ---- the reference's own kernel benchmark (kernels/bench.py:8-49): agemm.matmul at N = K = 4096, KE = 0, M = 8 ... 4096, every M
    #      against the roof that bounds it.  M <= 512: weights rotated through > 320 MB (HBM-cold), HIP-graph replay; above:
    #      sustained eager launches.  `us` is the faster of the reference-layout kernel and, where it applies (M <= 64), the
    #      repacked weight-streaming kernel; both are listed.
    ref_sweep = {}
    for m in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        n = kq = 4096
        q = make_problem(m, n, kq, 0, device)
        gbytes, gflops = gemm_bytes(m, n, kq), gemm_flops(m, n, kq)
        rec = {}
        if m <= 512:
            rot = max(2, int(320e6 // (n * kq * 9 / 16)) + 1)
            o = torch.empty((m, n), dtype=torch.bfloat16, device=device)
            qws, sfws = [q["qw"].clone() for _ in range(rot)], [q["sfw"].clone() for _ in range(rot)]
            rec["reference_layout_us"] = round(graph_time([(lambda i=i: agemm.matmul(q["qx"], qws[i], q["sfx"], sfws[i], q["alpha"], out=o)) for i in range(rot)]), 2)
            t = rec["reference_layout_us"]
            if agemm.repacked_supported(m, n, kq):
                rps = [agemm.repack_w(qws[i], sfws[i]) for i in range(rot)]
                rec["repacked_us"] = round(graph_time([(lambda i=i: agemm.matmul_repacked(q["qx"], rps[i][0], q["sfx"], rps[i][1], q["alpha"], n, out=o))
                                                       for i in range(rot)]), 2)
                t = min(t, rec["repacked_us"])
                del rps
            del qws, sfws
        else:
            t = round(time_events_steady(lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"]), 50, 30.0), 2)
        t_hbm, t_mfma = gbytes / (PEAK_HBM_GBS * 1e3), gflops / (PEAK_F16_TFLOPS * 1e6)          # us at the two roofs
        bound = "hbm" if t_hbm >= t_mfma else "mfma"
        rec.update({"us": t, "TFLOPs": round(gflops / t / 1e6, 1), "GBps": round(gbytes / t / 1e3, 1), "bound": bound,
                    "frac_of_bounding_roof": round(max(t_hbm, t_mfma) / t, 4)})
        ref_sweep[f"M{m}"] = rec
        del q
        torch.cuda.empty_cache()
    ref_sweep["note"] = ("kernels/bench.py shape: N = K = 4096, KE = 0; bound = the larger of bytes / 8 TB/s and flops / 2.5 PFLOP/s (fp16 MFMA: "
                         "the exact contraction's roof); M <= 512 HBM-cold under graph replay")
    extra["reference_m_sweep"] = ref_sweep
    # ---- the prefill GEMMs the model actually has (Qwen2.5-7B, M = 4096 tokens = bs 4 x 1024): q|k|v, o, gate|up + SiLU*up, down
    try:
        pre = {}
        for name, (n, kq, silu) in {"qkv_3584_to_10752": (10752, 3584, False), "o_3584_to_3584": (3584, 3584, False),
                                    "gateup_silu_3584_to_37888": (37888, 3584, True), "down_18944_to_3584": (3584, 18944, False)}.items():
            q = make_problem(4096, n, kq, 64, device)
            if silu:
                f = lambda: agemm.matmul_silu_mul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"])    # noqa: E731
            else:
                f = lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"])              # noqa: E731
            t = min(time_events_steady(f, 30, 40.0) for _ in range(2))
            fl = gemm_flops(4096, n, kq + 64)
            pre[name] = {"us": round(t, 1), "TFLOPs": round(fl / t / 1e6, 1), "frac": round(fl / t / 1e6 / PEAK_F16_TFLOPS, 4)}
            # ... and with the epilogue operand the model gives it (Qwen2.5: bias on q|k|v and gate|up, the residual stream into o / down)
            gen = torch.Generator().manual_seed(n)
            if silu or n == 10752:
                bias = torch.randn(n, generator=gen).to(torch.bfloat16).to(device)
                if silu:
                    g = lambda: agemm.matmul_silu_mul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], bias=bias)    # noqa: E731
                else:
                    g = lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], bias=bias)              # noqa: E731
                pre[name]["epilogue_operand"] = "bias"
            else:
                res = torch.randn(4096, n, generator=gen).to(torch.bfloat16).to(device)
                g = lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], residual=res)               # noqa: E731
                pre[name]["epilogue_operand"] = "residual"
            pre[name]["us_as_in_model"] = round(min(time_events_steady(g, 30, 30.0) for _ in range(2)), 1)
            del q
            torch.cuda.empty_cache()
        tot_fl = sum(gemm_flops(4096, n, k + 64) for n, k in ((10752, 3584), (3584, 3584), (37888, 3584), (3584, 18944)))
        tot_us = sum(v["us"] for v in pre.values())
        tot_model = sum(v["us_as_in_model"] for v in pre.values())
        pre["layer_total"] = {"us": round(tot_us, 1), "TFLOPs": round(tot_fl / tot_us / 1e6, 1), "frac": round(tot_fl / tot_us / 1e6 / PEAK_F16_TFLOPS, 4),
                              "us_as_in_model": round(tot_model, 1), "frac_as_in_model": round(tot_fl / tot_model / 1e6 / PEAK_F16_TFLOPS, 4)}
        pre["note"] = ("M = 4096, KE = 64, sustained launches; frac = of the 2.5 PFLOP/s fp16 MFMA roof (the headline's roofline.frac on the model's shapes); "
                       "us_as_in_model = the same launch with the bias or residual the model's layer fuses into it")
        extra["prefill_gemms"] = pre
    except Exception as e:
        extra["prefill_gemms"] = {"error": f"{type(e).__name__}: {e}"}
    # ---- BASELINE config[2]: the seven linears of one Llama-3-8B layer at bs=1, seqlen=1 (sum of the graph-timed launches above)
    try:
        c3 = (2 * extra["decode_gemm_M1_N4096_KQ4096"]["us_per_launch_graph"] + 2 * extra["decode_gemm_M1_N1024_KQ4096"]["us_per_launch_graph"]
              + 2 * extra["decode_gemm_M1_N14336_KQ4096"]["us_per_launch_graph"] + extra["decode_gemm_M1_N4096_KQ14336"]["us_per_launch_graph"])
        c3_16 = (2 * extra["decode_gemm_M1_N4096_KQ4096"]["fp16_rocblas_us"] + 2 * extra["decode_gemm_M1_N1024_KQ4096"]["fp16_rocblas_us"]
                 + 2 * extra["decode_gemm_M1_N14336_KQ4096"]["fp16_rocblas_us"] + extra["decode_gemm_M1_N4096_KQ14336"]["fp16_rocblas_us"])
        wbytes = (2 * 4096 + 2 * 1024 + 2 * 14336) * 4160 * 9 / 16 + 4096 * 14400 * 9 / 16
        extra["llama3_8b_layer_linears_decode"] = {"us": round(c3, 2), "GBps": round(wbytes / c3 / 1e3, 1), "fp16_rocblas_us": round(c3_16, 2),
                                                  "speedup_vs_fp16_rocblas": round(c3_16 / c3, 2),
                                                  "note": "q,o 4096x4096; k,v 1024x4096; gate,up 14336x4096; down 4096x14336; M=1, KE=64"}
    except KeyError:
        pass
    # ---- BASELINE config[4]: the four sharded linears of one Llama-3-70B layer on ONE of 8 ranks (bs=4 decode); the two all-reduces
    #      (4 x 8192 fp32 partials = 128 KB each) and the hand-off (tp.handoff_*) are the driver's multi-GPU run to measure
    try:
        keys = ["decode_gemm_M4_N1280_KQ8192", "decode_gemm_M4_N7168_KQ8192", "decode_gemm_M4_N8192_KQ1024", "decode_gemm_M4_N8192_KQ3584"]
        c4 = sum(extra[k]["us_per_launch_graph"] for k in keys)
        c4_16 = sum(extra[k]["fp16_rocblas_us"] for k in keys)
        wb4 = (1280 + 7168) * 8256 * 9 / 16 + 8192 * (1088 + 3648) * 9 / 16
        extra["llama3_70b_tp8_rank_linears_decode"] = {"us": round(c4, 2), "GBps": round(wb4 / c4 / 1e3, 1), "fp16_rocblas_us": round(c4_16, 2),
                                                      "speedup_vs_fp16_rocblas": round(c4_16 / c4, 2),
                                                      "note": "per rank of TP=8, M=4, KE=64: q|k|v 1280x8192 and gate|up 7168x8192 column shards, "
                                                              "o 8192x1088 and down 8192x3648 row shards (K slices of the augmented axis); "
                                                              "collectives not included (single GPU)"}
    except KeyError:
        pass
    # ---- decode-batch / short-prefill token counts (split-K tiles) and the decode-step quantisers, graph-timed
    for (m, n, kq) in [(32, 4096, 4096), (128, 4096, 4096), (64, 3584, 18944)]:
        q = make_problem(m, n, kq, KE, device)
        o = torch.empty((m, n), dtype=torch.bfloat16, device=device)
        t = graph_time([lambda: agemm.matmul(q["qx"], q["qw"], q["sfx"], q["sfw"], q["alpha"], out=o)] * 4)
        extra[f"midM_gemm_M{m}_N{n}_KQ{kq}"] = {"us_per_call_graph": round(t, 2), "TFLOPs": round(gemm_flops(m, n, kq + KE) / t / 1e6, 1),
                                               "note": "split-K tile GEMM + finish pass, weights cache-resident"}
        del q
    xq = outlier_activations(4, 3584, device)
    gu = (torch.randn(4, 2 * 18944, device=device) * 2).to(torch.bfloat16)
    idx_h = torch.arange(3584, dtype=torch.int16, device=device)
    idx_i = torch.arange(18944, dtype=torch.int16, device=device)
    wn = torch.ones(3584, dtype=torch.bfloat16, device=device)
    gu_slots = torch.full((2 * 18944 // 16,), 0x4000, dtype=torch.int32, device=device)     # any valid abs-max words: timing only
    extra["decode_quantisers_us_graph"] = {
        "rmsnorm_quantize_x_M4_KQ3584": round(graph_time([lambda: agemm.rmsnorm_quantize_x(xq, wn, 1e-6, idx_h, 64)] * 8), 2),
        "reorder_quantize_x_dynamic_M4_KQ3584": round(graph_time([lambda: agemm.reorder_quantize_x_dynamic(xq, idx_h, 64)] * 8), 2),
        "silu_mul_quantize_x_dynamic_M4_KQ18944": round(graph_time([lambda: agemm.silu_mul_quantize_x_dynamic(gu, idx_i, 64)] * 8), 2),
        "silu_mul_quantize_x_dynamic_absmax_slots_M4_KQ18944": round(graph_time(
            [lambda: agemm.silu_mul_quantize_x_dynamic(gu, idx_i, 64, layout=agemm.GU_PAIRS, absmax_slots=gu_slots)] * 8), 2),
        "note": "per call, HIP-graph replay; the SiLU*up variant is two launches, the others one (absmax_slots: the abs-max words "
                "come from the repacked gate|up GEMM's epilogue, matmul_repacked_silu_absmax)"}
    del xq, gu
    # ---- fused decode linears (quantiser as the GEMM prologue) against the two launches they replace, graph-timed
    try:
        fused = {}
        for (m, n, kq) in [(4, 3584, 3584), (4, 10752, 3584), (4, 37888, 3584)]:
            q = make_problem(m, n, kq, KE, device)
            rot = max(2, int(320e6 // (n * (kq + KE) * 9 / 16)) + 1)        # weight copies: > 320 MB in all, nothing cache-resident
            rps = [agemm.repack_w(q["qw"].clone(), q["sfw"].clone()) for _ in range(rot)]
            x, sw = q["x"], float(q["sw"])
            wn1 = torch.ones(kq, dtype=torch.bfloat16, device=device)
            o = torch.empty((m, n), dtype=torch.bfloat16, device=device)

            def pair_rms(i):
                a_, sfa_ = agemm.rmsnorm_quantize_x(x, wn1, 1e-6, q["idx"], KE)
                agemm.matmul_repacked(a_, rps[i][0], sfa_, rps[i][1], sw, n, out=o)

            def pair_dyn(i):
                qa_, sfa_, sa_ = agemm.reorder_quantize_x_dynamic(x, q["idx"], KE)
                agemm.matmul_repacked(qa_, rps[i][0], sfa_, rps[i][1], sa_, n, scale_host=sw, out=o)

            fused[f"M{m}_N{n}_KQ{kq}"] = {
                "rmsnorm_fused_us": round(graph_time([(lambda i=i: agemm.rmsnorm_matmul_repacked(x, wn1, 1e-6, q["idx"], KE, rps[i][0], rps[i][1], sw, n, out=o))
                                                      for i in range(rot)]), 2),
                "rmsnorm_two_launches_us": round(graph_time([(lambda i=i: pair_rms(i)) for i in range(rot)]), 2),
                "dynamic_fused_us": round(graph_time([(lambda i=i: agemm.dynamic_matmul_repacked(x, q["idx"], KE, rps[i][0], rps[i][1], sw, n, out=o))
                                                      for i in range(rot)]), 2),
                "dynamic_two_launches_us": round(graph_time([(lambda i=i: pair_dyn(i)) for i in range(rot)]), 2)}
            del q, rps
        fused["note"] = ("per linear (the two-launch figure is the PAIR quantiser + GEMM), HIP-graph replay over weight copies totalling > 320 MB; in "
                         "the 28-layer decode graph fusing q|k|v, o and gate|up is worth 1500 -> 1714 tok/s with biases on (tools/e2e_fuse_ab.py)")
        extra["fused_decode_linears"] = fused
    except Exception as e:
        extra["fused_decode_linears"] = {"error": f"{type(e).__name__}: {e}"}
    torch.cuda.empty_cache()
    # ---- BASELINE config[3]: Qwen2.5-7B-shape, bs=4, prefill 1024 + 128 decode steps, biases on as benchmark_e2e_arc.py:27-36.
    #      HEADLINE = the reference's own protocol (benchmark_e2e_arc.py:81-166: prefill, 128 decode steps over a GROWING cache,
    #      both; 2 warm-up + 4 timed calls per repeat, mean +- 1.96 sigma), attention over the whole bf16 KV cache.
    try:
        from arcquant_amd.e2e import bench_decode, bench_protocol
        proto = {}
        for graph in (True, False):
            proto["hip_graph" if graph else "eager"] = bench_protocol("qwen2.5-7b", batch=4, prefill=1024, decode_steps=128, device=device,
                                                                       repeats=3, fused=True, attention="cache", graph=graph)
            torch.cuda.empty_cache()
        proto["headline_decode_tok_per_s"] = proto["hip_graph"]["decode_tok_per_s"]
        extra["qwen2.5-7b_e2e_reference_protocol"] = proto
        # secondary: one decode step at a fixed 1040-token window.  "current_token_attention" mirrors a quirk of the reference
        # harness (modeling_arc.py:169-198 attends over the tokens of the current call only: no KV read) and is NOT the headline.
        extra["qwen2.5-7b_decode_step_full_cache"] = bench_decode("qwen2.5-7b", batch=4, prefill=1024, steps=16, device=device, fused=True, attention="cache")
        torch.cuda.empty_cache()
        os.environ["ARCQ_E2E_DECODE_ATTENTION"] = "sdpa"     # the same step with torch's SDPA as the decode attention (harness glue A-B)
        extra["qwen2.5-7b_decode_step_full_cache_torch_sdpa_attention"] = bench_decode("qwen2.5-7b", batch=4, prefill=1024, steps=16, device=device,
                                                                                         fused=True, attention="cache")
        del os.environ["ARCQ_E2E_DECODE_ATTENTION"]
        torch.cuda.empty_cache()
        extra["qwen2.5-7b_decode_step_current_token_attention_harness_quirk"] = bench_decode("qwen2.5-7b", batch=4, prefill=1024, steps=16, device=device,
                                                                                               fused=True, attention="current")
        torch.cuda.empty_cache()
        extra["qwen2.5-7b_decode_step_reference_call_structure"] = bench_decode("qwen2.5-7b", batch=4, prefill=1024, steps=16, device=device, fused=False,
                                                                                  attention="cache")
    except Exception as e:  # the e2e harness is optional for the headline number
        extra["qwen2.5-7b_e2e_reference_protocol"] = {"error": f"{type(e).__name__}: {e}"}
    return extra


def cpu_baseline():
    """The reference's CPU fake-quant path (our port, oracle/fake_quant.py) on the SAME workload as the GPU
    step: fake ARC linear (quantise x, quantise w, F.linear) at M=4096, N=KQ=4096, KE=64 in bf16 on all host
    cores, plus BASELINE config[0] (fake NVFP4 of one 4096x4096 fp16 weight).  Bounded: 2 + 2 repeats (~30 s of CPU work)."""
    from oracle import fake_quant as FQ
    cores = os.cpu_count() or 1
    torch.set_num_threads(cores)
    M_s, N, KQ, KE = 4096, 4096, 4096, 64
    x = outlier_activations(M_s, KQ, "cpu")
    g = torch.Generator().manual_seed(1)
    w = (torch.rand(N, KQ, generator=g) * 3).to(torch.bfloat16)
    w16 = w.to(torch.float16)
    idx = torch.arange(KQ)
    t_lin, t_w = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        FQ.fake_arc_linear(x, w, idx, KE)
        t_lin.append(time.perf_counter() - t0)
    for _ in range(2):
        t0 = time.perf_counter()
        FQ.fake_nvfp4(w16)
        t_w.append(time.perf_counter() - t0)
    best = min(t_lin)
    flops = gemm_flops(M_s, N, KQ + KE)
    return {"value": round(flops / best / 1e12, 5), "unit": "TFLOP/s", "cores": cores, "kind": "port",
            "sample": f"full workload: fake_arc_linear (quantise x + w, F.linear) M=4096 N=KQ=4096 KE=64 bf16, best of 2 = {best:.3f} s "
                      f"(mean {sum(t_lin) / len(t_lin):.3f} s); fake NVFP4 of one 4096x4096 fp16 weight (config[0]): best of 2 = "
                      f"{min(t_w):.3f} s; torch {torch.__version__} CPU, {cores} threads"}


def strong_scaling(S, rank, world, device, dist, iters=20, two_shot=True):
    """ONE S x S x (S + 64) ARC-GEMM split over `world` ranks, both tensor-parallel ways, with the exchange arcquant_amd/tp.py performs:
      column-parallel: rank r owns output columns [r N/p, (r+1) N/p) (128-row scale tiles stay whole), full activation;
                       all-gather of the bf16 [M, N/p] blocks (what a q/k/v/gate/up layer pays when its output is needed whole);
      row-parallel:    rank r owns a 64-aligned slice of the augmented K axis of BOTH operands; bf16 partial [M, N] ->
                       tp.all_reduce_sum (two-shot: reduce-scatter + all-gather over RCCL; one all-reduce on the gloo rehearsal).
    Times are the max over ranks (HIP events around GEMM + collective on the current stream)."""
    from arcquant_amd import agemm, tp
    M = N = KQ = S
    KE = 64
    p = make_problem(M, N, KQ, KE, device, seed=45510)           # the same problem on every rank
    flops = gemm_flops(M, N, KQ + KE)
    out = {}
    # column-parallel
    cp = tp.ColumnParallelARCLinear(p["qw"], p["sfw"], p["sw"], rank, world)
    widths = [b - a for a, b in cp.ranges]
    wmax = max(widths)
    y = torch.zeros((M, wmax), dtype=torch.bfloat16, device=device)
    gathered = torch.empty((world * M, wmax), dtype=torch.bfloat16, device=device)

    def col_step():
        agemm.matmul(p["qx"], cp.W, p["sfx"], cp.SFW, p["alpha"], out=y[:, :widths[rank]] if widths[rank] == wmax else None)
        dist.all_gather_into_tensor(gathered, y)

    def col_gemm_only():
        agemm.matmul(p["qx"], cp.W, p["sfx"], cp.SFW, p["alpha"])

    # row-parallel
    rp = tp.RowParallelARCLinear(p["qw"], p["sfw"], p["sw"], rank, world)
    a_sh, sfa_sh = rp.shard_activation(p["qx"], p["sfx"])
    part = torch.empty((M, N), dtype=torch.bfloat16, device=device)

    def row_step():
        agemm.matmul(a_sh, rp.W, sfa_sh, rp.SFW, p["alpha"], out=part)
        tp.all_reduce_sum(part, two_shot=two_shot)

    def row_gemm_only():
        agemm.matmul(a_sh, rp.W, sfa_sh, rp.SFW, p["alpha"], out=part)

    # FIXED launch counts, identical on every rank: two of the four steps hold collectives, and time_events_steady's warm-up and
    # timed counts depend on the rank's own measured time -- ranks would issue different numbers of collectives and hang
    for name, fn in (("column_parallel_allgather", col_step), ("column_parallel_gemm_only", col_gemm_only),
                     ("row_parallel_bf16_two_shot_allreduce" if two_shot else "row_parallel_bf16_allreduce", row_step),
                     ("row_parallel_gemm_only", row_gemm_only)):
        dist.barrier()
        us = time_events(fn, 5 * iters, 300)                   # >= 300 launches first: past the clock ramp after idle
        t = torch.tensor([us], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        out[name] = {"us": round(float(t.item()), 1), "TFLOPs_total": round(flops / float(t.item()) / 1e6, 1),
                     "frac_of_fp4_peak_total": round(flops / float(t.item()) / 1e6 / (world * PEAK_FP4_TFLOPS), 4)}
    rows = M // world
    out["bytes_exchanged_per_rank"] = {"column_parallel": int((world - 1) * M * wmax * 2), "row_parallel": int(2 * (world - 1) * rows * N * 2)}
    return out


def _extras_child(conn, backend, one_device):
    """Runs in a process of its own, started by its rank BEFORE that rank touched the GPU: waits for the rendezvous port, then times
    the strong-scaling splits over a process group of its own and sends the result back.  A hang or an RCCL abort in here costs
    the rank's JSON line nothing: the parent waits with a timeout and reports the failure as a string."""
    try:
        msg = conn.recv()
        if not msg:
            return
        os.environ["MASTER_PORT"] = str(msg["port"])
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import torch.distributed as dist
        rank, world, local_rank = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
        dev_index = 0 if one_device else local_rank
        torch.cuda.set_device(dev_index)
        device = torch.device("cuda", dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        out = {}
        for S in msg["sizes"]:
            try:
                out[f"gemm_{S}"] = strong_scaling(S, rank, world, device, dist, two_shot=(backend == "nccl"))
            except Exception as e:                               # symmetric failures (shapes, memory) keep the other size alive
                out[f"gemm_{S}"] = {"error": repr(e)[:200]}
        conn.send(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        try:
            conn.send({"error": repr(e)[:300]})
        except Exception:
            pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    # default warm-up: ~55 ms of continuous load, past the power-management transient after idle (time_events_steady above;
    # profiles/r01f_clock_transient.txt).  Timed steps inside that ramp read 1200-1260 instead of ~1350 TFLOP/s, so a caller's
    # small --warmup is preceded by --prewarm-ms of the same untimed load.
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--prewarm-ms", type=float, default=60.0,
                    help="continuous load (the same step) before the W warm-up steps, so that a small --warmup also measures sustained clocks")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default, the contract's mode): every rank its own 4096 output columns, no data-path collective; strong: ONE "
                         "4096^2 ARC-GEMM split over the ranks (column-parallel shards + RCCL all-gather of the bf16 output) as the timed step")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the secondary measurements: the CPU baseline and `extra` (one GPU), the "
                         "strong-scaling splits (--gpus N > 1).  Off by default: a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float32, a fixed sample of rows)")
    ap.add_argument("--no-strong-extra", action="store_true",
                    help="with --full and --gpus N > 1: do NOT time the strong-scaling splits (ONE 4096^2 and ONE 8192^2 ARC-GEMM over the "
                         "ranks, both tensor-parallel ways with their exchange; extra.strong_scaling).  They run in a helper process per rank, "
                         "so a failing collective costs the JSON line nothing")
    ap.add_argument("--strong-extra", action="store_true", help=argparse.SUPPRESS)      # round-2 spelling: now part of --full
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the secondary GPU measurements")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    from arcquant_amd import launch
    if args.gpus > 1 and not launch.launched():
        # `python bench.py --gpus N` as the driver runs it: start the N ranks ourselves.  This parent makes no GPU call.
        sys.exit(launch.launch_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    # The contract is ONE JSON line on standard output.  Libraries print there too (gloo: "[Gloo] Rank 0 is connected to ..."), from C,
    # past sys.stdout: keep the real descriptor aside, point fd 1 at stderr for the whole run, and write the line to the kept one.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    # Rehearsal switches (not used by the driver): ARCQ_BENCH_ONE_DEVICE=1 maps every rank to cuda:0 and
    # ARCQ_BENCH_BACKEND=gloo replaces RCCL, so the N > 1 code path can be exercised on a one-GPU box.
    one_device = os.environ.get("ARCQ_BENCH_ONE_DEVICE") == "1"
    backend = os.environ.get("ARCQ_BENCH_BACKEND", "nccl")
    dev_index = 0 if one_device else local_rank
    # the strong-scaling extras run in a helper process of this rank, started NOW -- before this process touches the GPU (an exec
    # from a GPU-initialised process is refused on the pool) -- and idle until the headline has been measured
    helper = helper_conn = None
    if world > 1 and args.full and not args.no_extra and not args.no_strong_extra:
        import multiprocessing as mp
        ctx = mp.get_context("spawn")
        helper_conn, child_conn = ctx.Pipe()
        helper = ctx.Process(target=_extras_child, args=(child_conn, backend, one_device), daemon=True)
        helper.start()
        child_conn.close()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    from arcquant_amd import agemm

    # ---- headline workload: this rank's column shard of the M=4096 ARC-GEMM
    M, N, KQ, KE = 4096, 4096, 4096, 64
    K = KQ + KE
    p = make_problem(M, N, KQ, KE, device, seed=45510 + rank)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=device)

    def step():
        agemm.matmul(p["qx"], p["qw"], p["sfx"], p["sfw"], p["alpha"], out=out)

    strong = args.scaling == "strong" and world > 1
    if strong:                                               # ONE 4096^2 GEMM over the ranks: column shard + all-gather
        from arcquant_amd import tp
        p = make_problem(M, N, KQ, KE, device, seed=45510)     # the same problem on every rank
        cp = tp.ColumnParallelARCLinear(p["qw"], p["sfw"], p["sw"], rank, world)
        widths = [b - a for a, b in cp.ranges]
        y_sh = torch.zeros((M, max(widths)), dtype=torch.bfloat16, device=device)
        gathered = torch.empty((world * M, max(widths)), dtype=torch.bfloat16, device=device)

        def step():  # noqa: F811
            agemm.matmul(p["qx"], cp.W, p["sfx"], cp.SFW, p["alpha"], out=y_sh if widths[rank] == max(widths) else None)
            dist.all_gather_into_tensor(gathered, y_sh)

    if args.prewarm_ms > 0:                       # untimed: bring the clocks to their sustained state (see time_events_steady)
        if strong:                                # the step holds a collective: the SAME launch count on every rank (an adaptive count hangs)
            for _ in range(300):
                step()
            torch.cuda.synchronize()
        else:
            time_events_steady(step, 5, args.prewarm_ms)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kern_us = e0.elapsed_time(e1) * 1e3 / args.steps
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:                         # what the last timed step left: `out` (weak, one file per rank) or the gathered output (strong)
        if strong:
            if rank == 0:
                dump_output(args.dump_outputs, "out", gathered, 1024)
        else:
            dump_output(args.dump_outputs, "out" if world == 1 else f"out_rank{rank}", out, 1024 // world)

    flops = gemm_flops(M, N, K)
    # HBM traffic per launch from the committed PMC passes (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE);
    # bench.py cannot run rocprofv3 on itself, so the number is read from profiles/ and labelled as such
    traffic, traffic_file = None, None
    for name in ("r03_pmc_tile_gemm.json", "r02_pmc_tile_gemm.json"):      # the newest committed PMC pass of the shipped kernel
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                traffic = json.load(f)["per_launch"]["hbm_traffic_bytes"]
            traffic_file = name
            break
        except Exception:
            continue
    value = (1 if strong else world) * flops * args.steps / elapsed / 1e12
    if strong:            # the step's event bracket also holds the all-gather: time this rank's GEMM launch alone for `roofline`
        kern_us = time_events(lambda: agemm.matmul(p["qx"], cp.W, p["sfx"], cp.SFW, p["alpha"]), max(20, args.steps), 5)
    achieved = (flops / world if strong else flops) / kern_us / 1e6   # TFLOP/s of this rank's launch of the dominant kernel, HIP-event timed

    result = {
        "metric": "ARC-NVFP4 GEMM TFLOP/s (M=4096, N=KQ=4096, KE=64)",
        "value": round(value, 2), "unit": "TFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "prewarm_ms": args.prewarm_ms,
        "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True, "scaling": "strong" if strong else "weak",
        "vs_baseline": None, "dtype": "f16", "data": "synthetic",
        "config": {"workload": "agemm.matmul on pre-quantised NVFP4 operands: M=4096 tokens x N=4096 (per rank) x K_aug=4160 "
                               "(KQ=4096 + 64 residual channels), activations per kernels/main.py outlier recipe, weights rand*3, "
                               "exact e2m1 x ue4m3 products on fp16 MFMA with fp32 accumulate, bf16 out",
                   "M": M, "N_per_rank": N // world if strong else N, "KQ": KQ, "KE": KE,
                   "parallelism": (f"one 4096^2 GEMM column-parallel x{world} + RCCL all-gather of the bf16 output" if strong
                                   else f"column-parallel x{world} (no collective)")},
        "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(achieved / PEAK_F16_TFLOPS, 4), "traffic": traffic,
                     "traffic_source": f"profiles/{traffic_file} (rocprofv3 --pmc FETCH_SIZE x 2 [gfx950 correction] + WRITE_SIZE, bytes per launch, separate passes)",
                     "kernel": "arcq::gemm_tile_kernel", "kernel_us": round(kern_us, 2),
                     "frac_of_fp4_peak": round(achieved / PEAK_FP4_TFLOPS, 4),
                     "note": "NVFP4 (ue4m3 scale per 16) has no exact mapping onto gfx950's E8M0-per-32 scaled fp4 MFMA; the exact "
                             "contraction runs on fp16 MFMA, so `peak` is the dense fp16/bf16 rate; frac_of_fp4_peak is the "
                             "north-star denominator.  In-kernel clock stamps (s_memtime / s_memrealtime around the K loop, "
                             "profiles/r02_tile_gemm_in_kernel_clock.jsonl): the K loop runs at 2.07 GHz under sustained load, not the "
                             "2.4 GHz `peak` assumes, with the matrix pipe busy 72.6 % of it; the K loop is 88.7 of the ~103 us launch "
                             "(the rest: first loads + the 33.5 MB store burst at one tile per CU); "
                             "extra.gemm_4096.fp16_rocblas_TFLOPs is what the vendor fp16 GEMM sustains beside it in the same state"},
    }
    if rank == 0 and world == 1 and args.full:
        if not args.no_cpu:
            result["cpu_baseline"] = cpu_baseline()
        if not args.no_extra:
            result["extra"] = bench_extra(args, device, rank)
    elif helper is not None:
        # strong scaling of ONE fixed GEMM over the ranks, with the collective a real layer pays (reported beside, never part of a weak
        # `value`), in the helper processes: own process group on a fresh port, bounded wait.  A hang, an RCCL abort or a crash in
        # there becomes an "error" string; this rank's JSON line does not depend on it.
        strong_x = {}
        try:
            port = torch.tensor([launch.free_port() if rank == 0 else 0], dtype=torch.int64, device=device)
            dist.broadcast(port, src=0)
            helper_conn.send({"port": int(port.item()), "sizes": [4096, 8192]})
            if helper_conn.poll(float(os.environ.get("ARCQ_BENCH_EXTRA_TIMEOUT_S", "240"))):
                strong_x = helper_conn.recv()
            else:
                strong_x = {"error": "no answer from the strong-scaling helper within its time limit"}
        except Exception as e:
            strong_x = {"error": repr(e)[:200]}
        helper.join(timeout=20)
        if helper.is_alive():
            helper.kill()                                       # our own child, by handle
        if rank == 0:
            strong_x["note"] = ("ONE S x S x (S+64) ARC-GEMM split over the ranks: column-parallel + all-gather of the bf16 output; row-parallel "
                                "(64-aligned slices of the augmented K axis) + tp.all_reduce_sum of the bf16 partial (two-shot: reduce-scatter "
                                "+ all-gather); us = max over ranks, HIP events around GEMM + collective")
            result["extra"] = {"strong_scaling": strong_x}
    if rank == 0:
        os.write(json_fd, (json.dumps(result) + "\n").encode())
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
