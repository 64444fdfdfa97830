"""A-B of the one-copy weight path: agemm.matmul on the reference-layout weight against agemm.matmul_rw on the repacked weight (and the
silu-mul epilogue: matmul_silu_mul against matmul_rw_silu_mul), same operands, same process, interleaved rounds on one GPU.

    python tools/rw_ab.py [out.jsonl]
    python tools/rw_ab.py --e2e [out.jsonl]     # the Qwen2.5-7B harness with and without repacked_only (arcquant_amd/e2e.py)

Per shape: `warm` = the best of ROUNDS interleaved time_events_steady (bench.py) measurements of each side (operands L2/MALL-resident
where they fit); `cold` (M <= 512 only) = graph replay over enough weight copies (> 320 MB) that every launch streams its weight from
HBM, the copies of both sides interleaved round by round.  The route column is agemm.rw_route: 1 = the repacked decode kernels (the
rw side is then matmul_repacked's kernel), 2 = register-tiled, 3 = LDS-tiled over RW; `gprime` marks the decode shapes matmul serves
with an LDS-transposing kernel."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from arcquant_amd import agemm  # noqa: E402

ROUNDS = 3
KE = 64


def _problem(M, N, KQ, dev):
    p = bench.make_problem(M, N, KQ, KE, dev)
    p["rw"], p["rsf"] = agemm.repack_w(p["qw"], p["sfw"])
    g = torch.Generator(device=dev).manual_seed(N)
    p["bias"] = (torch.randn(N, generator=g, device=dev) * 0.02).to(torch.bfloat16)
    p["res"] = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16)
    return p


def _calls(p, N, epi, qw, sfw, rw, rsf, out):
    kw = {}
    if "bias" in epi:
        kw["bias"] = p["bias"]
    if "res" in epi:
        kw["residual"] = p["res"]
    if epi == "silu_bias":
        return (lambda: agemm.matmul_silu_mul(p["qx"], qw, p["sfx"], sfw, p["alpha"], bias=p["bias"]),
                lambda: agemm.matmul_rw_silu_mul(p["qx"], rw, p["sfx"], rsf, p["alpha"], N, bias=p["bias"]))
    return (lambda: agemm.matmul(p["qx"], qw, p["sfx"], sfw, p["alpha"], out=out, **kw),
            lambda: agemm.matmul_rw(p["qx"], rw, p["sfx"], rsf, p["alpha"], N, out=out, **kw))


def _graph_us(fn_list):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for f in fn_list:
            f()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for f in fn_list:
                f()
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(fn_list))


def measure(M, N, KQ, epi, group, dev):
    K = KQ + KE
    p = _problem(M, N, KQ, dev)
    out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    ref, rw = _calls(p, N, epi, p["qw"], p["sfw"], p["rw"], p["rsf"], out)
    warm = {"matmul": [], "matmul_rw": []}
    for _ in range(ROUNDS):
        warm["matmul"].append(bench.time_events_steady(ref, 50))
        warm["matmul_rw"].append(bench.time_events_steady(rw, 50))
    rec = {"group": group, "M": M, "N": N, "K": K, "epilogue": epi, "route": agemm.rw_route(M, N, K),
           "gprime": agemm.rw_route(M, N, K) == 2 and M <= 8 and (N > 16384 or K > 8448),
           "warm_us_matmul": round(min(warm["matmul"]), 3), "warm_us_matmul_rw": round(min(warm["matmul_rw"]), 3)}
    rec["warm_ratio"] = round(rec["warm_us_matmul_rw"] / rec["warm_us_matmul"], 4)
    if M <= 512:
        rot = max(2, int(320e6 // (N * K * 9 / 16)) + 1)
        copies = [(p["qw"].clone(), p["sfw"].clone(), p["rw"].clone(), p["rsf"].clone()) for _ in range(rot)]
        fr = [_calls(p, N, epi, c[0], c[1], c[2], c[3], out)[0] for c in copies]
        fw = [_calls(p, N, epi, c[0], c[1], c[2], c[3], out)[1] for c in copies]
        cold = {"matmul": [], "matmul_rw": []}
        for _ in range(ROUNDS):
            cold["matmul"].append(_graph_us(fr))
            cold["matmul_rw"].append(_graph_us(fw))
        rec.update(cold_us_matmul=round(min(cold["matmul"]), 3), cold_us_matmul_rw=round(min(cold["matmul_rw"]), 3), cold_copies=rot)
        rec["cold_ratio"] = round(rec["cold_us_matmul_rw"] / rec["cold_us_matmul"], 4)
        del copies, fr, fw
    del p, out
    torch.cuda.empty_cache()
    return rec


def shapes():
    h, it = 3584, 18944
    qwen = [(3 * h, h, "bias"), (h, h, "bias_res"), (2 * it, h, "silu_bias"), (h, it, "bias_res")]
    out = [(4096, N, KQ, epi, "lds_tiled: Qwen2.5-7B prefill") for N, KQ, epi in qwen]
    out.append((4096, 4096, 4096, "plain", "lds_tiled: 4096^2 headline"))
    out += [(M, 4096, 4096, "plain", "reg_tiled: N = K = 4096 M sweep") for M in (17, 32, 64, 128, 256, 512)]
    out += [(M, N, KQ, "plain" if epi == "silu_bias" else epi, "reg_tiled: harness shapes bs %d" % M) for M in (32, 64) for N, KQ, epi in qwen]
    out += [(M, h, it, "plain", "gprime") for M in (5, 8)] + [(1, 2 * it, h, "plain", "gprime")]
    return out


def e2e_ab(fh, name="qwen2.5-7b"):
    """Resident weight memory of the built fused model and bench_decode (graph replay, full cache) in both modes, bs 4 and 8,
    interleaved: two-copy, one-copy, two-copy, one-copy."""
    import dataclasses
    from arcquant_amd import e2e
    dev = torch.device("cuda:0")
    for ro in (False, True):
        torch.cuda.empty_cache()
        m0 = torch.cuda.memory_allocated(dev)
        with torch.no_grad():
            model = e2e.DecoderModel(dataclasses.replace(e2e.MODEL_CFGS[name]), 4, 1024 + 17, dev, fused=True, attention="cache", repacked_only=ro)
        rec = {"what": "resident", "model": name, "repacked_only": ro, "memory_allocated_after_build": torch.cuda.memory_allocated(dev) - m0,
               "weight_bytes": model.weight_bytes()}
        del model
        torch.cuda.empty_cache()
        _emit(fh, rec)
    for batch in (4, 8):
        for rnd in range(2):
            for ro in (False, True):
                r = e2e.bench_decode(name, batch=batch, fused=True, attention="cache", repacked_only=ro)
                r.update(what="bench_decode", round=rnd, repacked_only=ro)
                _emit(fh, r)
                torch.cuda.empty_cache()


def _emit(fh, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def main():
    if "--e2e" in sys.argv:
        args = [a for a in sys.argv[1:] if a != "--e2e"]
        fh = open(args[0], "w") if args else None
        e2e_ab(fh)
        return
    dest = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    fh = open(dest, "w") if dest else None
    with torch.no_grad():
        for M, N, KQ, epi, group in shapes():
            _emit(fh, measure(M, N, KQ, epi, group, dev))


if __name__ == "__main__":
    main()
