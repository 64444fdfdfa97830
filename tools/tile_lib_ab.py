#!/usr/bin/env python3
"""A-B of two builds of the library on the tile GEMM (tuning aid): steady-state time per launch (bench.py's sustained-clock protocol),
each build in its own subprocess, rounds interleaved; per shape and build the values of every round, their median and their
run-to-run band (max - min).  usage: tile_lib_ab.py [--rounds N] name=path[:ENV=VAL] ...     (the comparator first)
ENV ARCQ_AB_OVERLAP_TAIL=0|1|2 calls arcq_debug_set_tile_overlap_tail with that value first (a library that has the setter),
ARCQ_AB_PAIR_LOADS=0|1 arcq_debug_set_tile_pair_loads, ARCQ_AB_QUAD_LOADS=0|1 arcq_debug_set_tile_quad_loads."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# M, N, KQ, epilogue: "" plain, "silu" SiLU * up, "bias", "residual", "rw" plain over the repacked weight[, KE = 64]      (the model shapes:
# down, gate|up, q|k|v with its bias, o with its residual; KE = 0: an even number of K steps; M = 1024: the 128 x 256 tile)
SHAPES = [(4096, 4096, 4096, ""), (8192, 8192, 8192, ""), (4096, 4096, 4096, "", 0), (4096, 3584, 18944, ""), (4096, 37888, 3584, "silu"),
          (4096, 10752, 3584, "bias"), (4096, 3584, 3584, "residual"), (4096, 4096, 4096, "rw"), (1024, 4096, 4096, "")]

CODE = """
import json, os, sys, torch
sys.path.insert(0, {root!r})
import bench
from arcquant_amd import agemm
if os.environ.get('ARCQ_AB_OVERLAP_TAIL'):
    agemm._debug_set_tile_overlap_tail(int(os.environ['ARCQ_AB_OVERLAP_TAIL']))
if os.environ.get('ARCQ_AB_PAIR_LOADS'):
    agemm._debug_set_tile_pair_loads(int(os.environ['ARCQ_AB_PAIR_LOADS']))
if os.environ.get('ARCQ_AB_QUAD_LOADS'):
    agemm._debug_set_tile_quad_loads(int(os.environ['ARCQ_AB_QUAD_LOADS']))
dev = torch.device('cuda:0')
out = []
for (M, N, KQ, epi, *ke) in {shapes!r}:
    p = bench.make_problem(M, N, KQ, ke[0] if ke else 64, dev)
    g = torch.Generator().manual_seed(N)
    bias = torch.randn(N, generator=g).to(torch.bfloat16).to(dev) if epi == 'bias' else None
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev) if epi == 'residual' else None
    if epi == 'silu':
        f = lambda: agemm.matmul_silu_mul(p['qx'], p['qw'], p['sfx'], p['sfw'], p['alpha'])
    elif epi == 'rw':
        rw, rsf = agemm.repack_w(p['qw'], p['sfw'])
        o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        f = lambda: agemm.matmul_rw(p['qx'], rw, p['sfx'], rsf, p['alpha'], N, out=o)
    else:
        o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        f = lambda: agemm.matmul(p['qx'], p['qw'], p['sfx'], p['sfw'], p['alpha'], bias=bias, residual=res, out=o)
    us = bench.time_events_steady(f, 100, warm_ms=60.0)
    out.append({{"shape": [M, N, KQ], "KE": ke[0] if ke else 64, "epilogue": epi, "us": round(us, 2)}})
    del p
    torch.cuda.empty_cache()
print("RESULT " + json.dumps(out))
"""


def run(spec):
    path, *envs = spec.split(":")
    env = dict(os.environ, ARCQ_HIP_LIB=os.path.join(ROOT, path))
    for e in envs:
        k, v = e.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, "-c", CODE.format(root=ROOT, shapes=SHAPES)], env=env, capture_output=True, text=True, cwd=ROOT)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(r.stderr[-800:])


if __name__ == "__main__":
    args = sys.argv[1:]
    rounds = 3
    if args and args[0] == "--rounds":
        rounds, args = int(args[1]), args[2:]
    specs = dict(a.split("=", 1) for a in args)
    acc = {n: [] for n in specs}
    for rnd in range(rounds):
        for n, s in specs.items():
            acc[n].append(run(s))
            print(f"round {rnd + 1} of {rounds}: {n} done", file=sys.stderr, flush=True)      # (rows come at the end: a sign of life)
    for i, shp in enumerate(SHAPES):
        row = {"shape": list(shp[:3]), "KE": shp[4] if len(shp) > 4 else 64, "epilogue": shp[3] or "plain"}
        for n in specs:
            us = [r[i]["us"] for r in acc[n]]
            row[n] = {"us": us, "median": round(statistics.median(us), 2), "band": round(max(us) - min(us), 2)}
        print(json.dumps(row), flush=True)
