#!/usr/bin/env python3
"""Decode attention over the int4 paged KV cache (arcquant_amd/kvcache.py) against the harness's bf16 kernel (include/arcq_harness.h) on
the same logical cache, and the one-launch quantising append against the torch quantiser + append_kv_i4, in one process on one device;
writes profiles/kv_int4_decode.json (the evidence behind DESIGN.md 11).

    python tools/kv_bench.py [--layers 28] [--heads 28] [--out profiles/kv_int4_decode.json]

Shapes: B = 4 and B = 1, `--heads` heads (kv heads == query heads, as the harness models them), 1040 and 4096 positions, P = 16.
Method (tools/mx_bench.py's graph_time): a record's launches -- one per layer over `--layers` separate layers' caches, so that the
bytes a launch reads were not left in a cache by the launch before (28 layers: 0.45 / 1.7 GB at 1040 positions, bs = 4) -- are replayed
from one HIP graph, warmed for ~40 ms and timed for >= 10 ms between two events; us is per launch.  Bytes are what the kernel must
read: int4 2 * B * H * T * (64 + 4), bf16 2 * B * H * T * 256.  The two kernels ALTERNATE for `--rounds` rounds; a record keeps the best
round of each and `round_spread`, the largest (max - min) / min either showed between rounds.
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

from arcquant_amd import _lib, kvcache  # noqa: E402
from mx_bench import graph_time  # noqa: E402

P = 16


def alternate(chains, rounds):
    seen = {n: [] for n in chains}
    for _ in range(rounds):
        for n, launches in chains.items():
            seen[n].append(graph_time(launches))
    return {n: min(t) for n, t in seen.items()}, round(max((max(t) - min(t)) / min(t) for t in seen.values()), 3)


def random_cache(B, H, T, layers, dev):
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, H)
    c.pages.copy_(torch.randint(0, 256, c.pages.shape, dtype=torch.uint8, device=dev))
    c.scales[..., 0] = 0.4
    c.scales[..., 1] = 3.0
    return c


def decode(B, H, T, layers, dev, rounds):
    lib = _lib.lib()
    c = random_cache(B, H, T, layers, dev)
    tables = c.tables(T)
    q = torch.randn(B, H, 128, device=dev).to(torch.bfloat16)
    o = torch.empty_like(q)
    qkv = torch.randn(B, 3 * H * 128, device=dev).to(torch.bfloat16)
    dense = [torch.randn(2, B, H, T, 128, device=dev).to(torch.bfloat16) for _ in range(layers)]
    out = torch.empty(B, H * 128, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(max(int(lib.arcq_harness_attn_workspace_bytes(B, H, T)) // 4, 1), dtype=torch.float32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream     # noqa: E731

    def bf16(layer):
        def f():
            _lib.check(lib.arcq_harness_attn_decode(qkv.data_ptr(), dense[layer][0].data_ptr(), dense[layer][1].data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                    B, H, T, T - 1, stream()), "harness attn_decode")
        return f
    chains = {"int4": [lambda layer=layer: kvcache.batch_decode_i4(o, q, **tables, layer_idx=layer) for layer in range(layers)],
              "bf16": [bf16(layer) for layer in range(layers)]}
    us, spread = alternate(chains, rounds)
    b_i4, b_bf = 2 * B * H * T * 68, 2 * B * H * T * 256
    return {"what": "decode attention", "B": B, "heads": H, "positions": T, "page_size": P, "layers_rotated": layers,
            "int4_us": round(us["int4"], 2), "int4_bytes": b_i4, "int4_GBps": round(b_i4 / us["int4"] / 1e3, 1),
            "bf16_us": round(us["bf16"], 2), "bf16_bytes": b_bf, "bf16_GBps": round(b_bf / us["bf16"] / 1e3, 1),
            "speedup_over_bf16": round(us["bf16"] / us["int4"], 3), "byte_ratio": round(b_bf / b_i4, 3), "round_spread": spread,
            "int4_slices_per_sequence": int(lib.arcq_kv_decode_workspace_bytes(B, H, H, tables["kv_indices"].numel(), P)) // (B * H * 130 * 4) or 1}


def append(B, H, T, layers, dev, rounds):
    c = random_cache(B, H, T, layers, dev)
    tables = c.tables(T)
    k, v = (torch.randn(B, H, 128, device=dev) * 3).to(torch.bfloat16), (torch.randn(B, H, 128, device=dev) * 3).to(torch.bfloat16)

    def reference_flow(layer):
        def f():
            kq, ks, kz = kvcache.asym_quantize_and_pack_i4(k)
            vq, vs, vz = kvcache.asym_quantize_and_pack_i4(v)
            kvcache.append_kv_i4(**tables, k=kq, v=vq, k_param=torch.cat([ks, kz], -1).to(torch.float16), v_param=torch.cat([vs, vz], -1).to(torch.float16),
                                 layer_idx=layer)
        return f
    chains = {"fused": [lambda layer=layer: kvcache.append_kv_quantize_i4(**tables, k=k, v=v, layer_idx=layer) for layer in range(layers)],
              "torch": [reference_flow(layer) for layer in range(layers)]}
    us, spread = alternate(chains, rounds)
    return {"what": "quantise + append one token per sequence", "B": B, "heads": H, "positions": T, "append_kv_quantize_i4_us": round(us["fused"], 2),
            "torch_quantiser_plus_append_kv_i4_us": round(us["torch"], 2), "speedup": round(us["torch"] / us["fused"], 2), "round_spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--heads", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_int4_decode.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    with torch.no_grad():
        for B in (4, 1):
            for T in (1040, 4096):
                records.append(decode(B, a.heads, T, a.layers, dev, a.rounds))
                print(json.dumps(records[-1]), flush=True)
                torch.cuda.empty_cache()
        records.append(append(4, a.heads, 1040, a.layers, dev, a.rounds))
        print(json.dumps(records[-1]), flush=True)
    res = {"tool": "tools/kv_bench.py", "device": torch.cuda.get_device_name(0), "records": records}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
