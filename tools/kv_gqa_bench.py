#!/usr/bin/env python3
"""Decode attention of GQA models over the int4 paged KV cache: kvcache.batch_decode_gqa_i4 (the g query heads of a kv head in one pass on
MFMA, kv_decode_gqa.hip) against kvcache.batch_decode_i4 (the VALU kernel, ceil(g / 4) passes) on the same pages and queries, in one
process on one device; writes profiles/kv_int4_decode_gqa.json (the evidence behind DESIGN.md 11 "GQA decode on MFMA").

    python tools/kv_gqa_bench.py [--rounds 3] [--out profiles/kv_int4_decode_gqa.json]
    python tools/kv_gqa_bench.py --table f16 [--rounds 3] [--out profiles/kv_f16_decode_gqa.json]
    python tools/kv_gqa_bench.py --table fp8 [--rounds 3] [--out profiles/kv_fp8_decode_gqa.json]

Shapes: (Nq, N) = (28, 4), (32, 8), (64, 8) -- Qwen2.5-7B, Llama-3-8B, Llama-3-70B -- at batch sizes 1, 4, 16 and 1040, 4096, 16384
positions, bf16, P = 16.  Method (tools/kv_bench.py's): a record's launches -- one per layer over separate layers' caches, enough layers
that a round reads >= 600 MB (more than L2 and MALL hold; at most 512 layers, `cold` says whether that was reached) -- are replayed from
one HIP graph, warmed for ~40 ms and timed for >= 10 ms between two events; us is per launch.  Bytes are the pages read once:
2 * B * N * T * (64 + 4).  The two kernels ALTERNATE for `--rounds` rounds; a record keeps the best round of each and `round_spread`.
Before a shape is timed the two results are compared (max |difference| is recorded).

``--table f16`` (DESIGN.md 11 "GQA decode over a 16-bit cache"): kvcache.batch_decode_gqa_f16 (kv_decode_gqa16.hip) against
kvcache.batch_decode_f16 on the same bf16 pages (randn * 3 rows; bytes 2 * B * N * T * 256), and against batch_decode_gqa_i4 over int4
pages that hold the quantised values of the same rows (bytes as above), the three alternating in the same rounds.

``--table fp8`` (DESIGN.md 11 "FP8 cache"): kvcache.batch_decode_gqa_fp8 (kv_decode_gqa8.hip) over e4m3 pages that hold ``quantize_fp8`` of
the same randn * 3 rows (bytes 2 * B * N * T * (128 + 4)) against batch_decode_gqa_f16 over the bf16 rows and batch_decode_gqa_i4 over their
int4 pages, the three alternating in the same rounds; then one record of the quantising append, ``append_kv_quantize_fp8`` against
``append_kv_quantize_i4`` at batch size 4, 28 kv heads, 28 layers.
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
from kv_bench import alternate, random_cache  # noqa: E402

P = 16
COLD_BYTES, MAX_LAYERS = 600e6, 512
HEADS = ((28, 4), (32, 8), (64, 8))


def record(B, Nq, N, T, dev, rounds):
    lib = _lib.lib()
    nbytes = 2 * B * N * T * 68
    layers = int(max(2, min(MAX_LAYERS, -(-COLD_BYTES // nbytes))))
    c = random_cache(B, N, T, layers, dev)
    tables = c.tables(T)
    q = torch.randn(B, Nq, 128, device=dev).to(torch.bfloat16)
    o = {"gqa": torch.empty_like(q), "i4": torch.empty_like(q)}
    fns = {"gqa": kvcache.batch_decode_gqa_i4, "i4": kvcache.batch_decode_i4}
    for n, fn in fns.items():
        fn(o[n], q, **tables, layer_idx=layers - 1)
    diff = float((o["gqa"].float() - o["i4"].float()).abs().max())
    chains = {n: [lambda layer=layer, n=n: fns[n](o[n], q, **tables, layer_idx=layer) for layer in range(layers)] for n in fns}
    us, spread = alternate(chains, rounds)
    nnz = tables["kv_indices"].numel()
    return {"Nq": Nq, "N": N, "g": Nq // N, "B": B, "positions": T, "page_size": P, "dtype": "bf16", "layers_rotated": layers,
            "cold": layers * nbytes >= COLD_BYTES, "bytes": nbytes, "gqa_us": round(us["gqa"], 2), "i4_us": round(us["i4"], 2),
            "gqa_GBps": round(nbytes / us["gqa"] / 1e3, 1), "i4_GBps": round(nbytes / us["i4"] / 1e3, 1), "speedup": round(us["i4"] / us["gqa"], 3),
            "round_spread": spread, "max_abs_diff": diff,
            "gqa_slices": int(lib.arcq_kv_decode_gqa_workspace_bytes(B, Nq, N, nnz, P)) // (B * Nq * 130 * 4) or 1,
            "i4_slices": int(lib.arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P)) // (B * Nq * 130 * 4) or 1}


def record_f16(B, Nq, N, T, dev, rounds):
    lib = _lib.lib()
    nbytes, nbytes_i4 = 2 * B * N * T * 256, 2 * B * N * T * 68
    layers = int(max(2, min(MAX_LAYERS, -(-COLD_BYTES // nbytes))))
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, N)
    t4 = c.tables(T)
    pages16 = (torch.randn(c.pages.shape[:-1] + (128,), device=dev, dtype=torch.bfloat16) * 3)
    for layer in range(layers):                          # the int4 pages: the quantised values of the same rows
        codes, scale, zero = kvcache.asym_quantize_and_pack_i4(pages16[:, layer])
        c.pages[:, layer] = codes
        c.scales[:, layer] = torch.cat((scale, zero), -1).to(torch.float16)
    t16 = dict(t4, kv_data=pages16)
    q = torch.randn(B, Nq, 128, device=dev).to(torch.bfloat16)
    fns = {"gqa16": (kvcache.batch_decode_gqa_f16, t16), "f16": (kvcache.batch_decode_f16, t16), "gqa_i4": (kvcache.batch_decode_gqa_i4, t4)}
    o = {n: torch.empty_like(q) for n in fns}
    for n, (fn, tables) in fns.items():
        fn(o[n], q, **tables, layer_idx=layers - 1)
    diff = float((o["gqa16"].float() - o["f16"].float()).abs().max())
    chains = {n: [lambda layer=layer, n=n: fns[n][0](o[n], q, **fns[n][1], layer_idx=layer) for layer in range(layers)] for n in fns}
    us, spread = alternate(chains, rounds)
    nnz = t4["kv_indices"].numel()
    return {"Nq": Nq, "N": N, "g": Nq // N, "B": B, "positions": T, "page_size": P, "dtype": "bf16", "layers_rotated": layers,
            "cold": layers * nbytes >= COLD_BYTES, "bytes": nbytes, "bytes_i4": nbytes_i4, "gqa16_us": round(us["gqa16"], 2),
            "f16_us": round(us["f16"], 2), "gqa_i4_us": round(us["gqa_i4"], 2), "gqa16_GBps": round(nbytes / us["gqa16"] / 1e3, 1),
            "f16_GBps": round(nbytes / us["f16"] / 1e3, 1), "gqa_i4_GBps": round(nbytes_i4 / us["gqa_i4"] / 1e3, 1),
            "speedup_over_f16": round(us["f16"] / us["gqa16"], 3), "time_over_gqa_i4": round(us["gqa16"] / us["gqa_i4"], 3),
            "round_spread": spread, "max_abs_diff_f16": diff,
            "gqa_slices": int(lib.arcq_kv_decode_gqa_workspace_bytes(B, Nq, N, nnz, P)) // (B * Nq * 130 * 4) or 1,
            "f16_slices": int(lib.arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P)) // (B * Nq * 130 * 4) or 1}


def record_fp8(B, Nq, N, T, dev, rounds):
    lib = _lib.lib()
    nbytes = {"fp8": 2 * B * N * T * 132, "gqa16": 2 * B * N * T * 256, "gqa_i4": 2 * B * N * T * 68}
    layers = int(max(2, min(MAX_LAYERS, -(-COLD_BYTES // nbytes["fp8"]))))
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, N)
    t4 = c.tables(T)
    pages16 = (torch.randn(c.pages.shape[:-1] + (128,), device=dev, dtype=torch.bfloat16) * 3)
    pages8 = torch.empty(pages16.shape, device=dev, dtype=torch.float8_e4m3fn)
    scales8 = torch.zeros_like(c.scales)
    for layer in range(layers):                          # the int4 and e4m3 pages: the quantised values of the same rows
        codes, scale, zero = kvcache.asym_quantize_and_pack_i4(pages16[:, layer])
        c.pages[:, layer] = codes
        c.scales[:, layer] = torch.cat((scale, zero), -1).to(torch.float16)
        code8, scale8 = kvcache.quantize_fp8(pages16[:, layer])
        pages8[:, layer] = code8
        scales8[:, layer, ..., 0:1] = scale8
    t16, t8 = dict(t4, kv_data=pages16), dict(t4, kv_data=pages8, kv_param=scales8)
    q = torch.randn(B, Nq, 128, device=dev).to(torch.bfloat16)
    fns = {"fp8": (kvcache.batch_decode_gqa_fp8, t8), "gqa16": (kvcache.batch_decode_gqa_f16, t16), "gqa_i4": (kvcache.batch_decode_gqa_i4, t4)}
    o = {n: torch.empty_like(q) for n in fns}
    for n, (fn, tables) in fns.items():
        fn(o[n], q, **tables, layer_idx=layers - 1)
    diff = float((o["fp8"].float() - o["gqa16"].float()).abs().max())
    chains = {n: [lambda layer=layer, n=n: fns[n][0](o[n], q, **fns[n][1], layer_idx=layer) for layer in range(layers)] for n in fns}
    us, spread = alternate(chains, rounds)
    nnz = t4["kv_indices"].numel()
    rec = {"Nq": Nq, "N": N, "g": Nq // N, "B": B, "positions": T, "page_size": P, "dtype": "bf16", "layers_rotated": layers,
           "cold": layers * nbytes["fp8"] >= COLD_BYTES}
    for n in fns:
        rec.update({f"{n}_bytes": nbytes[n], f"{n}_us": round(us[n], 2), f"{n}_TBps": round(nbytes[n] / us[n] / 1e6, 3)})
    rec.update({"time_over_gqa16": round(us["fp8"] / us["gqa16"], 3), "time_over_gqa_i4": round(us["fp8"] / us["gqa_i4"], 3), "round_spread": spread,
                "max_abs_diff_gqa16": diff, "gqa_slices": int(lib.arcq_kv_decode_gqa_workspace_bytes(B, Nq, N, nnz, P)) // (B * Nq * 130 * 4) or 1})
    return rec


def append_fp8(B, H, T, layers, dev, rounds):
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, H)
    t4 = c.tables(T)
    t8 = dict(t4, kv_data=torch.zeros(c.pages.shape[:-1] + (128,), device=dev, dtype=torch.float8_e4m3fn), kv_param=torch.zeros_like(c.scales))
    k, v = ((torch.randn(B, H, 128, device=dev) * 3).to(torch.bfloat16) for _ in range(2))
    chains = {"fp8": [lambda layer=layer: kvcache.append_kv_quantize_fp8(**t8, k=k, v=v, layer_idx=layer) for layer in range(layers)],
              "i4": [lambda layer=layer: kvcache.append_kv_quantize_i4(**t4, k=k, v=v, layer_idx=layer) for layer in range(layers)]}
    us, spread = alternate(chains, rounds)
    return {"what": "quantise + append one token per sequence", "B": B, "heads": H, "positions": T, "layers": layers, "dtype": "bf16",
            "append_kv_quantize_fp8_us": round(us["fp8"], 2), "append_kv_quantize_i4_us": round(us["i4"], 2),
            "time_over_i4": round(us["fp8"] / us["i4"], 3), "round_spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table", choices=("i4", "f16", "fp8"), default="i4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", {"i4": "kv_int4_decode_gqa.json", "f16": "kv_f16_decode_gqa.json", "fp8": "kv_fp8_decode_gqa.json"}[a.table])
    one = {"i4": record, "f16": record_f16, "fp8": record_fp8}[a.table]
    dev = torch.device("cuda:0")
    records = []
    with torch.no_grad():
        for Nq, N in HEADS:
            for B in (1, 4, 16):
                for T in (1040, 4096, 16384):
                    records.append(one(B, Nq, N, T, dev, a.rounds))
                    print(json.dumps(records[-1]), flush=True)
                    torch.cuda.empty_cache()
        if a.table == "fp8":
            records.append(append_fp8(4, 28, 1040, 28, dev, a.rounds))
            print(json.dumps(records[-1]), flush=True)
    res = {"tool": "tools/kv_gqa_bench.py", "table": a.table, "device": torch.cuda.get_device_name(0), "records": records}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
