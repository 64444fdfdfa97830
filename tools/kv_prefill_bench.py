#!/usr/bin/env python3
"""Causal prefill attention over the int4 paged KV cache (kvcache.batch_prefill_i4) against what a caller had to do without it, in one
process on one device; writes profiles/kv_int4_prefill.json (the evidence behind DESIGN.md 11 "Prefill").

    python tools/kv_prefill_bench.py [--layers 4] [--rounds 3] [--harness-layers 8] [--out profiles/kv_int4_prefill.json]

Shapes: Qwen2.5-7B attention, 28 query heads of 128, with N = 28 kv heads (the harness's) and N = 4 (the model's GQA), P = 16:
bs = 4 with a chunk of 512 new tokens over 0 / 1024 / 4096 cached positions, and bs = 1 x 2048 from empty.  bf16.
Comparators:
  (a) gather     over the SAME pages with torch: index the pages by the table, unpack_i4_and_asym_dequantize to bf16, then
                 F.scaled_dot_product_attention with the causal offset mask;
  (b) dense      from-empty shapes only: F.scaled_dot_product_attention(is_causal=True) on dense bf16 K / V of the call -- the harness
                 path the flag replaces (it attends over UNQUANTISED K / V, so it computes something else).
Method (tools/mx_bench.py's graph_time): a record's launches -- one per layer over `--layers` layers of one cache -- are replayed from
one HIP graph, warmed for ~40 ms and timed for >= 10 ms between two events; us is per launch.  The candidates ALTERNATE for `--rounds`
rounds; a record keeps the best round of each and `round_spread`, the largest (max - min) / min any showed between rounds.
FLOPs are the causal ones, 4 * 128 * (positions a query attends to) per query row; the roof is BASELINE.md's bf16-MFMA 2.52 PFLOP/s.
Bytes are what the kernel must read and write once: 2 * B * N * T * 68 of pages + 2 * tokens * Nq * 256 of q and o.
`--harness-layers` > 0 adds e2e.bench_decode (bs = 4, prefill 1024, that many layers) with the flag unset and set, alternating twice.
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

from arcquant_amd import kvcache  # noqa: E402
from mx_bench import graph_time  # noqa: E402

P, NQ, D = 16, 28, 128
ROOF_TFLOPS = 2520.0


def alternate(chains, rounds):
    seen = {n: [] for n in chains}
    for _ in range(rounds):
        for n, launches in chains.items():
            seen[n].append(graph_time(launches))
    return {n: min(t) for n, t in seen.items()}, round(max((max(t) - min(t)) / min(t) for t in seen.values()), 3)


def shape(B, N, cached, n_new, layers, dev, rounds):
    T, g = cached + n_new, NQ // N
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, N)
    c.pages.copy_(torch.randint(0, 256, c.pages.shape, dtype=torch.uint8, device=dev))
    c.scales[..., 0] = 0.4
    c.scales[..., 1] = 3.0
    tables = c.prefill_tables(T, n_new)
    qo = tables.pop("qo_indptr")
    q = torch.randn(B * n_new, NQ, D, device=dev).to(torch.bfloat16)
    o = torch.empty_like(q)
    cnt = c.page_cnt_from_length(T)
    own = tables["kv_indices"].view(B, cnt).long()
    mask = torch.arange(T, device=dev).unsqueeze(0) <= (cached + torch.arange(n_new, device=dev)).unsqueeze(1)        # [n_new, T]
    q4 = q.view(B, n_new, NQ, D).transpose(1, 2)

    def gather(layer):
        def f():
            rows = c.pages[own, layer].permute(0, 2, 3, 1, 4, 5).reshape(B, 2, N, cnt * P, 64)[:, :, :, :T]
            prm = c.scales[own, layer].permute(0, 2, 3, 1, 4, 5).reshape(B, 2, N, cnt * P, 2)[:, :, :, :T]
            kv = kvcache.unpack_i4_and_asym_dequantize(rows, prm[..., 0:1], prm[..., 1:2]).to(torch.bfloat16)
            k, v = kv[:, 0], kv[:, 1]
            if g > 1:
                k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
            return F.scaled_dot_product_attention(q4, k, v, attn_mask=mask)
        return f
    chains = {"prefill_i4": [lambda layer=layer: kvcache.batch_prefill_i4(o, q, qo, **tables, layer_idx=layer) for layer in range(layers)],
              "gather_dequant_sdpa": [gather(layer) for layer in range(layers)]}
    if cached == 0:
        dk, dv = (torch.randn(B, N, T, D, device=dev).to(torch.bfloat16) for _ in range(2))
        if g > 1:
            chains["dense_sdpa"] = [lambda: F.scaled_dot_product_attention(q4, dk.repeat_interleave(g, dim=1), dv.repeat_interleave(g, dim=1), is_causal=True)]
        else:
            chains["dense_sdpa"] = [lambda: F.scaled_dot_product_attention(q4, dk, dv, is_causal=True)]
    us, spread = alternate(chains, rounds)
    flops = 4 * D * B * NQ * (n_new * cached + n_new * (n_new + 1) // 2)
    nbytes = 2 * B * N * T * 68 + 2 * B * n_new * NQ * D * 2
    rec = {"what": "causal prefill attention", "B": B, "query_heads": NQ, "kv_heads": N, "cached": cached, "new_tokens": n_new, "page_size": P,
           "layers_rotated": layers, "causal_gflop": round(flops / 1e9, 2), "bytes": nbytes, "workgroups": -(-n_new // (128 // g)) * B * N,
           "prefill_i4_us": round(us["prefill_i4"], 1), "prefill_i4_tflops": round(flops / us["prefill_i4"] / 1e6, 1),
           "prefill_i4_fraction_of_bf16_mfma_roof": round(flops / us["prefill_i4"] / 1e6 / ROOF_TFLOPS, 4),
           "prefill_i4_GBps": round(nbytes / us["prefill_i4"] / 1e3, 1),
           "gather_dequant_sdpa_us": round(us["gather_dequant_sdpa"], 1), "speedup_over_gather_dequant_sdpa": round(us["gather_dequant_sdpa"] / us["prefill_i4"], 2),
           "round_spread": spread}
    if "dense_sdpa" in us:
        rec.update(dense_sdpa_us=round(us["dense_sdpa"], 1), dense_sdpa_tflops=round(flops / us["dense_sdpa"] / 1e6, 1),
                   speedup_over_dense_sdpa=round(us["dense_sdpa"] / us["prefill_i4"], 2))
    return rec


def harness(layers):
    from arcquant_amd import e2e
    out = []
    for flag in (False, True, False, True):
        r = e2e.bench_decode("qwen2.5-7b", batch=4, prefill=1024, steps=16, layers=layers, fused=True, attention="cache", kv_cache="int4",
                             kv_paged_prefill=flag)
        out.append({k: r.get(k) for k in ("layers", "batch", "prefill", "prefill_ms", "prefill_tok_per_s", "decode_tok_per_s", "kv_paged_prefill")})
        out[-1]["kv_paged_prefill"] = flag
        print(json.dumps(out[-1]), flush=True)
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--harness-layers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_int4_prefill.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    with torch.no_grad():
        for N in (28, 4):
            for B, cached, n_new in ((4, 0, 512), (4, 1024, 512), (4, 4096, 512), (1, 0, 2048)):
                records.append(shape(B, N, cached, n_new, a.layers, dev, a.rounds))
                print(json.dumps(records[-1]), flush=True)
                torch.cuda.empty_cache()
        res = {"tool": "tools/kv_prefill_bench.py", "device": torch.cuda.get_device_name(0), "bf16_mfma_roof_tflops": ROOF_TFLOPS, "records": records}
        if a.harness_layers > 0:
            res["harness"] = harness(a.harness_layers)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
