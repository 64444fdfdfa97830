#!/usr/bin/env python3
"""The decode step of the int4 paged KV cache as one launch (arcquant_amd/kvstep.py) against the chain it replaces and against the
harness's bf16 kernel, on the same logical cache, in one process on one device; writes profiles/kv_int4_decode_step.json (the evidence
behind DESIGN.md 11, "Decode step").

    python tools/kv_step_bench.py [--layers 28] [--heads 28] [--out profiles/kv_int4_decode_step.json]

Three launch sets per layer, all starting from the same q|k|v projection output [B, 3 * heads * 128]:

    chain   what the harness does without kv_fused_step: the transposing copy of q|k|v, append_kv_quantize_i4, batch_decode_i4
            (the attention and, where the sequences are sliced, its combine): 3 or 4 launches
    step    decode_step_i4 on views of the same q|k|v: 1 launch
    bf16    arcq_harness_attn_decode, which appends to the dense bf16 cache and attends: 1 launch

Shapes and method are tools/kv_bench.py's: B = 4 and B = 1, `--heads` heads (kv heads == query heads), 1040 and 4096 positions (the new
one included), P = 16; a record's launch sets -- one per layer over `--layers` rotated caches -- are replayed from one HIP graph
(tools/mx_bench.py's graph_time); us is per layer.  The three ALTERNATE for `--rounds` rounds; a record keeps the best round of each and
`round_spread`, the largest (max - min) / min any of them showed between rounds.  `step_beats_chain` is step_us < chain_us by more than
that spread.
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

from arcquant_amd import _lib, kvcache, kvstep  # noqa: E402
from kv_bench import P, alternate, random_cache  # noqa: E402


def step(B, H, T, layers, dev, rounds):
    lib = _lib.lib()
    c = random_cache(B, H, T, layers, dev)
    tables = c.tables(T)
    qkv = torch.randn(B, 3 * H * 128, device=dev).to(torch.bfloat16)
    qv, kv_, vv = qkv.view(B, 3 * H, 128).split(H, dim=1)
    o = torch.empty(B, H, 128, dtype=torch.bfloat16, device=dev)
    state = kvstep.DecodeStepState(B, H, H, dev)
    dense = [torch.randn(2, B, H, T, 128, device=dev).to(torch.bfloat16) for _ in range(layers)]
    out = torch.empty(B, H * 128, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(max(int(lib.arcq_harness_attn_workspace_bytes(B, H, T)) // 4, 1), dtype=torch.float32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream     # noqa: E731

    def chain(layer):
        def f():
            qq, kk, vv2 = qkv.view(B, 3, H, 128).transpose(0, 1).contiguous().unbind(0)
            kvcache.append_kv_quantize_i4(**tables, k=kk, v=vv2, layer_idx=layer)
            kvcache.batch_decode_i4(o, qq, **tables, layer_idx=layer)
        return f

    def bf16(layer):
        def f():
            _lib.check(lib.arcq_harness_attn_decode(qkv.data_ptr(), dense[layer][0].data_ptr(), dense[layer][1].data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                    B, H, T, T - 1, stream()), "harness attn_decode")
        return f
    chains = {"chain": [chain(layer) for layer in range(layers)],
              "step": [lambda layer=layer: kvstep.decode_step_i4(o, qv, kv_, vv, **tables, layer_idx=layer, state=state) for layer in range(layers)],
              "bf16": [bf16(layer) for layer in range(layers)]}
    us, spread = alternate(chains, rounds)
    slices = int(lib.arcq_kv_decode_workspace_bytes(B, H, H, tables["kv_indices"].numel(), P)) // (B * H * 130 * 4) or 1
    assert not state.counters.any(), "the arrival counters were not handed back zeroed"
    return {"what": "decode step: append + attention", "B": B, "heads": H, "positions": T, "page_size": P, "layers_rotated": layers,
            "chain_us": round(us["chain"], 2), "chain_launches": 3 + (slices > 1), "step_us": round(us["step"], 2), "bf16_us": round(us["bf16"], 2),
            "step_saves_us": round(us["chain"] - us["step"], 2), "step_over_bf16": round(us["step"] / us["bf16"], 3), "round_spread": spread,
            "step_beats_chain": bool(us["step"] < us["chain"] * (1 - spread)), "int4_slices_per_sequence": slices}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--heads", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_int4_decode_step.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    with torch.no_grad():
        for B in (4, 1):
            for T in (1040, 4096):
                records.append(step(B, a.heads, T, a.layers, dev, a.rounds))
                print(json.dumps(records[-1]), flush=True)
                torch.cuda.empty_cache()
    res = {"tool": "tools/kv_step_bench.py", "device": torch.cuda.get_device_name(0), "records": records}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
