#!/usr/bin/env python3
"""RoPE on the KV path (arcquant_amd/kvrope.py): the rotation fused into the int4 cache's quantising write against what a caller writes
without it, in one process on one device; writes profiles/kv_rope.json (the evidence behind DESIGN.md 11 "RoPE").

    python tools/kv_rope_bench.py [--layers 28] [--heads 28] [--out profiles/kv_rope.json]

Shapes: Qwen2.5-7B's 28 heads of 128 (kv heads == query heads, as the harness models them), bf16, P = 16; a decode step at bs = 1 and 4
over 1040 positions and a prefill of bs = 4 x 512 tokens.  q, k and v are the slices of one [tokens, 3 * heads * 128] projection output, as
in the harness.  Per shape, per layer:

    fused        kvrope.rope_append_kv_quantize_i4 / rope_init_kv_quantize_i4: rotation, contiguous q and the quantising write, ONE launch
    eager_rope   torch eager x * cos + rotate_half(x) * sin on q and k (tables gathered by position), v made contiguous, then
                 kvcache.append_kv_quantize_i4 / init_kv_quantize_i4: what a caller of the reference's apply_rotary_pos_emb writes today
    no_rope      the RoPE-free pair the fused call replaces in the harness: one transposing copy + the quantising write
    rope_qk      kvrope.rope_qk_ alone, in place on the q and k slices

Method (tools/kv_bench.py's): a record's launches -- one per layer over `--layers` layers of one cache -- are replayed from one HIP graph,
warmed for ~40 ms and timed for >= 10 ms between two events; us is per layer.  The four ALTERNATE for `--rounds` rounds; a record keeps the
best round of each and `round_spread`, the largest (max - min) / min any of them showed between rounds.
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

from arcquant_amd import kvcache, kvrope  # noqa: E402
from kv_bench import alternate  # noqa: E402

P = 16


def rotate_half(x):
    return torch.cat((-x[..., 64:], x[..., :64]), dim=-1)


def bench(B, q_len, T, H, layers, dev, rounds, theta):
    """B sequences of T positions, the last q_len of them new (q_len = 1: a decode step)."""
    ntok = B * q_len
    c = kvcache.PagedKVCacheI4(B, P, T, dev, layers, H)
    tables = c.prefill_tables(T, q_len)
    qo = tables.pop("qo_indptr")
    cos, sin = kvrope.rope_tables(T, theta, torch.bfloat16, dev)
    positions = torch.arange(T - q_len, T, dtype=torch.int32, device=dev)
    pos_long = positions.long().repeat(B)
    qkv = (torch.randn(ntok, 3 * H * 128, device=dev) * 2).to(torch.bfloat16)
    q, k, v = qkv.view(ntok, 3 * H, 128).split(H, dim=1)
    q_out = torch.empty((ntok, H, 128), dtype=torch.bfloat16, device=dev)
    decode = q_len == 1

    def write(kk, vv, layer):
        if decode:
            kvcache.append_kv_quantize_i4(**tables, k=kk, v=vv, layer_idx=layer)
        else:
            kvcache.init_kv_quantize_i4(**tables, k=kk, v=vv, seqlen_indptr=qo, layer_idx=layer)

    def fused(layer):
        if decode:
            kvrope.rope_append_kv_quantize_i4(q_out, q, k, v, cos, sin, **tables, layer_idx=layer)
        else:
            kvrope.rope_init_kv_quantize_i4(q_out, q, k, v, cos, sin, **tables, seqlen_indptr=qo, layer_idx=layer)

    def eager_rope(layer):
        cs, sn = cos[pos_long].unsqueeze(1), sin[pos_long].unsqueeze(1)
        q_rot = q * cs + rotate_half(q) * sn
        k_rot = k * cs + rotate_half(k) * sn
        write(k_rot, v.contiguous(), layer)
        return q_rot

    def no_rope(layer):
        qq, kk, vv = qkv.view(ntok, 3, H, 128).transpose(0, 1).contiguous().unbind(0)
        write(kk, vv, layer)
        return qq

    def rope_qk(layer):
        kvrope.rope_qk_(q, k, positions, cos, sin)

    chains = {name: [lambda layer=layer, f=f: f(layer) for layer in range(layers)]
              for name, f in (("fused", fused), ("eager_rope", eager_rope), ("no_rope", no_rope), ("rope_qk", rope_qk))}
    us, spread = alternate(chains, rounds)
    return {"what": "decode step" if decode else "prefill", "B": B, "new_tokens_per_sequence": q_len, "positions": T, "heads": H, "page_size": P,
            "layers_rotated": layers, "rope_theta": theta,
            "fused_rope_write_us": round(us["fused"], 2), "eager_rope_copy_write_us": round(us["eager_rope"], 2),
            "no_rope_copy_write_us": round(us["no_rope"], 2), "rope_qk_us": round(us["rope_qk"], 2),
            "fused_over_eager_rope": round(us["eager_rope"] / us["fused"], 2), "fused_over_no_rope_pair": round(us["no_rope"] / us["fused"], 2),
            "round_spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--heads", type=int, default=28)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--theta", type=float, default=1e6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_rope.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    records = []
    with torch.no_grad():
        for B, q_len, T in ((1, 1, 1040), (4, 1, 1040), (4, 512, 512)):
            records.append(bench(B, q_len, T, a.heads, a.layers, dev, a.rounds, a.theta))
            print(json.dumps(records[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/kv_rope_bench.py", "device": torch.cuda.get_device_name(0), "records": records}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
