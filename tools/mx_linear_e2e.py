#!/usr/bin/env python3
"""The decode step of the Qwen2.5-7B shape with and without the MXFP4 fused decode linears (DecoderModel's mx_fused_linears), beside the
unflagged MXFP4 model and the NVFP4 default; writes profiles/mxfp4_linear_e2e.jsonl.

    python tools/mx_linear_e2e.py [--rounds 2] [--parent-root DIR] [--out FILE]

Every figure is e2e.bench_decode's `fused`, attention "current" line (bs = 4, prefill 1024, 28 layers, the decode step replayed from a
HIP graph) taken in a FRESH process; the configurations alternate for `--rounds` rounds, and every record carries its row name and round.
--parent-root names a built checkout of the parent commit: its unflagged figure (mx_repacked_only, which has no fused linears there) is then
taken in the same alternation, as row "parent_commit:mxfp4_repacked_only", by the parent's own code and library.  This process never
touches the GPU."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = [
    ("nvfp4_default", dict()),
    ("mxfp4", dict(quant_type="MXFP4")),
    ("mxfp4_repacked_only", dict(quant_type="MXFP4", mx_repacked_only=True)),
    ("mxfp4_repacked_only+fused_qkv_o_gateup", dict(quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears="qkv,o,gateup")),
    ("mxfp4_repacked_only+fused_qkv", dict(quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears="qkv")),
    ("mxfp4_repacked_only+fused_o", dict(quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears="o")),
    ("mxfp4_repacked_only+fused_gateup", dict(quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears="gateup")),
]

ONE = ("import json, sys; sys.path.insert(0, sys.argv[1]); from arcquant_amd import e2e; kw = json.loads(sys.argv[2]); "
       "print('RESULT ' + json.dumps(e2e.bench_decode('qwen2.5-7b', fused=True, attention='current', **kw)), flush=True)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows", default=None)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mxfp4_linear_e2e.jsonl"))
    a = ap.parse_args()
    rows = [(n, kw, ROOT) for n, kw in ROWS]
    if a.parent_root:
        rows.append(("parent_commit:mxfp4_repacked_only", dict(quant_type="MXFP4", mx_repacked_only=True), os.path.abspath(a.parent_root)))
    want = a.rows.split(",") if a.rows else [r[0] for r in rows]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        for rnd in range(a.rounds):
            for name, kw, root in rows:
                if name not in want:
                    continue
                r = subprocess.run([sys.executable, "-c", ONE, root, json.dumps(kw)], capture_output=True, text=True, timeout=600, cwd=root)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not lines:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit(f"mx_linear_e2e: {name} round {rnd} failed with exit code {r.returncode}: nothing further is started")
                rec = dict(row=name, round=rnd, **json.loads(lines[0][len("RESULT "):]))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
