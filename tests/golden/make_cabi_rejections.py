"""Writes tests/golden/cabi_rejections.json: what the eleven GEMM / linear entry points of the C-ABI answer to calls they must reject
(or accept as empty) BEFORE their first HIP call -- status and ``arcq_last_error()`` text.  tests/test_cabi.py replays the table against
the built library and compares for equality, so a change of the validation code cannot change which fault a call reports, or how.

Every pointer is a stand-in address that is never dereferenced: each case ends in a rejection (-1 shape, -2 unsupported, -4 NULL) or in
the empty-shape return (0 with M == 0 or N == 0).  The script refuses to write a table with any other outcome, so no case can reach a
launch.  Run it on the commit whose behaviour is to be pinned:  python tests/golden/make_cabi_rejections.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

P = 4096                       # 16-byte aligned stand-in address
BIG = 1 << 30                  # > INT32_MAX / 2, a multiple of 128


# Per entry point: ``order`` = its arguments in C order (the fused linears' KQ is called K here, so that one override means the same
# everywhere), ``p16`` / ``p4`` = the pointers it wants 16- / 4-byte aligned, ``base`` = a shape it would run, ``faults`` = its
# divisibility / enum faults, ``limits`` = one shape per size limit, ``opt`` = optional pointers and the offset that misaligns them,
# ``unsupported`` = calls its `supported` predicate (or a rule of its own) refuses.
K_FAULT = [("K % 64", dict(K=100))]
SPECS = [
    dict(name="arcq_gemm_nvfp4", order=["A", "B", "SFA", "SFB", "D", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "residual", "out_dtype",
                                         "workspace", "workspace_bytes", "stream"],
         p16=["A", "B", "D"], p4=["SFA", "SFB"], base=dict(M=32, N=128, K=128),
         faults=K_FAULT, limits=[dict(M=BIG), dict(N=BIG), dict(K=BIG), dict(M=1 << 21, N=1 << 21)]),
    dict(name="arcq_gemm_nvfp4_silu_mul", order=["A", "B", "SFA", "SFB", "ACT", "absmax_slots", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "stream"],
         p16=["A", "B", "ACT"], p4=["SFA", "SFB", "absmax_slots"], base=dict(M=32, N=128, K=128),
         faults=K_FAULT + [("N % 8", dict(N=132))], limits=[dict(M=BIG), dict(N=BIG), dict(K=BIG), dict(M=1 << 21, N=1 << 21)],
         unsupported=[dict(M=16, bias=P), dict(M=16, bias=P, A=P + 8), dict(M=16, bias=P, SFA=None)]),
    dict(name="arcq_gemm_nvfp4_repacked", order=["A", "RW", "SFA", "RSF", "D", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "residual", "out_dtype", "stream"],
         p16=["A", "RW", "D"], p4=["SFA", "RSF"], base=dict(M=4, N=4096, K=4160),
         faults=K_FAULT, limits=[dict(N=BIG), dict(K=BIG)], opt=dict(bias=2, residual=4),
         unsupported=[dict(M=129), dict(M=BIG), dict(M=129, N=4098, bias=P + 2)]),
    dict(name="arcq_gemm_nvfp4_repacked_stream", order=["A", "RW", "SFA", "RSF", "D", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "residual", "out_dtype", "stream"],
         p16=["A", "RW", "D"], p4=["SFA", "RSF"], base=dict(M=4, N=4096, K=4160),
         faults=K_FAULT, limits=[dict(N=BIG), dict(K=BIG)], opt=dict(bias=2, residual=4),
         unsupported=[dict(M=17), dict(M=BIG), dict(M=17, N=4098, residual=P + 4)]),
    dict(name="arcq_gemm_nvfp4_repacked_silu_absmax", order=["A", "RW", "SFA", "RSF", "D", "absmax_slots", "M", "N", "K", "alpha_host", "alpha_dev", "stream"],
         p16=["A", "RW", "D"], p4=["SFA", "RSF", "absmax_slots"], base=dict(M=4, N=4096, K=4160),
         faults=K_FAULT + [("N % 4", dict(N=4098))], limits=[dict(N=BIG), dict(K=BIG)], unsupported=[dict(M=129), dict(M=BIG)]),
    dict(name="arcq_gemm_nvfp4_rw", order=["A", "RW", "SFA", "RSF", "D", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "residual", "out_dtype", "workspace",
                                            "workspace_bytes", "stream"],
         p16=["A", "RW", "D"], p4=["SFA", "RSF"], base=dict(M=32, N=128, K=128),
         faults=K_FAULT, limits=[dict(M=BIG), dict(N=BIG), dict(K=BIG), dict(M=1 << 21, N=1 << 21)],
         # a misaligned bias keeps a decode shape off the repacked kernels; this weight is beyond the register-tiled kernel's 32-bit offsets
         unsupported=[dict(M=4, N=1 << 29, K=4160, bias=P + 2)]),
    dict(name="arcq_gemm_nvfp4_rw_silu_mul", order=["A", "RW", "SFA", "RSF", "ACT", "absmax_slots", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "stream"],
         p16=["A", "RW", "ACT"], p4=["SFA", "RSF", "absmax_slots"], base=dict(M=32, N=128, K=128),
         faults=K_FAULT + [("N % 8", dict(N=132))], limits=[dict(M=BIG), dict(N=BIG), dict(K=BIG), dict(M=1 << 21, N=1 << 21)],
         unsupported=[dict(M=16), dict(M=1), dict(M=16, A=None), dict(M=16, SFA=P + 2), dict(M=16, N=132)]),
    dict(name="arcq_gemm_mxfp4", order=["A", "B", "SFA", "SFB", "D", "M", "N", "K", "alpha_host", "alpha_dev", "bias", "residual", "out_dtype", "workspace",
                                         "workspace_bytes", "stream"],
         p16=["A", "B", "D"], p4=["SFA", "SFB"], base=dict(M=32, N=128, K=128),
         faults=[("K % 128", dict(K=192)), ("N % 16", dict(N=136))],
         limits=[dict(M=65535 * 128 + 1, N=16), dict(N=BIG), dict(K=BIG), dict(M=1 << 21, N=1 << 21)], opt=dict(bias=1, residual=1)),
    dict(name="arcq_linear_rmsnorm_repacked", order=["X", "Wn", "eps", "reorder_index", "RW", "RSF", "D", "M", "N", "K", "KE", "variant", "alpha_host", "alpha_dev",
                                                      "bias", "residual", "out_dtype", "stream"],
         p16=["X", "reorder_index", "RW", "D", "Wn"], p4=["RSF"], base=dict(M=4, N=3584, K=3584, KE=64, variant=1),
         faults=[("KQ % 64", dict(K=3600)), ("KE % 64", dict(KE=100)), ("KE > KQ", dict(KE=3648)), ("KE < 0", dict(KE=-64)), ("variant", dict(variant=7))],
         limits=[dict(N=BIG), dict(K=32768)], opt=dict(bias=2, residual=4),
         unsupported=[dict(M=17), dict(K=1024), dict(M=17, N=3586, bias=P + 2)]),
    dict(name="arcq_linear_rmsnorm_silu_repacked", order=["X", "Wn", "eps", "reorder_index", "RW", "RSF", "ACT", "absmax_slots", "M", "N", "K", "KE", "variant",
                                                           "alpha_host", "alpha_dev", "bias", "act_scatter_index", "stream"],
         p16=["X", "reorder_index", "RW", "ACT", "Wn"], p4=["RSF", "absmax_slots"], base=dict(M=4, N=3584, K=3584, KE=64, variant=1),
         faults=[("KQ % 64", dict(K=3600)), ("KE % 64", dict(KE=100)), ("KE > KQ", dict(KE=3648)), ("variant", dict(variant=7)), ("N % 4", dict(N=3586))],
         limits=[dict(N=BIG), dict(K=32768)], opt=dict(bias=4, act_scatter_index=2), unsupported=[dict(M=17), dict(M=17, act_scatter_index=P)],
         out_dtype=False),
    dict(name="arcq_linear_dynamic_repacked", order=["X", "reorder_index", "RW", "RSF", "D", "scale_out", "absmax_slots", "nslots", "M", "N", "K", "KE", "variant",
                                                      "alpha_host", "bias", "residual", "out_dtype", "stream"],
         p16=["X", "reorder_index", "RW", "D"], p4=["RSF"], base=dict(M=4, N=3584, K=3584, KE=64, variant=1, scale_out=P, absmax_slots=None, nslots=0),
         faults=[("KQ % 64", dict(K=3600)), ("KE % 64", dict(KE=100)), ("KE > KQ", dict(KE=3648)), ("variant", dict(variant=7)),
                 ("nslots", dict(absmax_slots=P, nslots=0)), ("nslots", dict(absmax_slots=P, nslots=1 << 31)), ("absmax_slots", dict(absmax_slots=P + 2, nslots=8))],
         limits=[dict(N=BIG), dict(K=32768)], opt=dict(bias=2, residual=4), unsupported=[dict(M=17), dict(M=17, absmax_slots=P, nslots=8)]),
]


def _cases(s):
    base = {a: None for a in s["order"]}
    base.update({p: P for p in s["p16"] + s["p4"]}, alpha_host=1.0, workspace_bytes=0, eps=1e-6, out_dtype=0)
    base.update(s["base"])
    has_od = "out_dtype" in s["order"]
    ptrs = [a for a in s["order"] if a in s["p16"] or a in s["p4"]]
    nulls = {p: None for p in ptrs}
    first16, first4 = s["p16"][0], s["p4"][0]
    out = [f[1] for f in s["faults"]]
    out += [dict(K=0), dict(M=-1), dict(N=-1)]
    if has_od:
        out += [dict(out_dtype=7), dict(out_dtype=-1)]
    out += [dict(M=0), dict(N=0), dict(M=0, **nulls), dict(N=0, **nulls), dict(M=0, N=0)]
    out += [{p: None} for p in ptrs]
    out += [{p: P + 8} for p in s["p16"]] + [{p: P + 2} for p in s["p4"]]
    for name, off in s.get("opt", {}).items():
        out += [{name: P + off}, {name: P + off, "M": 0}]
    out += s["limits"]
    out += list(s.get("unsupported", ()))
    # pairs of faults from different classes: which one is reported is part of the contract
    shape = s["faults"][0][1]
    out += [dict(shape, **{first16: None}), dict(shape, **{first4: P + 2}), dict(shape, M=0), dict(shape, **nulls)]
    if has_od:
        out += [dict(out_dtype=7, **{first16: None}), dict(out_dtype=7, M=0), dict(out_dtype=7, **shape), dict(out_dtype=7, **s["limits"][0])]
    out += [{ptrs[-1]: None, first16: P + 8}, {first16: P + 8, first4: P + 2}, {first4: None, ptrs[-1]: P + 2}]
    out += [dict(s["limits"][0], **{first16: None}), dict(s["limits"][0], **{first16: P + 8}), dict(s["limits"][-1], **{first4: P + 2})]
    for name, off in s.get("opt", {}).items():
        out += [{name: P + off, first16: P + 8}, {name: P + off, first4: None}, dict(s["limits"][0], **{name: P + off})]
    for f in s["faults"][1:]:
        out += [dict(f[1], **{first16: None}), dict(f[1], M=0)]
    seen, cases = set(), []
    for over in out:
        args = [dict(base, **over)[a] for a in s["order"]]
        if json.dumps(args) not in seen:
            seen.add(json.dumps(args))
            cases.append(dict(fn=s["name"], args=args, M=dict(base, **over)["M"], N=dict(base, **over)["N"]))
    return cases


def main():
    from arcquant_amd import _lib
    L = _lib.lib()
    table = []
    for s in SPECS:
        for c in _cases(s):
            st = int(getattr(L, c["fn"])(*c["args"]))
            ok = st in (-1, -2, -4) or (st == 0 and (c["M"] == 0 or c["N"] == 0))
            if not ok:
                raise SystemExit(f"{c['fn']}{tuple(c['args'])} -> {st}: not a rejection, such a case must not be in the table")
            table.append(dict(fn=c["fn"], args=c["args"], M=c["M"], N=c["N"], status=st,
                              error=L.arcq_last_error().decode() if st else ""))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cabi_rejections.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in table) + "\n]\n")
    print(f"{len(table)} cases -> {path}")


if __name__ == "__main__":
    main()
