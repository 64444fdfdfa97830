"""Writes tests/golden/cabi_rejections.json: what the eleven GEMM / linear entry points of the C-ABI answer to calls they must reject
(or accept as empty) BEFORE their first HIP call -- status and ``arcq_last_error()`` text.  tests/test_cabi.py replays the table against
the built library and compares for equality, so a change of the validation code cannot change which fault a call reports, or how.

Every pointer is a stand-in address that is never dereferenced: each case ends in a rejection (-1 shape, -2 unsupported, -4 NULL) or in
the empty-shape return (0 with M == 0 or N == 0).  The script refuses to write a table with any other outcome, so no case can reach a
launch.  Run it on the commit whose behaviour is to be pinned:  python tests/golden/make_cabi_rejections.py

A second table, tests/golden/cabi_quant_rejections.json, holds the same for the twelve quantiser entry points (QUANT_SPECS below; rows == 0
is their empty shape), replayed by its own test of tests/test_cabi.py.
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


# ---- the quantisers: tests/golden/cabi_quant_rejections.json ---------------------------------------------------------------------------
# Per entry point: ``order`` = its arguments in C order (the row count is called M everywhere), ``align`` = every pointer it needs with
# the alignment it demands BEFORE its first HIP call (0: none), ``data`` = the pointers that may be NULL when M == 0, ``base`` = a shape
# it would run.  ``neg_rows`` / ``big_rows``: M < 0 and M > INT32_MAX are rejections of this entry before its first HIP call.
#   arcq_quantize_x_dyn and the two arcq_silu_mul_quantize_x_dyn* accept M < 0 as empty (0 with rows != 0: not a case for this table).
#   arcq_quantize_x_dyn (beyond the decode-sized single launch) and arcq_silu_mul_quantize_x_dyn launch their abs-max pass before the row
#   limit and the reorder_index / QX / SFX alignment are looked at, and the identity form of arcq_quantize_x_dyn_slots has no row limit:
#   those faults reach a HIP call there, so the table cannot hold them (arcq_quantize_x_dyn's base shape is decode-sized).
_NV = ["X", "reorder_index", "QX", "SFX", "M", "KQ", "KE", "variant", "stream"]
_NV_ALIGN = dict(X=16, reorder_index=16, QX=8, SFX=4)
_MX_ALIGN = dict(X=16, reorder_index=16, QX=16, SFX=0)
_DATA = ["X", "reorder_index", "QX", "SFX"]
QUANT_SPECS = [
    dict(name="arcq_quantize_x", order=_NV, align=_NV_ALIGN, data=_DATA, base=dict(variant=1), neg_rows=True, big_rows=True),
    dict(name="arcq_quantize_w", order=_NV, align=_NV_ALIGN, data=_DATA, base=dict(variant=1), neg_rows=True, big_rows=True),
    dict(name="arcq_rmsnorm_quantize_x", order=["X", "W", "eps", "reorder_index", "QX", "SFX", "M", "KQ", "KE", "variant", "stream"],
         align=dict(_NV_ALIGN, W=16), data=_DATA + ["W"], base=dict(KQ=4096, variant=0), neg_rows=True, big_rows=True, rms="W"),
    dict(name="arcq_quantize_x_dyn", order=["X", "reorder_index", "QX", "SFX", "scale_out", "state", "M", "KQ", "KE", "variant", "stream"],
         align=dict(_NV_ALIGN, scale_out=0, state=0), data=_DATA, base=dict(variant=1), dyn=["scale_out", "state"]),
    dict(name="arcq_quantize_x_dyn_slots", order=["X", "reorder_index", "QX", "SFX", "scale_out", "absmax_slots", "nslots", "M", "KQ", "KE", "variant", "stream"],
         align=dict(_NV_ALIGN, scale_out=0, absmax_slots=0), data=_DATA, base=dict(variant=1), neg_rows=True, big_rows=True,
         dyn=["scale_out", "absmax_slots"], keep="reorder_index"),      # (without it the call is the next group's)
    # reorder_index == NULL: X is already in reordered channel order (its own kernel, its own checks)
    dict(name="arcq_quantize_x_dyn_slots", group="arcq_quantize_x_dyn_slots, reorder_index == NULL",
         order=["X", "reorder_index", "QX", "SFX", "scale_out", "absmax_slots", "nslots", "M", "KQ", "KE", "variant", "stream"],
         align=dict(X=16, QX=8, SFX=4, scale_out=0, absmax_slots=0), data=["X", "QX", "SFX"], base=dict(variant=1), neg_rows=True,
         dyn=["scale_out", "absmax_slots"]),
    dict(name="arcq_silu_mul_quantize_x_dyn", order=["X", "reorder_index", "QX", "SFX", "scale_out", "state", "M", "KQ", "KE", "variant", "layout", "stream"],
         align=dict(X=16, reorder_index=0, QX=0, SFX=0, scale_out=0, state=0), data=_DATA, base=dict(variant=1), dyn=["scale_out", "state"]),
    dict(name="arcq_silu_mul_quantize_x_dyn_slots", order=["X", "reorder_index", "QX", "SFX", "scale_out", "absmax_slots", "nslots", "M", "KQ", "KE", "variant",
                                                            "layout", "stream"],
         align=dict(_NV_ALIGN, scale_out=0, absmax_slots=0), data=_DATA, base=dict(variant=1), big_rows=True, dyn=["scale_out", "absmax_slots"]),
    dict(name="arcq_mx_quantize_x", order=_NV[:7] + ["stream"], align=_MX_ALIGN, data=_DATA, neg_rows=True, big_rows=True),
    dict(name="arcq_mx_quantize_w", order=_NV[:7] + ["stream"], align=_MX_ALIGN, data=_DATA, neg_rows=True, big_rows=True),
    dict(name="arcq_mx_rmsnorm_quantize_x", order=["X", "W", "eps", "reorder_index", "QX", "SFX", "M", "KQ", "KE", "stream"],
         align=dict(_MX_ALIGN, W=16), data=_DATA + ["W"], base=dict(KQ=4096), neg_rows=True, big_rows=True, rms="W"),
    dict(name="arcq_mx_silu_mul_quantize_x", order=_NV[:7] + ["layout", "stream"], align=_MX_ALIGN, data=_DATA, neg_rows=True, big_rows=True),
]


def _quant_cases(s):
    """One case per fault, pointer and pairing that the entry has: the table stays readable, a second value per fault would pin nothing more."""
    order, align, data = s["order"], s["align"], s["data"]
    base = {a: None for a in order}
    base.update({p: P for p in align}, eps=1e-6, M=4, KQ=3584, KE=64, variant=0, layout=0, nslots=8)
    base.update(s.get("base", {}))
    KQ, big = base["KQ"], dict(M=1 << 31)
    mis = {p: P + a // 2 for p, a in align.items() if a}         # one misaligned address per pointer with an alignment rule
    shape = [dict(KQ=KQ + 16), dict(KE=100), dict(KE=-64), dict(KE=KQ + 64), dict(KQ=0), dict(KQ=32768)]
    shape += [dict(KQ=1024), dict(KQ=8256)] if s.get("rms") else []
    shape += [dict(M=-1)] if s.get("neg_rows") else []
    enums = [{e: 7} for e in ("variant", "layout") if e in order]
    slots = [dict(nslots=0), dict(nslots=1 << 31)] if "nslots" in order else []
    faults = shape + enums + slots + ([big] if s.get("big_rows") else [])
    nulls, x, q = {p: None for p in data}, data[0], "QX"
    out = faults + [{p: None} for p in align] + [{p: v} for p, v in mis.items()]
    out += [dict(M=0), dict(M=0, **nulls), dict(M=0, **{p: None for p in align}), dict(shape[0], M=0), dict(shape[5], M=0), dict(M=0, **{x: mis[x]})]
    out += [dict(e, M=0) for e in enums + slots[:1]]
    # pairs of faults from different classes: which one is reported is part of the contract
    out += [dict(shape[0], **{x: None}), dict(shape[0], **{x: mis[x]}), dict(shape[5], **{x: None}), {x: None, q: mis.get(q, P)}, {"SFX": None, x: mis[x]}]
    out += [dict(shape[0], **e) for e in enums + slots[:1]] + [dict(shape[5], **e) for e in enums] + [dict(e, **{x: None}) for e in enums + slots[:1]]
    out += [{x: mis[x], q: mis[q]}] if q in mis else []
    out += [dict(big, **{x: None}), dict(big, **{x: mis[x]}), dict(big, **shape[0])] if s.get("big_rows") else []
    for d in s.get("dyn", ()):
        out += [dict(shape[0], **{d: None}), {d: None, "M": 0}, {d: None, x: None}]
    if s.get("rms"):
        w = s["rms"]
        out += [dict(shape[0], **{w: mis[w]}), dict(shape[6], **{w: mis[w]}), {w: mis[w], "M": 0}, {w: mis[w], x: None}, {w: None, x: mis[x]}, dict(big, **{w: mis[w]})]
        out += [dict(e, **{w: mis[w]}) for e in enums]
    seen, cases = set(), []
    for over in out:
        full = dict(base, **over)
        args = [full[a] for a in order]
        if json.dumps(args) not in seen and full.get(s.get("keep"), P) is not None:
            seen.add(json.dumps(args))
            cases.append(args)
    return dict(fn=s["name"], group=s.get("group", s["name"]), rows_arg=order.index("M"), cases=cases)


def _absmax_cases():
    """arcq_absmax_scale(X, n, scale_out, stream) has no empty return (n == 0 still issues a memset): rejections only."""
    out = [(x, n, so) for n in (-1, -(1 << 40)) for x in (P, None, P + 2) for so in (P, None)]
    out += [(x, n, None) for n in (0, 8) for x in (P, None, P + 8)]
    out += [(None, 1, P), (None, 1 << 40, P)] + [(P + off, n, P) for off in (1, 2, 4, 8) for n in (0, 4096)]
    return dict(fn="arcq_absmax_scale", group="arcq_absmax_scale", rows_arg=1, cases=[[x, n, so, None] for x, n, so in out])


def quant_main(L):
    """The table: one object per entry point (``group``: the reorder_index == NULL form of arcq_quantize_x_dyn_slots apart), its cases as
    [args, status, error text], ``rows_arg`` = which argument is the row count."""
    groups = [_quant_cases(s) for s in QUANT_SPECS] + [_absmax_cases()]
    for g in groups:
        for i, args in enumerate(g["cases"]):
            st = int(getattr(L, g["fn"])(*args))
            ok = st in (-1, -2, -4) or (st == 0 and args[g["rows_arg"]] == 0 and g["fn"] != "arcq_absmax_scale")
            if not ok:
                raise SystemExit(f"{g['fn']}{tuple(args)} -> {st}: not a rejection, such a case must not be in the table")
            g["cases"][i] = [args, st, L.arcq_last_error().decode() if st else ""]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cabi_quant_rejections.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(dict(g, cases=[])).replace("[]}", "[\n") + ",\n".join(json.dumps(c) for c in g["cases"]) + "\n]}"
                                    for g in groups) + "\n]\n")
    print(f"{sum(len(g['cases']) for g in groups)} cases, at least {min(len(g['cases']) for g in groups)} per entry point -> {path}")


def main():
    from arcquant_amd import _lib
    L = _lib.lib()
    quant_main(L)
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
