"""Writes tests/golden/cabi_kv_rejections.json and tests/golden/kv_python_rejections.json: what the paged KV cache's boundary answers to
calls it must reject (or accept as empty) BEFORE its first HIP call.  tests/test_kv_rejections.py replays both tables and compares for
equality, so a change of the validation code cannot change which fault a call reports, or how.

cabi_kv_rejections.json: the ten validating entry points of include/arcq_kv.h -- status and ``arcq_last_error()`` text -- and a handful of
values of the two pure-integer size functions.  Every pointer is a stand-in address that is never dereferenced: each case ends in a
rejection (-1 shape, -2 unsupported, -4 NULL, -5 workspace) or in the empty return (0 with B == 0 or ntok == 0).  The script refuses to
write a table with any other outcome, so no case can reach a launch.

kv_python_rejections.json: the exact ``str()`` of the RuntimeError that CPU tensors provoke in every public function of kvcache, kvstep,
kvprefill and kvrope.  From a valid CPU argument set one thing is broken at a time; the unbroken set ends in "must live on the GPU", and
where tensors live is checked last, so no case can launch either.  A tensor is recorded as {"t": dtype, "shape": ..., "stride": ...} (the
stride only where it is not the contiguous one); its contents are never read.

Run it on the commit whose behaviour is to be pinned:  python tests/golden/make_kv_rejections.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

X = 4096                       # 16-byte aligned stand-in address
FAR = 1 << 20                  # q_out's: apart from q
BIG = 1 << 30                  # > INT32_MAX / 2
TOP = BIG - 1                  # the largest dimension the boundary takes
INT32_MAX = (1 << 31) - 1
MAX_TABLE_BYTES = 127332       # (the size of cabi_rejections.json)

TABLES = ["kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_offset"]
GEOM = ["B", "L", "layer_idx", "N", "P", "format"]
SIZE_FNS = ("arcq_kv_decode_workspace_bytes", "arcq_kv_decode_step_state_bytes")

# Per entry point: ``order`` = its arguments in C order, ``p16`` / ``p4`` = the pointers it wants 16- / 4-byte aligned (all required),
# ``opt4`` = pointers it takes NULL but wants 4-byte aligned, ``empty`` = the counts whose zero ends the call early, ``int4only`` = it
# refuses ARCQ_KV_16BIT, ``strides`` = the names of its two token strides, ``rows`` = a shape beyond its row range.  Which checks an entry
# point has follows from which arguments it takes.
SPECS = [
    dict(name="arcq_rope_qk", order=["q", "k", "q_stride", "k_stride", "positions", "n_pos", "cos", "sin", "rope_len", "ntok", "Nq", "N", "dtype", "stream"],
         p16=["q", "k", "cos", "sin"], p4=["positions"], empty=["ntok"], strides=("q_stride", "k_stride"), base=dict(ntok=6, n_pos=3),
         rows=dict(ntok=TOP, n_pos=1, Nq=32, N=16)),
    dict(name="arcq_kv_rope_append_quantize", order=TABLES + ["q_out", "q", "k", "v", "q_stride", "kv_stride", "cos", "sin", "rope_len", "B", "Nq", "L", "layer_idx",
                                                              "N", "P", "format", "dtype", "stream"],
         p16=["kv_data", "q_out", "q", "k", "v", "cos", "sin"], p4=TABLES[1:], empty=["B"], int4only=True, strides=("q_stride", "kv_stride"),
         rows=dict(B=TOP, Nq=32, N=16)),
    dict(name="arcq_kv_rope_init_quantize", order=TABLES + ["q_out", "q", "k", "v", "q_stride", "kv_stride", "cos", "sin", "rope_len", "seqlen_indptr", "ntok", "B",
                                                            "Nq", "L", "layer_idx", "N", "P", "format", "dtype", "stream"],
         p16=["kv_data", "q_out", "q", "k", "v", "cos", "sin"], p4=TABLES[1:] + ["seqlen_indptr"], empty=["B", "ntok"], int4only=True,
         strides=("q_stride", "kv_stride"), rows=dict(ntok=TOP, Nq=32, N=16)),
    dict(name="arcq_kv_init", order=TABLES + ["k", "v", "k_param", "v_param", "seqlen_indptr", "ntok"] + GEOM + ["stream"],
         p16=["kv_data", "k", "v"], p4=TABLES[1:] + ["k_param", "v_param", "seqlen_indptr"], empty=["B", "ntok"]),
    dict(name="arcq_kv_append", order=TABLES + ["k", "v", "k_param", "v_param"] + GEOM + ["stream"],
         p16=["kv_data", "k", "v"], p4=TABLES[1:] + ["k_param", "v_param"], empty=["B"]),
    dict(name="arcq_kv_append_quantize", order=TABLES + ["k", "v"] + GEOM + ["dtype", "stream"],
         p16=["kv_data", "k", "v"], p4=TABLES[1:], empty=["B"], int4only=True),
    dict(name="arcq_kv_init_quantize", order=TABLES + ["k", "v", "seqlen_indptr", "ntok"] + GEOM + ["dtype", "stream"],
         p16=["kv_data", "k", "v"], p4=TABLES[1:] + ["seqlen_indptr"], empty=["B", "ntok"], int4only=True),
    dict(name="arcq_kv_batch_decode", order=["o", "q"] + TABLES + ["B", "Nq", "L", "layer_idx", "N", "P", "nnz", "format", "dtype", "workspace", "workspace_bytes",
                                                                   "stream"],
         p16=["o", "q", "kv_data"], p4=TABLES[1:], opt4=["workspace"], empty=["B"]),
    dict(name="arcq_kv_batch_prefill", order=["o", "q", "qo_indptr"] + TABLES + ["ntok", "B", "Nq", "L", "layer_idx", "N", "P", "nnz", "format", "dtype", "stream"],
         p16=["o", "q", "kv_data"], p4=["qo_indptr"] + TABLES[1:], empty=["B", "ntok"], int4only=True),
    dict(name="arcq_kv_decode_step", order=["o", "q", "k", "v", "q_stride", "kv_stride"] + TABLES + ["B", "Nq", "L", "layer_idx", "N", "P", "nnz", "format", "dtype",
                                                                                                   "workspace", "workspace_bytes", "state", "state_bytes", "stream"],
         p16=["o", "q", "k", "v", "kv_data"], p4=TABLES[1:], opt4=["workspace", "state"], empty=["B"], int4only=True, strides=("q_stride", "kv_stride")),
]
# a shape at which decode attention splits the sequence, so arcq_kv_decode_workspace_bytes is positive
SPLIT = dict(B=1, Nq=1, N=1, nnz=1024, P=16, L=2, layer_idx=1)


def _overrides(s, L):
    """The overrides of one entry point's valid call, one case each."""
    def has(a):
        return a in s["order"]

    name, ptrs = s["name"], [a for a in s["order"] if a in s["p16"] or a in s["p4"]]
    nulls = dict({p: None for p in ptrs}, **{p: None for p in s.get("opt4", ())})
    first16, first4, last = s["p16"][0], s["p4"][0], ptrs[-1]
    qs, ks = s.get("strides", (None, None))
    rope_qk = name == "arcq_rope_qk"
    cls = {}                   # fault class -> its first single fault, for the pairs below
    out = []

    def add(kind, *overs):
        cls.setdefault(kind, overs[0])
        out.extend(overs)

    # ---- every single fault
    if has("format"):
        add("enum", dict(format=2))
    if has("dtype"):
        add("enum", dict(dtype=2))
    if has("L"):
        add("geometry", dict(P=0), dict(B=-1), dict(L=0), dict(N=0), dict(layer_idx=-1), dict(layer_idx=2))
        add("limit", dict(B=BIG), dict(L=BIG), dict(P=BIG), dict(N=65536))
    if has("ntok"):
        add("ntok", dict(ntok=-1))
        add("limit", dict(ntok=BIG, n_pos=1))
    if has("Nq"):
        add("Nq", dict(Nq=3), dict(Nq=0))
        add("limit", dict(Nq=65536) if not rope_qk else dict(Nq=65536, N=0, k=None))
        if rope_qk:
            add("Nq", dict(N=-1), dict(N=3))
            add("limit", dict(Nq=65536 * 2, N=65536))
    if has("nnz"):
        add("nnz", dict(nnz=-1))
        add("limit", dict(nnz=BIG), dict(nnz=1 << 28, P=16))
    if has("rope_len"):
        add("rope_len", dict(rope_len=0))
        add("limit", dict(rope_len=BIG))
    if has("n_pos"):
        add("n_pos", dict(n_pos=4), dict(n_pos=0), dict(n_pos=12))
        add("limit", dict(n_pos=BIG))
    if qs:
        add("stride", {qs: 504}, {qs: 516}, {ks: 248}, {ks: 260})
        add("limit", {qs: BIG}, {ks: BIG})
    if "rows" in s:
        add("limit", s["rows"])
    if has("workspace"):
        add("limit", dict(B=1 << 20, Nq=1 << 10))                                 # B * Nq
    if s.get("int4only"):
        add("int4only", dict(format=1))
    # ---- the empty returns, alone, with every pointer NULL, with a shape fault, with a refusal
    late = {qs: 8} if qs else dict(P=0)
    zero = {s["empty"][0]: 0}
    out += [zero, dict(zero, **nulls), dict(zero, **late), dict(zero, format=1) if has("format") else zero, dict(zero, **{first16: X + 8, first4: X + 2}),
            dict(zero, Nq=3) if has("Nq") else zero]
    if len(s["empty"]) == 2:
        out += [dict(ntok=0), dict(ntok=0, **nulls), dict(ntok=0, **late), dict(B=0, ntok=-1)]
    # ---- pointers: NULL and misaligned, one at a time
    add("NULL", *[{p: None} for p in ptrs])
    add("mis16", *[{p: X + 8} for p in s["p16"]])
    add("mis4", *[{p: X + 2} for p in s["p4"]])
    # ---- pairs of faults from different classes: which one is reported is part of the contract
    # (the classes an entry point checks one after the other, so every step of its order is held)
    for a, b in (("enum", "NULL"), ("enum", "geometry"), ("geometry", "Nq"), ("ntok", "Nq"), ("Nq", "nnz"), ("Nq", "rope_len"), ("nnz", "ntok"),
                 ("ntok", "int4only"), ("rope_len", "int4only"), ("rope_len", "n_pos"), ("rope_len", "stride"), ("n_pos", "stride"),
                 ("stride", "int4only"), ("int4only", "NULL")):
        if a in cls and b in cls:
            out.append(dict(cls[a], **cls[b]))
    if has("dtype"):
        out += [dict(dtype=2, P=0) if has("L") else dict(dtype=2, ntok=-1)]
    lim = cls["limit"]
    out += [dict(lim, **{first16: None}), dict(s["rows"], **{first4: X + 2}) if "rows" in s else dict(lim, **{first4: X + 2})]
    if "rows" in s:
        out += [dict(s["rows"], **zero) if not rope_qk else dict(s["rows"], **{qs: 504})]
    out += [{last: None, first16: X + 8}, {first16: X + 8, first4: X + 2}, nulls]
    # ---- what single entry points have of their own
    if name == "arcq_rope_qk":
        out += [dict(N=0, k=None, k_stride=0, q=None), dict(N=0, k=None, k_stride=0, cos=X + 8), dict(N=0, k=X + 8, k_stride=4, positions=X + 2),
                dict(N=0, k=None, k_stride=0, q_stride=504), dict(N=0, k=None, k_stride=0, Nq=0), dict(N=0, k=None, k_stride=0, rope_len=0),
                dict(N=0, k=None, k_stride=0, ntok=0), dict(k=None), dict(k=None, q=X + 8), dict(ntok=7)]
    if "q_out" in s["order"]:
        rows = s["base"]["ntok"] if has("ntok") else s["base"]["B"]
        out += [dict(q_out=X + 1024), dict(q_out=X + rows * 1024 - 16), dict(q=1 << 16, q_out=(1 << 16) - rows * 1024 + 16), dict(q_out=X, q_stride=1024),
                dict(q_out=X, q_stride=1024, kv_param=X + 2), dict(q_out=X, q_stride=1024, cos=None), dict(q_out=X + 1024, B=0)]
    if name in ("arcq_kv_init", "arcq_kv_append", "arcq_kv_batch_decode"):
        # these take 16-bit caches: a valid one together with one more fault
        out += [dict(format=1, **{first16: None}), dict(format=1, **{first16: X + 8}), dict(format=1, **{first4: X + 2})]
    if name == "arcq_kv_batch_decode":
        out += [dict(format=1, kv_param=None, o=None), dict(format=1, kv_param=None, q=X + 8), dict(format=1, kv_param=None, kv_indptr=X + 2),
                dict(format=1, kv_param=X + 2)]
    if has("workspace"):
        need = int(L.arcq_kv_decode_workspace_bytes(SPLIT["B"], SPLIT["Nq"], SPLIT["N"], SPLIT["nnz"], SPLIT["P"]))
        assert need > 0, "the split shape no longer needs a workspace"
        ws = dict(SPLIT, workspace=X, workspace_bytes=need)
        out += [dict(SPLIT), dict(ws, workspace_bytes=need - 1), dict(ws, workspace=None), dict(ws, workspace_bytes=-1),
                dict(SPLIT, q=X + 8), dict(SPLIT, kv_param=X + 2), dict(SPLIT, o=None), dict(ws, workspace=X + 2), dict(workspace=X + 2, workspace_bytes=BIG),
                dict(ws, workspace_bytes=need - 1, kv_indices=X + 2)]
        if has("state"):
            need_state = int(L.arcq_kv_decode_step_state_bytes(SPLIT["B"], SPLIT["Nq"], SPLIT["N"]))
            assert need_state > 0
            out += [dict(ws), dict(ws, state=X, state_bytes=need_state - 1), dict(ws, state=None, state_bytes=need_state),
                    dict(ws, state=X + 2, state_bytes=need_state), dict(ws, workspace_bytes=need - 1, state=X, state_bytes=need_state),
                    dict(ws, workspace=None, state=X, state_bytes=need_state), dict(SPLIT, state=X, state_bytes=need_state),
                    # no workspace needed, so no state either: the call rejects for the other fault
                    dict(state=None, q=X + 8), dict(state=None, o=None), dict(state=X + 2, state_bytes=BIG)]
    return out


def _cases(s, L):
    base = {a: None for a in s["order"]}
    base.update({p: X for p in s["p16"] + s["p4"]}, B=3, L=2, layer_idx=1, N=2, P=5, Nq=4, ntok=5, nnz=4, rope_len=16, format=0, dtype=0, workspace_bytes=0,
                state_bytes=0)
    base.update(s.get("base", {}))
    if "q_out" in base:
        base["q_out"] = FAR
    base = {a: base[a] for a in s["order"]}
    s["base"] = base
    qs, ks = s.get("strides", (None, None))
    seen, cases = set(), []
    for over in _overrides(s, L):
        v = dict(base, **over)
        if qs:                 # contiguous rows unless the case sets a stride
            v[qs] = over.get(qs, max(v["Nq"], 0) * 128)
            v[ks] = over.get(ks, max(v["N"], 0) * 128)
        args = [v[a] for a in s["order"]]
        if json.dumps(args) not in seen:
            seen.add(json.dumps(args))
            cases.append(dict(fn=s["name"], args=args, B=v.get("B"), ntok=v.get("ntok")))
    return cases


def c_table():
    from arcquant_amd import _lib
    L = _lib.lib()
    table = []
    for s in SPECS:
        for c in _cases(s, L):
            st = int(getattr(L, c["fn"])(*c["args"]))
            if not (st in (-1, -2, -4, -5) or (st == 0 and (c["B"] == 0 or c["ntok"] == 0))):
                raise SystemExit(f"{c['fn']}{tuple(c['args'])} -> {st}: not a rejection, such a case must not be in the table")
            row = dict(fn=c["fn"], args=c["args"], status=st, error=L.arcq_last_error().decode() if st else "")
            table.append(row if st else dict(row, B=c["B"], ntok=c["ntok"]))
    for fn, rows in (("arcq_kv_decode_workspace_bytes", [(1, 1, 1, 1024, 16), (4, 28, 4, 264, 16), (3, 4, 2, 4, 5), (64, 32, 8, 64 * 512, 16), (1, 8, 8, 1 << 20, 16),
                                                         (1, 1, 1, 0, 16), (0, 4, 2, 4, 5), (3, 0, 2, 4, 5), (3, 4, 0, 4, 5), (3, 3, 2, 4, 5)]),
                     ("arcq_kv_decode_step_state_bytes", [(1, 1, 1), (3, 4, 2), (4, 28, 4), (4, 28, 28), (2, 64, 1), (0, 4, 2), (3, 0, 2), (3, 4, 0), (3, 3, 2)])):
        table += [dict(fn=fn, args=list(r), status=int(getattr(L, fn)(*r)), error="") for r in rows]
    per_fn = {s["name"]: sum(c["fn"] == s["name"] for c in table) for s in SPECS}
    assert len(table) >= 300 and min(per_fn.values()) >= 20, per_fn
    text = "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in table) + "\n]\n"
    assert len(text) <= MAX_TABLE_BYTES, len(text)
    return text, f"{len(table)} cases, {per_fn}"


# ---------------------------------------------------------------------------------------------------------------- the Python mirrors
def enc(v):
    """A value of a call as JSON: tensors by dtype, shape and (where not contiguous) stride."""
    import torch
    from arcquant_amd import kvstep
    if isinstance(v, torch.Tensor):
        d = dict(t=str(v.dtype).split(".")[1], shape=list(v.shape))
        if not v.is_contiguous():
            d["stride"] = list(v.stride())
        return d
    if isinstance(v, torch.dtype):
        return dict(dtype=str(v).split(".")[1])
    if isinstance(v, kvstep.DecodeStepState):
        return dict(state=[v.batch_size, v.num_q_heads, v.num_kv_heads])
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items()}
    assert v is None or isinstance(v, (int, float, str)), v
    return v


def dec(v):
    """The inverse (tests/test_kv_rejections.py has its own copy)."""
    import torch
    from arcquant_amd import kvstep
    if not isinstance(v, dict):
        return v
    if "dtype" in v:
        return getattr(torch, v["dtype"])
    if "state" in v:
        return kvstep.DecodeStepState(*v["state"], "cpu")
    if "t" not in v:
        return {k: dec(x) for k, x in v.items()}
    dtype, shape = getattr(torch, v["t"]), v["shape"]
    if "stride" not in v:
        return torch.zeros(shape, dtype=dtype)
    return torch.zeros(1 + sum((n - 1) * s for n, s in zip(shape, v["stride"])), dtype=dtype).as_strided(shape, v["stride"])


def py_cases():
    """[(function, what is broken, keyword arguments)], the last of each function being its unbroken set."""
    import torch
    from arcquant_amd import kvstep
    F16, BF16, F32, U8, I32 = torch.float16, torch.bfloat16, torch.float32, torch.uint8, torch.int32
    PAGES, L, N, P, B, ROPE_LEN, NQ = 4, 2, 2, 5, 3, 16, 4
    z = torch.zeros

    def i32(n):
        return z(n, dtype=I32)

    def tables(i4=True, dtype=F16):
        return dict(kv_data=z((PAGES, L, 2, N, P, 64 if i4 else 128), dtype=U8 if i4 else dtype), kv_param=z((PAGES, L, 2, N, P, 2), dtype=F16),
                    kv_indptr=i32(B + 1), kv_indices=i32(4), last_page_offset=i32(B), layer_idx=1)

    def sliced(ntok, dtype=F16):
        return z((ntok, NQ + 2 * N, 128), dtype=dtype).split([NQ, N, N], dim=1)

    def noncontig(t):          # same shape, the last dimension two elements apart
        return z(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)[..., ::2]

    out = []

    def generic(fn, base, rows=(), optional=()):
        """dtype, rank and contiguity (``rows``: the row rules instead) of every tensor; ``optional``: None is a valid one."""
        for key, t in base.items():
            if not isinstance(t, torch.Tensor):
                continue
            out.append((fn, f"{key} dtype", dict(base, **{key: t.to(torch.float64 if t.dtype is F32 else F32)})))
            if t.dtype in (F16, BF16):
                out.append((fn, f"{key} other 16-bit dtype", dict(base, **{key: t.to(BF16 if t.dtype is F16 else F16)})))
            out.append((fn, f"{key} rank", dict(base, **{key: t.unsqueeze(0)})))
            if key not in optional:
                out.append((fn, f"{key} not a tensor", dict(base, **{key: None})))
            if key not in rows:
                out.append((fn, f"{key} non-contiguous", dict(base, **{key: noncontig(t)})))
                continue
            n, h = t.shape[0], t.shape[1]
            out.append((fn, f"{key} head stride", dict(base, **{key: z((n, 2 * h, 128), dtype=t.dtype)[:, ::2]})))
            out.append((fn, f"{key} element stride", dict(base, **{key: z((n, h, 256), dtype=t.dtype)[:, :, ::2]})))
            out.append((fn, f"{key} head dimension", dict(base, **{key: z((n, h, 64), dtype=t.dtype)})))
            out.append((fn, f"{key} token stride % 8", dict(base, **{key: z((n, h * 128 + 4), dtype=t.dtype)[:, :h * 128].view(n, h, 128)})))
            out.append((fn, f"{key} token stride too small", dict(base, **{key: z((h * 128 + (n - 1) * 128,), dtype=t.dtype).as_strided((n, h, 128), (128, 128, 1))})))
            if key == "q":             # (k's and v's strides must stay equal)
                out.append((fn, f"{key} padded (valid)", dict(base, **{key: z((n, h * 128 + 8), dtype=t.dtype)[:, :h * 128].view(n, h, 128)})))

    def cache_faults(fn, base, i4=True):
        row = 64 if i4 else 128
        d = base["kv_data"].dtype
        for what, over in (("cache row width", dict(kv_data=z((PAGES, L, 2, N, P, row // 2), dtype=d))),
                           ("cache K/V pair", dict(kv_data=z((PAGES, L, 3, N, P, row), dtype=d))),
                           ("kv_param shape", dict(kv_param=z((PAGES, L, 2, N, P, 4), dtype=F16))),
                           ("kv_param pages", dict(kv_param=z((PAGES + 1, L, 2, N, P, 2), dtype=F16))),
                           ("no layer", dict(kv_data=z((PAGES, 0, 2, N, P, row), dtype=d), kv_param=z((PAGES, 0, 2, N, P, 2), dtype=F16))),
                           ("no head", dict(kv_data=z((PAGES, L, 2, 0, P, row), dtype=d), kv_param=z((PAGES, L, 2, 0, P, 2), dtype=F16))),
                           ("no page entry", dict(kv_data=z((PAGES, L, 2, N, 0, row), dtype=d), kv_param=z((PAGES, L, 2, N, 0, 2), dtype=F16))),
                           ("layer_idx = L", dict(layer_idx=L)), ("layer_idx < 0", dict(layer_idx=-1)),
                           ("kv_indptr short", dict(kv_indptr=i32(B))), ("kv_indptr long", dict(kv_indptr=i32(B + 2))),
                           ("last_page_offset long", dict(last_page_offset=i32(B + 1)))):
            out.append((fn, what, dict(base, **over)))

    # ---- kvcache: the reference's six and the quantising pair
    for i4 in (True, False):
        sfx, row, rd = ("i4", 64, U8) if i4 else ("f16", 128, F16)
        for init in (True, False):
            fn = f"kvcache.{'init' if init else 'append'}_kv_{sfx}"
            ntok = B + 2 if init else B
            base = dict(tables(i4), k=z((ntok, N, row), dtype=rd), v=z((ntok, N, row), dtype=rd), k_param=z((ntok, N, 2), dtype=F16),
                        v_param=z((ntok, N, 2), dtype=F16))
            if init:
                base["seqlen_indptr"] = i32(B + 1)
            generic(fn, base)
            cache_faults(fn, base, i4)
            for what, over in (("v shape", dict(v=z((ntok, N, row // 2), dtype=rd))), ("k heads", dict(k=z((ntok, N + 1, row), dtype=rd))),
                               ("k and v heads", dict(k=z((ntok, N + 1, row), dtype=rd), v=z((ntok, N + 1, row), dtype=rd))),
                               ("k_param shape", dict(k_param=z((ntok, N, 4), dtype=F16))), ("v_param tokens", dict(v_param=z((ntok + 1, N, 2), dtype=F16))),
                               ("tokens", dict(k=z((ntok + 1, N, row), dtype=rd), v=z((ntok + 1, N, row), dtype=rd)))):
                out.append((fn, what, dict(base, **over)))
            if init:
                out.append((fn, "seqlen_indptr length", dict(base, seqlen_indptr=i32(B))))
            if not i4:
                bf = dict(base, kv_data=base["kv_data"].to(BF16), k=base["k"].to(BF16), v=base["v"].to(BF16))
                out.append((fn, "a bfloat16 cache (valid)", bf))
                out.append((fn, "a bfloat16 cache, float16 rows", dict(bf, k=base["k"])))
            out.append((fn, "valid", base))
        fn = f"kvcache.batch_decode_{sfx}"
        base = dict(o=z((B, NQ, 128), dtype=F16), q=z((B, NQ, 128), dtype=F16), **tables(i4))
        generic(fn, base)
        cache_faults(fn, base, i4)
        for what, over in (("o shape", dict(o=z((B, N, 128), dtype=F16))), ("batch", dict(o=z((B + 1, NQ, 128), dtype=F16), q=z((B + 1, NQ, 128), dtype=F16))),
                           ("head dimension", dict(o=z((B, NQ, 64), dtype=F16), q=z((B, NQ, 64), dtype=F16))),
                           ("Nq % N", dict(o=z((B, 3, 128), dtype=F16), q=z((B, 3, 128), dtype=F16))),
                           ("Nq = 0", dict(o=z((B, 0, 128), dtype=F16), q=z((B, 0, 128), dtype=F16))),
                           ("bfloat16 o and q" + (" (valid)" if i4 else " over a float16 cache"), dict(o=z((B, NQ, 128), dtype=BF16), q=z((B, NQ, 128), dtype=BF16)))):
            out.append((fn, what, dict(base, **over)))
        out.append((fn, "valid", base))
    for init in (True, False):
        fn = f"kvcache.{'init' if init else 'append'}_kv_quantize_i4"
        ntok = B + 2 if init else B
        base = dict(tables(), k=z((ntok, N, 128), dtype=F16), v=z((ntok, N, 128), dtype=F16))
        if init:
            base["seqlen_indptr"] = i32(B + 1)
        generic(fn, base)
        cache_faults(fn, base)
        for what, over in (("v shape", dict(v=z((ntok, N, 64), dtype=F16))), ("k and v heads", dict(k=z((ntok, N + 1, 128), dtype=F16), v=z((ntok, N + 1, 128), dtype=F16))),
                           ("tokens" + (" (valid: seqlen_indptr's contents are the caller's)" if init else ""),
                            dict(k=z((ntok + 1, N, 128), dtype=F16), v=z((ntok + 1, N, 128), dtype=F16))),
                           ("uint8 rows", dict(k=z((ntok, N, 64), dtype=U8), v=z((ntok, N, 64), dtype=U8))),
                           ("a 16-bit cache", dict(kv_data=z((PAGES, L, 2, N, P, 128), dtype=F16))),
                           ("bfloat16 rows (valid)", dict(k=z((ntok, N, 128), dtype=BF16), v=z((ntok, N, 128), dtype=BF16)))):
            out.append((fn, what, dict(base, **over)))
        if init:
            out.append((fn, "seqlen_indptr length", dict(base, seqlen_indptr=i32(B + 2))))
        out.append((fn, "valid", base))
    out.append(("kvcache.unpack_i4_and_asym_dequantize", "q dtype", dict(q=z((2, 64), dtype=torch.int8), scale=z((2, 1), dtype=F16), zero=z((2, 1), dtype=F16))))

    # ---- kvprefill
    fn = "kvprefill.batch_prefill_i4"
    ntok = B + 2
    base = dict(o=z((ntok, NQ, 128), dtype=F16), q=z((ntok, NQ, 128), dtype=F16), qo_indptr=i32(B + 1), **tables())
    generic(fn, base)
    cache_faults(fn, base)
    for what, over in (("qo_indptr length", dict(qo_indptr=i32(B))), ("o shape", dict(o=z((ntok, N, 128), dtype=F16))), ("o tokens", dict(o=z((ntok + 1, NQ, 128), dtype=F16))),
                       ("head dimension", dict(o=z((ntok, NQ, 64), dtype=F16), q=z((ntok, NQ, 64), dtype=F16))),
                       ("Nq % N", dict(o=z((ntok, 3, 128), dtype=F16), q=z((ntok, 3, 128), dtype=F16))),
                       ("Nq = 0", dict(o=z((ntok, 0, 128), dtype=F16), q=z((ntok, 0, 128), dtype=F16))),
                       ("a 16-bit cache", dict(kv_data=z((PAGES, L, 2, N, P, 128), dtype=F16))),
                       ("no tokens (valid)", dict(o=z((0, NQ, 128), dtype=F16), q=z((0, NQ, 128), dtype=F16))),
                       ("bfloat16 (valid)", dict(o=z((ntok, NQ, 128), dtype=BF16), q=z((ntok, NQ, 128), dtype=BF16)))):
        out.append((fn, what, dict(base, **over)))
    out.append((fn, "valid", base))

    # ---- kvstep
    fn = "kvstep.decode_step_i4"
    q, k, v = sliced(B)
    base = dict(o=z((B, NQ, 128), dtype=F16), q=q, k=k, v=v, **tables(), state=None)
    generic(fn, base, rows=("q", "k", "v"))
    cache_faults(fn, base)
    for what, over in (("k and v token strides differ", dict(v=z((B, N * 128 + 8), dtype=F16)[:, :N * 128].view(B, N, 128))),
                       ("state of another type", dict(state=7)), ("state of another batch", dict(state=kvstep.DecodeStepState(B + 1, NQ, N, "cpu"))),
                       ("state of other heads", dict(state=kvstep.DecodeStepState(B, 2 * NQ, N, "cpu"))),
                       ("a matching state (valid)", dict(state=kvstep.DecodeStepState(B, NQ, N, "cpu"))),
                       ("o shape", dict(o=z((B, N, 128), dtype=F16))), ("batch", dict(o=z((B + 1, NQ, 128), dtype=F16), q=z((B + 1, NQ, 128), dtype=F16))),
                       ("k heads", dict(k=z((B, N + 1, 128), dtype=F16))), ("k and v heads", dict(k=z((B, N + 1, 128), dtype=F16), v=z((B, N + 1, 128), dtype=F16))),
                       ("k and v tokens", dict(k=z((B + 1, N, 128), dtype=F16), v=z((B + 1, N, 128), dtype=F16))),
                       ("Nq % N", dict(o=z((B, 3, 128), dtype=F16), q=z((B, 3, 128), dtype=F16))),
                       ("Nq = 0", dict(o=z((B, 0, 128), dtype=F16), q=z((B, 0, 128), dtype=F16))),
                       ("a 16-bit cache", dict(kv_data=z((PAGES, L, 2, N, P, 128), dtype=F16))),
                       ("contiguous rows (valid)", dict(q=z((B, NQ, 128), dtype=F16), k=z((B, N, 128), dtype=F16), v=z((B, N, 128), dtype=F16)))):
        out.append((fn, what, dict(base, **over)))
    out.append((fn, "valid", base))
    for what, a in (("batch_size", (0, NQ, N)), ("num_kv_heads", (B, NQ, 0)), ("num_q_heads", (B, 0, N)), ("Nq % N", (B, 3, N)), ("negative", (B, -4, -2))):
        out.append(("kvstep.DecodeStepState", what, dict(batch_size=a[0], num_q_heads=a[1], num_kv_heads=a[2], device="cpu")))

    # ---- kvrope
    for what, over in (("rope_len = 0", dict(rope_len=0)), ("rope_len < 0", dict(rope_len=-3)), ("float32", dict(rope_len=8, dtype=F32)),
                       ("uint8", dict(rope_len=8, dtype=U8)), ("both", dict(rope_len=0, dtype=F32))):
        out.append(("kvrope.rope_tables", what, over))
    fn = "kvrope.rope_qk_"
    q, k, _ = sliced(6)
    base = dict(q=q, k=k, positions=i32(3), cos=z((ROPE_LEN, 128), dtype=F16), sin=z((ROPE_LEN, 128), dtype=F16))
    generic(fn, base, rows=("q", "k"), optional=("k",))
    for what, over in (("n_pos does not divide ntok", dict(positions=i32(4))), ("n_pos = 0", dict(positions=i32(0))), ("Nq % N", dict(k=z((6, 3, 128), dtype=F16))),
                       ("N = 0", dict(k=z((6, 0, 128), dtype=F16))), ("Nq = 0", dict(q=z((6, 0, 128), dtype=F16))), ("tokens of k", dict(k=z((5, N, 128), dtype=F16))),
                       ("no k, Nq = 0", dict(k=None, q=z((6, 0, 128), dtype=F16))), ("no k, n_pos", dict(k=None, positions=i32(4))),
                       ("cos width", dict(cos=z((ROPE_LEN, 64), dtype=F16))), ("cos against sin", dict(sin=z((ROPE_LEN + 1, 128), dtype=F16))),
                       ("rope_len = 0", dict(cos=z((0, 128), dtype=F16), sin=z((0, 128), dtype=F16))), ("no k (valid)", dict(k=None)),
                       ("one position (valid)", dict(positions=i32(1)))):
        out.append((fn, what, dict(base, **over)))
    out.append((fn, "valid", base))
    for init in (True, False):
        fn = f"kvrope.rope_{'init' if init else 'append'}_kv_quantize_i4"
        ntok = B + 2 if init else B
        q, k, v = sliced(ntok)
        base = dict(q_out=z((ntok, NQ, 128), dtype=F16), q=q, k=k, v=v, cos=z((ROPE_LEN, 128), dtype=F16), sin=z((ROPE_LEN, 128), dtype=F16), **tables())
        if init:
            base["seqlen_indptr"] = i32(B + 1)
        generic(fn, base, rows=("q", "k", "v"))
        cache_faults(fn, base)
        for what, over in (("k and v token strides differ", dict(v=z((ntok, N * 128 + 8), dtype=F16)[:, :N * 128].view(ntok, N, 128))),
                           ("cos width", dict(cos=z((ROPE_LEN, 64), dtype=F16))), ("cos against sin", dict(sin=z((ROPE_LEN + 1, 128), dtype=F16))),
                           ("rope_len = 0", dict(cos=z((0, 128), dtype=F16), sin=z((0, 128), dtype=F16))),
                           ("q_out against q", dict(q_out=z((ntok, N, 128), dtype=F16))), ("k heads", dict(k=z((ntok, N + 1, 128), dtype=F16))),
                           ("k and v heads", dict(k=z((ntok, N + 1, 128), dtype=F16), v=z((ntok, N + 1, 128), dtype=F16))),
                           ("tokens of k and v", dict(k=z((ntok + 1, N, 128), dtype=F16), v=z((ntok + 1, N, 128), dtype=F16))),
                           ("tokens of q and q_out", dict(q=z((ntok + 1, NQ, 128), dtype=F16), q_out=z((ntok + 1, NQ, 128), dtype=F16))),
                           ("Nq % N", dict(q=z((ntok, 3, 128), dtype=F16), q_out=z((ntok, 3, 128), dtype=F16))),
                           ("Nq = 0", dict(q=z((ntok, 0, 128), dtype=F16), q_out=z((ntok, 0, 128), dtype=F16))),
                           ("a 16-bit cache", dict(kv_data=z((PAGES, L, 2, N, P, 128), dtype=F16))),
                           ("contiguous rows (valid)", dict(q=z((ntok, NQ, 128), dtype=F16), k=z((ntok, N, 128), dtype=F16), v=z((ntok, N, 128), dtype=F16)))):
            out.append((fn, what, dict(base, **over)))
        if init:
            out.append((fn, "seqlen_indptr length", dict(base, seqlen_indptr=i32(B))))
        out.append((fn, "valid", base))

    # ---- PagedKVCacheI4: the constructor, and the two table builders of a (CPU) cache
    ctor = dict(batch_size=2, page_size=4, max_seq_len=10, device="cpu", n_layers=1, num_heads=1)
    for what, over in (("head_dim", dict(head_dim=64)), ("batch_size", dict(batch_size=0)), ("page_size", dict(page_size=0)), ("max_seq_len", dict(max_seq_len=0)),
                       ("n_layers", dict(n_layers=0)), ("num_heads", dict(num_heads=-1)), ("head_dim and batch_size", dict(head_dim=64, batch_size=0))):
        out.append(("kvcache.PagedKVCacheI4", what, dict(ctor, **over)))
    for length in (0, 11, -1):
        out.append(("kvcache.PagedKVCacheI4.tables", f"length {length}", dict(ctor=ctor, length=length)))
    for length, n_new in ((5, 0), (5, 6), (11, 1), (0, 0), (11, 12)):
        out.append(("kvcache.PagedKVCacheI4.prefill_tables", f"length {length}, {n_new} new", dict(ctor=ctor, length=length, n_new=n_new)))
    return out


def py_call(fn, kwargs):
    """The str() of the RuntimeError ``fn(**kwargs)`` raises (tests/test_kv_rejections.py has its own copy)."""
    import importlib
    mod, _, attr = fn.partition(".")
    target = importlib.import_module("arcquant_amd." + mod)
    kwargs = {k: dec(v) for k, v in kwargs.items()}
    try:
        if "ctor" in kwargs:
            cls, method = attr.split(".")
            getattr(getattr(target, cls)(**kwargs.pop("ctor")), method)(**kwargs)
        else:
            getattr(target, attr)(**kwargs)
    except RuntimeError as e:
        return str(e)
    raise SystemExit(f"{fn}({kwargs}) was accepted: such a case must not be in the table")


def py_table():
    """Per function: its valid keyword arguments once (``base``; empty where it has none), and per case what it sets differently."""
    by_fn = {}
    for fn, what, kwargs in py_cases():
        by_fn.setdefault(fn, []).append((what, kwargs))
    table, n = [], 0
    for fn, cases in by_fn.items():
        base = next((kw for what, kw in cases if what == "valid"), {})
        rec, seen = dict(fn=fn, base=enc(base), cases=[]), set()
        for what, kw in cases:
            over = enc({k: v for k, v in kw.items() if k not in base or v is not base[k]})
            if json.dumps(over) in seen:
                continue
            seen.add(json.dumps(over))
            error = py_call(fn, dict(rec["base"], **over))
            if ("must live on the GPU" in error) != ("valid" in what):
                raise SystemExit(f"{fn}, {what}: {error!r}: only an unbroken argument set may reach the device check, and it must")
            rec["cases"].append(dict(what=what, over=over, error=error))
        table.append(rec)
        n += len(rec["cases"])

    def dumps(v):
        return json.dumps(v, separators=(",", ":"))
    text = "[\n" + ",\n".join('{"fn":%s,"base":%s,"cases":[\n' % (dumps(r["fn"]), dumps(r["base"])) + ",\n".join(" " + dumps(c) for c in r["cases"]) + "\n]}"
                               for r in table) + "\n]\n"
    return text, f"{n} cases of {len(table)} functions"


def main():
    for name, make in (("cabi_kv_rejections.json", c_table), ("kv_python_rejections.json", py_table)):
        text, what = make()
        with open(os.path.join(HERE, name), "w") as f:
            f.write(text)
        print(f"{name}: {what}, {len(text)} bytes")


if __name__ == "__main__":
    main()
