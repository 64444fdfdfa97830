"""CPU tests of the KV-cache boundary: every public function of arcquant_amd.kvcache rejects a wrong dtype, rank, head dimension,
non-contiguity, Nq % N != 0 and mismatched table lengths with RuntimeError before anything is launched, and refuses CPU tensors LAST;
the C entry points of include/arcq_kv.h return their status codes without a GPU; the header and its binding table agree."""
import inspect
import os
import re

import pytest
import torch

from arcquant_amd import _lib, kvcache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
PAGES, L, N, P, B = 4, 2, 2, 5, 3


def _args(fn, fmt="i4", dtype=F16, nq=N, ntok=7):
    """Valid (CPU) arguments of ``fn`` by keyword."""
    row = 64 if fmt == "i4" else 128
    cache_dtype = U8 if fmt == "i4" else dtype
    a = dict(kv_data=torch.zeros((PAGES, L, 2, N, P, row), dtype=cache_dtype), kv_param=torch.zeros((PAGES, L, 2, N, P, 2), dtype=F16),
             kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
             last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)
    names = list(inspect.signature(fn).parameters)
    quant = "quantize" in fn.__name__
    n = ntok if "seqlen_indptr" in names else B
    if "k" in names:
        a["k"] = torch.zeros((n, N, 128 if quant else row), dtype=dtype if quant else cache_dtype)
        a["v"] = a["k"].clone()
    if "k_param" in names:
        a["k_param"], a["v_param"] = torch.zeros((n, N, 2), dtype=F16), torch.zeros((n, N, 2), dtype=F16)
    if "seqlen_indptr" in names:
        a["seqlen_indptr"] = torch.tensor([0, 1, 5, 7], dtype=I32)
    if "q" in names:
        a["q"], a["o"] = torch.zeros((B, nq, 128), dtype=dtype), torch.zeros((B, nq, 128), dtype=dtype)
    return {k: a[k] for k in names}


FUNCS = {"init_kv_i4": "i4", "append_kv_i4": "i4", "batch_decode_i4": "i4", "init_kv_f16": "f16", "append_kv_f16": "f16", "batch_decode_f16": "f16",
         "append_kv_quantize_i4": "i4", "init_kv_quantize_i4": "i4"}


def test_the_public_surface_is_the_references_plus_the_extensions():
    public = {n for n, f in vars(kvcache).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == kvcache.__name__}
    assert public == set(FUNCS) | {"asym_quantize_and_pack_i4", "unpack_i4_and_asym_dequantize"}
    # the reference's positional order and keyword names (model/kv_cache.py:45-110)
    tables = ["kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_offset"]
    rows = ["k", "v", "k_param", "v_param"]
    for suffix in ("i4", "f16"):
        assert list(inspect.signature(getattr(kvcache, f"init_kv_{suffix}")).parameters) == tables + rows + ["seqlen_indptr", "layer_idx"]
        assert list(inspect.signature(getattr(kvcache, f"append_kv_{suffix}")).parameters) == tables + rows + ["layer_idx"]
        assert list(inspect.signature(getattr(kvcache, f"batch_decode_{suffix}")).parameters) == ["o", "q"] + tables + ["layer_idx"]
    assert list(inspect.signature(kvcache.append_kv_quantize_i4).parameters) == tables + ["k", "v", "layer_idx"]
    assert list(inspect.signature(kvcache.init_kv_quantize_i4).parameters) == tables + ["k", "v", "seqlen_indptr", "layer_idx"]


@pytest.mark.parametrize("name", list(FUNCS))
def test_valid_cpu_arguments_are_refused_last(name):
    """Everything else in order: the only complaint left is where the tensors live."""
    fn = getattr(kvcache, name)
    for dtype in (F16, BF16) if ("quantize" in name or "decode" in name) else (F16,):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn(**_args(fn, FUNCS[name], dtype))
    if "decode" in name:
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            fn(**_args(fn, FUNCS[name], BF16, nq=4 * N))


def _broken(name):
    """(what, mutated keyword arguments, message fragment) for every tensor argument of the function."""
    fn, fmt = getattr(kvcache, name), FUNCS[name]
    out = []
    base = _args(fn, fmt)
    for key, t in base.items():
        if not isinstance(t, torch.Tensor):
            continue
        wrong = dict(base)
        wrong[key] = t.to(torch.float32 if t.dtype is not torch.float32 else torch.float64)
        out.append((f"{key} dtype", wrong, key if key not in ("o",) else "o"))
        wrong = dict(base)
        wrong[key] = t.unsqueeze(0)
        out.append((f"{key} rank", wrong, key))
        if t.dim() >= 2:
            wrong = dict(base)
            wrong[key] = torch.cat([t, t], dim=-1)[..., : t.shape[-1]]
            assert not wrong[key].is_contiguous()
            out.append((f"{key} non-contiguous", wrong, "contiguous"))
    # head dimension
    wrong = dict(base)
    wrong["kv_data"] = torch.zeros(base["kv_data"].shape[:-1] + (base["kv_data"].shape[-1] // 2,), dtype=base["kv_data"].dtype)
    out.append(("head dimension of the cache", wrong, "head dimension 128"))
    for key in ("k", "q"):
        if key in base:
            wrong = dict(base)
            for kk in (("k", "v") if key == "k" else ("q", "o")):
                wrong[kk] = torch.zeros(base[kk].shape[:-1] + (base[kk].shape[-1] // 2,), dtype=base[kk].dtype)
            out.append((f"head dimension of {key}", wrong, "must be"))
    # table lengths
    wrong = dict(base)
    wrong["kv_indptr"] = torch.tensor([0, 1, 2], dtype=I32)
    out.append(("kv_indptr length", wrong, "kv_indptr has"))
    wrong = dict(base)
    wrong["kv_param"] = torch.zeros((PAGES, L, 2, N, P + 1, 2), dtype=F16)
    out.append(("kv_param shape", wrong, "kv_param must be"))
    wrong = dict(base)
    wrong["layer_idx"] = L
    out.append(("layer_idx", wrong, "layer_idx"))
    if "seqlen_indptr" in base:
        wrong = dict(base)
        wrong["seqlen_indptr"] = torch.tensor([0, 1, 5], dtype=I32)
        out.append(("seqlen_indptr length", wrong, "seqlen_indptr has"))
    if "k_param" in base:
        wrong = dict(base)
        wrong["k_param"] = torch.zeros((base["k"].shape[0] + 1, N, 2), dtype=F16)
        out.append(("k_param tokens", wrong, "k_param must be"))
    if "k" in base and "seqlen_indptr" not in base:
        wrong = dict(base)
        wrong["k"], wrong["v"] = torch.cat([base["k"], base["k"]]), torch.cat([base["v"], base["v"]])
        out.append(("one token per sequence", wrong, "k and v must be"))
    if "q" in base:
        wrong = _args(fn, fmt, nq=3)
        out.append(("Nq % N", wrong, "not a multiple"))
        wrong = dict(base)
        wrong["q"], wrong["o"] = torch.zeros((B + 1, N, 128), dtype=F16), torch.zeros((B + 1, N, 128), dtype=F16)
        out.append(("batch of q", wrong, "o and q must be"))
    return out


@pytest.mark.parametrize("name", list(FUNCS))
def test_bad_arguments_raise_runtime_error_before_the_device_check(name):
    fn = getattr(kvcache, name)
    cases = _broken(name)
    assert len(cases) >= 12
    for what, kwargs, fragment in cases:
        with pytest.raises(RuntimeError) as e:
            fn(**kwargs)
        assert "must live on the GPU" not in str(e.value), what          # (the device check comes last: these fail earlier)
        assert fragment in str(e.value), (what, str(e.value))


def test_torch_quantiser_pair():
    x = (torch.randn(3, 2, 128) * 3).to(F16)
    q, s, z = kvcache.asym_quantize_and_pack_i4(x)
    assert q.dtype is U8 and q.shape == (3, 2, 64) and s.shape == z.shape == (3, 2, 1) and s.dtype is F16
    back = kvcache.unpack_i4_and_asym_dequantize(q, s.float(), z.float())
    assert back.shape == x.shape and float((back - x.float()).abs().max()) <= 0.51 * float(s.max()) + 0.02
    with pytest.raises(RuntimeError):
        kvcache.unpack_i4_and_asym_dequantize(q.to(torch.int32), s, z)


def test_paged_cache_builds_the_references_tables():
    c = kvcache.PagedKVCacheI4(batch_size=3, page_size=5, max_seq_len=12, device="cpu", n_layers=2, num_heads=4)
    assert c.pages.shape == (9, 2, 2, 4, 5, 64) and c.pages.dtype is U8 and c.scales.shape == (9, 2, 2, 4, 5, 2) and c.scales.dtype is F16
    t = c.tables(11)
    assert t["kv_indptr"].tolist() == [0, 3, 6, 9] and t["kv_indices"].tolist() == [0, 3, 6, 1, 4, 7, 2, 5, 8] and t["last_page_offset"].tolist() == [1, 1, 1]
    assert c.tables(10)["last_page_offset"].tolist() == [5] * 3 and c.tables(10)["kv_indptr"].tolist() == [0, 2, 4, 6]
    assert c.tables(1)["kv_indices"].tolist() == [0, 1, 2] and all(v.dtype is I32 for k, v in t.items() if k not in ("kv_data", "kv_param"))
    with pytest.raises(RuntimeError):
        c.tables(13)
    with pytest.raises(RuntimeError):
        kvcache.PagedKVCacheI4(1, 16, 16, "cpu", 1, 1, head_dim=64)


# ---- the C-ABI
def _header_symbols(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(arcq_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_table_agree():
    assert _header_symbols("arcq_kv.h") == sorted(_lib.KV_SYMBOLS)
    assert not set(_lib.KV_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.HARNESS_SYMBOLS))
    assert not set(_header_symbols("arcq_kv.h")) & (set(_header_symbols("arcq.h")) | set(_header_symbols("arcq_harness.h")))
    lib = _lib.lib()
    for name in _lib.KV_SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "arcq_kv.h")).read()
    for const, value in (("ARCQ_KV_INT4", _lib.KV_INT4), ("ARCQ_KV_16BIT", _lib.KV_16BIT), ("ARCQ_KV_F16", _lib.KV_F16), ("ARCQ_KV_BF16", _lib.KV_BF16)):
        assert re.search(rf"#define {const} {value}\b", text), const


def test_entry_points_validate_without_a_gpu():
    """Status codes of include/arcq.h: -1 shape, -2 unsupported, -4 NULL, -5 workspace; every check precedes any HIP call, so a fake
    aligned pointer is never dereferenced."""
    lib = _lib.lib()
    X = 4096
    init, app, appq, initq, dec = lib.arcq_kv_init, lib.arcq_kv_append, lib.arcq_kv_append_quantize, lib.arcq_kv_init_quantize, lib.arcq_kv_batch_decode
    # arcq_kv_init(kv_data, kv_param, indptr, indices, last, k, v, kp, vp, seqlen_indptr, ntok, B, L, layer, N, P, format, stream)
    assert init(X, X, X, X, X, X, X, X, X, X, 7, 3, 2, 2, 2, 5, 0, None) == -1 and b"layer_idx" in lib.arcq_last_error()
    assert init(X, X, X, X, X, X, X, X, X, X, 7, 3, 2, 0, 2, 0, 0, None) == -1              # P = 0
    assert init(X, X, X, X, X, X, X, X, X, X, 7, 3, 2, 0, 2, 5, 2, None) == -1 and b"format" in lib.arcq_last_error()
    assert init(X, X, X, X, X, X, X, X, X, X, -1, 3, 2, 0, 2, 5, 0, None) == -1
    assert init(None, None, None, None, None, None, None, None, None, None, 7, 0, 2, 0, 2, 5, 0, None) == 0      # B == 0
    assert init(None, None, None, None, None, None, None, None, None, None, 0, 3, 2, 0, 2, 5, 1, None) == 0      # no tokens
    assert init(X, X, X, X, X, X, X, X, X, None, 7, 3, 2, 0, 2, 5, 0, None) == -4           # seqlen_indptr
    assert init(X, X, X, X, X, X, X, None, X, X, 7, 3, 2, 0, 2, 5, 1, None) == -4           # k_param
    assert init(X + 8, X, X, X, X, X, X, X, X, X, 7, 3, 2, 0, 2, 5, 0, None) == -1 and b"16-byte" in lib.arcq_last_error()
    assert init(X, X + 2, X, X, X, X, X, X, X, X, 7, 3, 2, 0, 2, 5, 0, None) == -1 and b"4-byte" in lib.arcq_last_error()
    # arcq_kv_append(..., kp, vp, B, L, layer, N, P, format, stream)
    assert app(X, X, X, X, X, X, X, X, X, 3, 2, -1, 2, 5, 0, None) == -1
    assert app(X, X, X, X, X, X, X, X, X, 3, 2, 1, 0, 5, 0, None) == -1                      # N = 0
    assert app(None, None, None, None, None, None, None, None, None, 0, 2, 1, 2, 5, 0, None) == 0
    assert app(X, X, X, None, X, X, X, X, X, 3, 2, 1, 2, 5, 1, None) == -4
    assert app(X, X, X, X, X, X + 4, X, X, X, 3, 2, 1, 2, 5, 1, None) == -1
    # arcq_kv_append_quantize(kv_data, kv_param, indptr, indices, last, k, v, B, L, layer, N, P, format, dtype, stream)
    assert appq(X, X, X, X, X, X, X, 3, 2, 1, 2, 5, 0, 2, None) == -1 and b"dtype" in lib.arcq_last_error()
    assert appq(X, X, X, X, X, X, X, 3, 2, 1, 2, 5, 1, 0, None) == -2                        # the quantiser writes int4 caches only
    assert appq(None, None, None, None, None, None, None, 0, 2, 1, 2, 5, 0, 1, None) == 0
    assert appq(X, X, X, X, X, None, X, 3, 2, 1, 2, 5, 0, 1, None) == -4
    assert appq(X, X, X, X, X, X, X + 8, 3, 2, 1, 2, 5, 0, 1, None) == -1
    # arcq_kv_init_quantize(kv_data, kv_param, indptr, indices, last, k, v, seqlen_indptr, ntok, B, L, layer, N, P, format, dtype, stream)
    assert initq(X, X, X, X, X, X, X, X, 7, 3, 0, 0, 2, 5, 0, 0, None) == -1                 # L = 0
    assert initq(X, X, X, X, X, X, X, X, 7, 3, 2, 0, 2, 5, 1, 1, None) == -2
    assert initq(X, X, X, X, X, X, X, None, 7, 3, 2, 0, 2, 5, 0, 1, None) == -4
    assert initq(None, None, None, None, None, None, None, None, 0, 3, 2, 0, 2, 5, 0, 1, None) == 0
    # arcq_kv_batch_decode(o, q, kv_data, kv_param, indptr, indices, last, B, Nq, L, layer, N, P, nnz, format, dtype, ws, ws_bytes, stream)
    assert dec(X, X, X, X, X, X, X, 3, 3, 2, 1, 2, 5, 4, 0, 0, None, 0, None) == -1 and b"multiple" in lib.arcq_last_error()
    assert dec(X, X, X, X, X, X, X, 3, 8, 2, 1, 2, 5, 4, 0, 3, None, 0, None) == -1          # dtype
    assert dec(X, X, X, X, X, X, X, 3, 8, 2, 2, 2, 5, 4, 0, 0, None, 0, None) == -1          # layer
    assert dec(None, None, None, None, None, None, None, 0, 8, 2, 1, 2, 5, 4, 0, 0, None, 0, None) == 0
    assert dec(None, X, X, X, X, X, X, 3, 8, 2, 1, 2, 5, 4, 0, 0, None, 0, None) == -4
    assert dec(X, X, X, None, X, X, X, 3, 8, 2, 1, 2, 5, 4, 0, 0, None, 0, None) == -4       # int4 needs kv_param
    assert dec(X, X + 2, X, X, X, X, X, 3, 8, 2, 1, 2, 5, 4, 0, 0, None, 0, None) == -1 and b"16-byte" in lib.arcq_last_error()
    # the workspace: none for short sequences, required once the sequences are split
    wb = lib.arcq_kv_decode_workspace_bytes
    assert wb(3, 8, 2, 4, 5) == 0 and wb(0, 8, 2, 4, 5) == 0 and wb(3, 3, 2, 4, 5) == 0
    need = wb(2, 4, 1, 113, 16)
    assert need > 0 and need % (2 * 4 * 130 * 4) == 0
    assert dec(X, X, X, X, X, X, X, 2, 4, 2, 1, 1, 16, 113, 0, 0, None, 0, None) == -5
    assert dec(X, X, X, X, X, X, X, 2, 4, 2, 1, 1, 16, 113, 0, 0, X, need - 4, None) == -5 and b"workspace" in lib.arcq_last_error()
