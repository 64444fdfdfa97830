"""CPU tests of the FP8 paged KV cache's boundary (arcquant_amd/kvfp8.py re-exported from kvcache; include/arcq_kv.h
arcq_kv_fp8_append_quantize, arcq_kv_fp8_init_quantize, arcq_kv_batch_decode_gqa_fp8): signatures, the torch quantiser's rule, and
refusals that all happen before a launch -- stand-in addresses are never dereferenced, CPU tensors get as far as the device check."""
import inspect

import pytest
import torch

from arcquant_amd import _lib, kvcache, kvfp8

F16, BF16, I32, FP8 = torch.float16, torch.bfloat16, torch.int32, torch.float8_e4m3fn
X = 4096          # an aligned stand-in address
TABLES = ["kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_offset"]
SYMBOLS = ("arcq_kv_fp8_append_quantize", "arcq_kv_fp8_init_quantize", "arcq_kv_batch_decode_gqa_fp8")
FUNCS = ("append_kv_quantize_fp8", "init_kv_quantize_fp8", "batch_decode_gqa_fp8")


def test_signatures_and_symbols():
    assert list(inspect.signature(kvcache.append_kv_quantize_fp8).parameters) == TABLES + ["k", "v", "layer_idx"]
    assert list(inspect.signature(kvcache.init_kv_quantize_fp8).parameters) == TABLES + ["k", "v", "seqlen_indptr", "layer_idx"]
    assert list(inspect.signature(kvcache.batch_decode_gqa_fp8).parameters) == ["o", "q"] + TABLES + ["layer_idx"]
    assert list(inspect.signature(kvcache.quantize_fp8).parameters) == ["x"]
    for name in FUNCS + ("quantize_fp8",):
        assert getattr(kvcache, name) is getattr(kvfp8, name)
    for sym in SYMBOLS:
        assert sym in _lib.KV_SYMBOLS and hasattr(_lib.lib(), sym)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_quantize_fp8_is_within_half_an_e4m3_ulp(dtype):
    """3 mantissa bits: half an ulp of a normal code is 2^-4 |x|; the subnormal step of the codes is 2^-9, half of it scale 2^-10."""
    x = (torch.randn(8, 128, generator=torch.Generator().manual_seed(8)) * 3).to(dtype)
    x[1] = 0
    x[2, 5] = 65504.0                                              # amax = fp16's largest: the largest scale
    x[3] = (torch.arange(128) - 64).to(dtype) * 2.0 ** -20          # tiny values: the scale's floor
    code, scale = kvcache.quantize_fp8(x)
    assert code.dtype is FP8 and code.shape == x.shape and scale.dtype is F16 and scale.shape == (8, 1)
    c, s = code.float(), scale.float()
    assert torch.isfinite(c).all() and (c.abs() <= 448).all() and (s >= 2.0 ** -14).all() and torch.isfinite(s).all()
    assert ((c * s - x.float()).abs() <= 2.0 ** -4 * x.float().abs() + s * 2.0 ** -10).all()
    with pytest.raises(RuntimeError, match=r"^kvcache\.quantize_fp8:"):
        kvcache.quantize_fp8(x.float())


def _args(name, nq=8, cache=FP8, row=128, dtype=F16):
    pages, L, N, P = 4, 2, 2, 5
    a = dict(kv_data=torch.zeros((pages, L, 2, N, P, row), dtype=cache),
             kv_param=torch.zeros((pages, L, 2, N, P, 2), dtype=F16), kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32),
             kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32), last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)
    if name == "batch_decode_gqa_fp8":
        return dict(a, o=torch.zeros((3, nq, 128), dtype=dtype), q=torch.zeros((3, nq, 128), dtype=dtype))
    ntok = 7 if name.startswith("init") else 3
    a.update(k=torch.zeros((ntok, N, 128), dtype=dtype), v=torch.zeros((ntok, N, 128), dtype=dtype))
    if name.startswith("init"):
        a["seqlen_indptr"] = torch.tensor([0, 1, 5, 7], dtype=I32)
    return a


def _broken(name, what):
    a = _args(name)
    row = "q" if name == "batch_decode_gqa_fp8" else "k"
    if what == "cache dtype":
        return _args(name, cache=torch.uint8)
    if what == "16-bit cache":
        return _args(name, cache=F16)
    if what == "last dimension 64":
        return _args(name, row=64)
    if what == "rank":
        return dict(a, **{row: a[row].reshape(-1, 128)})
    if what == "non-contiguous":
        return dict(a, kv_param=torch.zeros((4, 2, 2, 2, 5, 4), dtype=F16)[..., ::2])
    if what == "table length":
        return dict(a, kv_indptr=torch.tensor([0, 1, 2], dtype=I32))
    if what == "Nq % N":
        return _args(name, nq=7)
    if what == "g = 17":
        return _args(name, nq=34)
    if what == "row dtype":
        return dict(a, **{row: a[row].float()})
    assert what in ("valid", "g = 16")
    return _args(name, nq=32) if what == "g = 16" else a


SHARED = ["cache dtype", "16-bit cache", "last dimension 64", "rank", "non-contiguous", "table length", "row dtype", "valid"]
CASES = [(n, w) for n in FUNCS for w in SHARED] + [("batch_decode_gqa_fp8", w) for w in ("Nq % N", "g = 17", "g = 16")]


@pytest.mark.parametrize("name,what", CASES)
def test_python_refusals(name, what):
    """One thing broken: a RuntimeError under the function's name that is not about where the tensors live; an unbroken set is refused
    last, for exactly that."""
    with pytest.raises(RuntimeError) as e:
        getattr(kvcache, name)(**_broken(name, what))
    assert str(e.value).startswith(f"kvcache.{name}:")
    assert ("must live on the GPU" in str(e.value)) == (what in ("valid", "g = 16"))
    if what == "g = 17":
        assert "17 query heads per kv head, at most 16" in str(e.value)


#        B, Nq, L, layer, N, P, nnz, dtype
GOOD = (3, 8, 2, 1, 2, 5, 4, 0)


def _decode(shape, ws=None, ws_bytes=0, o=X, param=X):
    lib = _lib.lib()
    st = lib.arcq_kv_batch_decode_gqa_fp8(o, X, X, param, X, X, X, *shape, ws, ws_bytes, None)
    return st, lib.arcq_last_error().decode()


def test_c_decode_entry_point_validates_without_a_gpu():
    """test_kv_gqa_f16_boundary.py's probes: -1 shape, -2 unsupported, -4 NULL, -5 workspace, 0 for an empty batch.  Unlike the 16-bit
    entry point this one reads kv_param: NULL is refused."""
    for shape in ((3, 7, 2, 1, 2, 5, 4, 0), (3, 8, 2, 1, 2, 5, 4, 3), (3, 8, 2, 2, 2, 5, 4, 0), (3, 8, 2, 1, 2, 5, -1, 0)):
        assert _decode(shape)[0] == -1, shape                             # Nq % N, dtype, layer, pages
    assert _decode(GOOD, o=None)[0] == -4 and _decode(GOOD, param=None)[0] == -4
    st, err = _decode(GOOD, o=X + 2)
    assert st == -1 and "16-byte aligned" in err
    st, err = _decode((3, 34, 2, 1, 2, 5, 4, 0))                          # g = 17
    assert st == -2 and "17 query heads per kv head, at most 16" in err
    assert _decode((3, 32, 2, 1, 2, 5, 4, 0), o=None)[0] == -4            # g = 16 gets as far as the pointers
    assert _decode((0,) + GOOD[1:], o=None)[0] == 0                       # B == 0: nothing to do
    split, need = (2, 4, 2, 1, 1, 16, 113, 0), _lib.lib().arcq_kv_decode_gqa_workspace_bytes(2, 4, 1, 113, 16)
    assert need > 0
    st, err = _decode(split, X, need - 4)
    assert st == -5 and f"workspace of {need - 4} bytes, need {need} (arcq_kv_decode_gqa_workspace_bytes)" in err
    st, err = _decode(split, X, need, param=X + 2)
    assert st == -1 and "4-byte aligned" in err


def test_c_writer_entry_points_validate_without_a_gpu():
    """arcq_kv_append_quantize's / arcq_kv_init_quantize's checks in their order, without a format."""
    lib = _lib.lib()
    app, init = lib.arcq_kv_fp8_append_quantize, lib.arcq_kv_fp8_init_quantize
    # (kv_data, kv_param, indptr, indices, last, k, v, B, L, layer, N, P, dtype, stream)
    assert app(X, X, X, X, X, X, X, 3, 2, 1, 2, 5, 2, None) == -1 and b"dtype" in lib.arcq_last_error()
    assert app(X, X, X, X, X, X, X, 3, 2, 2, 2, 5, 0, None) == -1 and b"layer_idx" in lib.arcq_last_error()
    assert app(None, None, None, None, None, None, None, 0, 2, 1, 2, 5, 1, None) == 0
    assert app(X, None, X, X, X, X, X, 3, 2, 1, 2, 5, 0, None) == -4
    assert app(X, X, X, X, X, X + 8, X, 3, 2, 1, 2, 5, 0, None) == -1 and b"16-byte" in lib.arcq_last_error()
    assert app(X, X + 2, X, X, X, X, X, 3, 2, 1, 2, 5, 0, None) == -1 and b"4-byte" in lib.arcq_last_error()
    # (kv_data, kv_param, indptr, indices, last, k, v, seqlen_indptr, ntok, B, L, layer, N, P, dtype, stream)
    assert init(X, X, X, X, X, X, X, X, -1, 3, 2, 1, 2, 5, 0, None) == -1 and b"ntok" in lib.arcq_last_error()
    assert init(X, X, X, X, X, X, X, X, 7, 3, 2, 1, 0, 5, 0, None) == -1                      # N = 0
    assert init(None, None, None, None, None, None, None, None, 0, 3, 2, 1, 2, 5, 0, None) == 0   # no tokens
    assert init(None, None, None, None, None, None, None, None, 7, 0, 2, 1, 2, 5, 0, None) == 0   # B == 0
    assert init(X, X, X, X, X, X, X, None, 7, 3, 2, 1, 2, 5, 0, None) == -4                    # seqlen_indptr
    assert init(X + 8, X, X, X, X, X, X, X, 7, 3, 2, 1, 2, 5, 0, None) == -1 and b"16-byte" in lib.arcq_last_error()
