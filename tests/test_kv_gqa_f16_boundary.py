"""CPU tests of the 16-bit GQA decode boundary (kvcache.batch_decode_gqa_f16, include/arcq_kv.h arcq_kv_batch_decode_gqa_16bit): every
refusal happens before a launch, so stand-in addresses are never dereferenced and CPU tensors get as far as the device check.  A mistake
arcq_kv_batch_decode_gqa knows is reported with its status and its words."""
import pytest
import torch

from arcquant_amd import _lib, kvcache

F16, U8, I32 = torch.float16, torch.uint8, torch.int32
X = 4096          # an aligned stand-in address
NAME = "arcq_kv_batch_decode_gqa_16bit"
#        B, Nq, L, layer, N, P, nnz, dtype
GOOD = (3, 8, 2, 1, 2, 5, 4, 0)


def _call(shape, ws=None, ws_bytes=0, o=X, param=X, name=NAME):
    """``shape`` is this entry point's; arcq_kv_batch_decode_gqa gets it with format ARCQ_KV_INT4 in its place."""
    lib = _lib.lib()
    if name != NAME:
        shape = shape[:7] + (0,) + shape[7:]
    st = getattr(lib, name)(o, X, X, param, X, X, X, *shape, ws, ws_bytes, None)
    return st, lib.arcq_last_error().decode().replace(name, "<fn>")


def test_the_symbol_is_bound():
    assert NAME in _lib.KV_SYMBOLS and hasattr(_lib.lib(), NAME)


@pytest.mark.parametrize("what,shape,o", [
    ("Nq % N", (3, 7, 2, 1, 2, 5, 4, 0), X), ("dtype", (3, 8, 2, 1, 2, 5, 4, 3), X), ("layer", (3, 8, 2, 2, 2, 5, 4, 0), X),
    ("pages", (3, 8, 2, 1, 2, 5, -1, 0), X), ("NULL o", GOOD, None), ("misaligned o", GOOD, X + 2)])
def test_shared_mistakes_are_reported_as_the_int4_entry_point_reports_them(what, shape, o):
    want = _call(shape, o=o, name="arcq_kv_batch_decode_gqa")
    assert want[0] < 0 and _call(shape, o=o) == want


def test_what_only_this_kernel_refuses_or_allows():
    st, err = _call((3, 34, 2, 1, 2, 5, 4, 0))                           # g = 17
    assert st == -2 and "17 query heads per kv head, at most 16" in err
    assert _call((3, 32, 2, 1, 2, 5, 4, 0), o=None)[0] == -4             # g = 16 gets as far as the pointers
    assert _call((0,) + GOOD[1:], o=None)[0] == 0                        # B == 0: nothing to do
    # kv_param is never read: NULL goes on to the next check (alignment, here the workspace's), a misaligned one stops there
    split, need = (2, 4, 2, 1, 1, 16, 113, 0), _lib.lib().arcq_kv_decode_gqa_workspace_bytes(2, 4, 1, 113, 16)
    assert need > 0
    st, err = _call(split, X, need - 4, param=None)
    assert st == -5 and err == f"<fn>: workspace of {need - 4} bytes, need {need} (arcq_kv_decode_gqa_workspace_bytes)"
    assert _call(split, param=None)[0] == -5
    st, err = _call(split, X, need, param=X + 2)
    assert st == -1 and "4-byte aligned" in err


def _args(nq=8, dtype=F16, cache=F16):
    pages, L, N, P = 4, 2, 2, 5
    return dict(o=torch.zeros((3, nq, 128), dtype=dtype), q=torch.zeros((3, nq, 128), dtype=dtype),
                kv_data=torch.zeros((pages, L, 2, N, P, 64 if cache is U8 else 128), dtype=cache), kv_param=torch.zeros((pages, L, 2, N, P, 2), dtype=F16),
                kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
                last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)


@pytest.mark.parametrize("what,change", [
    ("valid", {}), ("g = 16", dict(_args(32))), ("g = 17", dict(_args(34))), ("Nq % N", dict(_args(7))), ("int4 cache", dict(_args(cache=U8))),
    ("cache dtype", dict(_args(cache=torch.bfloat16))), ("q dtype", dict(q=torch.zeros((3, 8, 128)))),
    ("o dtype", dict(o=torch.zeros((3, 8, 128), dtype=torch.bfloat16))), ("q rank", dict(q=torch.zeros((3, 8, 128, 1), dtype=F16))),
    ("o rank", dict(o=torch.zeros((24, 128), dtype=F16)))])
def test_python_refusals_are_batch_decode_f16s(what, change):
    """The message batch_decode_f16 gives for the same arguments, under this function's name; g = 17 is this function's own; an unbroken
    set is refused last, for where it lives."""
    kwargs = dict(_args(), **change)
    with pytest.raises(RuntimeError) as e:
        kvcache.batch_decode_gqa_f16(**kwargs)
    if what == "g = 17":
        assert "17 query heads per kv head, at most 16" in str(e.value)
        return
    assert ("must live on the GPU" in str(e.value)) == (what in ("valid", "g = 16"))
    with pytest.raises(RuntimeError) as ref:
        kvcache.batch_decode_f16(**kwargs)
    assert str(e.value) == str(ref.value).replace("batch_decode_f16", "batch_decode_gqa_f16")
