"""CPU tests of the GQA decode boundary (kvcache.batch_decode_gqa_i4, include/arcq_kv.h arcq_kv_batch_decode_gqa): every refusal happens
before a launch, so stand-in addresses are never dereferenced and CPU tensors get as far as the device check.  A mistake the other KV entry
points know is reported with their status and their words."""
import pytest
import torch

from arcquant_amd import _lib, kvcache

F16, U8, I32 = torch.float16, torch.uint8, torch.int32
X = 4096          # an aligned stand-in address
#        B, Nq, L, layer, N, P, nnz, format, dtype
GOOD = (3, 8, 2, 1, 2, 5, 4, 0, 0)


def _call(name, shape, ws=None, ws_bytes=0, ptr=X):
    lib = _lib.lib()
    st = getattr(lib, name)(ptr, X, X, X, X, X, X, *shape, ws, ws_bytes, None)
    return st, lib.arcq_last_error().decode().replace(name, "<fn>")


@pytest.mark.parametrize("what,shape,ptr", [
    ("Nq % N", (3, 7, 2, 1, 2, 5, 4, 0, 0), X), ("dtype", (3, 8, 2, 1, 2, 5, 4, 0, 3), X), ("layer", (3, 8, 2, 2, 2, 5, 4, 0, 0), X),
    ("format", (3, 8, 2, 1, 2, 5, 4, 2, 0), X), ("pages", (3, 8, 2, 1, 2, 5, -1, 0, 0), X), ("NULL o", GOOD, None), ("misaligned o", GOOD, X + 2)])
def test_shared_mistakes_are_reported_as_batch_decode_reports_them(what, shape, ptr):
    want = _call("arcq_kv_batch_decode", shape, ptr=ptr)
    assert want[0] < 0 and _call("arcq_kv_batch_decode_gqa", shape, ptr=ptr) == want


def test_what_only_this_kernel_refuses():
    st, err = _call("arcq_kv_batch_decode_gqa", (3, 34, 2, 1, 2, 5, 4, 0, 0))                 # g = 17
    assert st == -2 and "17 query heads per kv head, at most 16" in err
    assert _call("arcq_kv_batch_decode_gqa", (3, 32, 2, 1, 2, 5, 4, 0, 0), ptr=None)[0] == -4   # g = 16 gets as far as the pointers
    # a 16-bit cache: the status and the words of the other int4-only entry points
    st, err = _call("arcq_kv_batch_decode_gqa", GOOD[:7] + (1, 0))
    assert st == -2 and err.endswith("ARCQ_KV_INT4 caches only")
    assert _call("arcq_kv_batch_decode_gqa", (0,) + GOOD[1:], ptr=None)[0] == 0                  # B == 0: nothing to do


def test_the_workspace_is_this_kernels_own():
    wb = _lib.lib().arcq_kv_decode_gqa_workspace_bytes
    assert wb(3, 8, 2, 4, 5) == 0 and wb(0, 8, 2, 4, 5) == 0 and wb(3, 3, 2, 4, 5) == 0
    split = (2, 4, 2, 1, 1, 16, 113, 0, 0)
    need = wb(2, 4, 1, 113, 16)
    assert need > 0 and need % (2 * 4 * 130 * 4) == 0
    assert _call("arcq_kv_batch_decode_gqa", split)[0] == -5
    st, err = _call("arcq_kv_batch_decode_gqa", split, X, need - 4)
    assert st == -5 and err == f"<fn>: workspace of {need - 4} bytes, need {need} (arcq_kv_decode_gqa_workspace_bytes)"
    # one slice is B * N workgroups whatever g is: the answer per query head does not depend on g (batch_decode's does, through its chunks)
    assert wb(2, 16, 1, 2000, 16) == 4 * wb(2, 4, 1, 2000, 16)


def _args(nq=8, dtype=F16, cache=U8):
    pages, L, N, P = 4, 2, 2, 5
    return dict(o=torch.zeros((3, nq, 128), dtype=dtype), q=torch.zeros((3, nq, 128), dtype=dtype),
                kv_data=torch.zeros((pages, L, 2, N, P, 64 if cache is U8 else 128), dtype=cache), kv_param=torch.zeros((pages, L, 2, N, P, 2), dtype=F16),
                kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
                last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)


@pytest.mark.parametrize("what,change", [
    ("valid", {}), ("g = 16", dict(_args(32))), ("g = 17", dict(_args(34))), ("Nq % N", dict(_args(7))), ("16-bit cache", dict(_args(cache=F16))),
    ("q dtype", dict(q=torch.zeros((3, 8, 128)))), ("o dtype", dict(o=torch.zeros((3, 8, 128), dtype=torch.bfloat16))),
    ("q rank", dict(q=torch.zeros((3, 8, 128, 1), dtype=F16))), ("o rank", dict(o=torch.zeros((24, 128), dtype=F16)))])
def test_python_refusals_are_batch_decodes(what, change):
    """The message batch_decode_i4 gives for the same arguments, under this function's name; g = 17 is this function's own; an unbroken
    set is refused last, for where it lives."""
    kwargs = dict(_args(), **change)
    with pytest.raises(RuntimeError) as e:
        kvcache.batch_decode_gqa_i4(**kwargs)
    if what == "g = 17":
        assert "17 query heads per kv head, at most 16" in str(e.value)
        return
    assert ("must live on the GPU" in str(e.value)) == (what in ("valid", "g = 16"))
    with pytest.raises(RuntimeError) as ref:
        kvcache.batch_decode_i4(**kwargs)
    assert str(e.value) == str(ref.value).replace("batch_decode_i4", "batch_decode_gqa_i4")
