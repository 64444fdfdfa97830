"""CPU tests of the 16-bit prefill attention's boundary: kvcache.batch_prefill_f16 raises RuntimeError for bad arguments before anything is
launched and refuses CPU tensors LAST; arcq_kv_batch_prefill_16bit returns its status codes without a GPU."""
import inspect

import pytest
import torch

from arcquant_amd import _lib, kvcache, kvprefill

F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
PAGES, L, N, P, B = 4, 2, 2, 5, 3


def _args(dtype=F16, nq=N, ntok=7):
    return dict(o=torch.zeros((ntok, nq, 128), dtype=dtype), q=torch.zeros((ntok, nq, 128), dtype=dtype), qo_indptr=torch.tensor([0, 1, 5, 7], dtype=I32),
                kv_data=torch.zeros((PAGES, L, 2, N, P, 128), dtype=dtype), kv_param=torch.zeros((PAGES, L, 2, N, P, 2), dtype=F16),
                kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
                last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)


def test_the_signature_and_where_it_lives():
    assert list(inspect.signature(kvcache.batch_prefill_f16).parameters) == ["o", "q", "qo_indptr", "kv_data", "kv_param", "kv_indptr", "kv_indices",
                                                                             "last_page_offset", "layer_idx"]
    assert kvcache.batch_prefill_f16 is kvprefill.batch_prefill_f16 and kvprefill.batch_prefill_f16.__module__ == kvprefill.__name__
    assert "arcq_kv_batch_prefill_16bit" in _lib.KV_SYMBOLS and hasattr(_lib.lib(), "arcq_kv_batch_prefill_16bit")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_valid_cpu_arguments_are_refused_last(dtype):
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        kvcache.batch_prefill_f16(**_args(dtype, nq=4 * N))


def _broken():
    out = []
    for key, t in _args().items():
        if isinstance(t, torch.Tensor):
            out += [(f"{key} dtype", {key: t.to(torch.float32)}, key), (f"{key} rank", {key: t.unsqueeze(0)}, key)]
            if t.dim() >= 2:
                out.append((f"{key} non-contiguous", {key: torch.cat([t, t], dim=-1)[..., : t.shape[-1]]}, "contiguous"))
    out += [(f"qo_indptr of {n} entries", {"qo_indptr": torch.zeros(n, dtype=I32)}, "qo_indptr has") for n in (B, B + 2)]
    out.append(("head dimension of q", {"q": torch.zeros((7, N, 64), dtype=F16), "o": torch.zeros((7, N, 64), dtype=F16)}, "o and q must be"))
    out.append(("Nq % N", {"q": torch.zeros((7, 3, 128), dtype=F16), "o": torch.zeros((7, 3, 128), dtype=F16)}, "not a multiple"))
    out.append(("an int4 cache", {"kv_data": torch.zeros((PAGES, L, 2, N, P, 64), dtype=U8)}, "kv_data"))
    out.append(("a cache of another dtype than q's", {"kv_data": torch.zeros((PAGES, L, 2, N, P, 128), dtype=BF16)}, "kv_data"))
    out += [(f"layer_idx {layer}", {"layer_idx": layer}, "layer_idx") for layer in (L, -1)]
    return [pytest.param(over, fragment, id=what) for what, over, fragment in out]


@pytest.mark.parametrize("over,fragment", _broken())
def test_bad_arguments_raise_runtime_error_before_the_device_check(over, fragment):
    with pytest.raises(RuntimeError) as e:
        kvcache.batch_prefill_f16(**dict(_args(), **over))
    assert "must live on the GPU" not in str(e.value) and fragment in str(e.value)


def test_entry_point_validates_without_a_gpu():
    """-1 shape, -4 NULL (include/arcq.h); every check precedes any HIP call, so a stand-in pointer is never dereferenced."""
    lib = _lib.lib()
    pf, X, err = lib.arcq_kv_batch_prefill_16bit, 4096, lib.arcq_last_error
    # (o, q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last, ntok, B, Nq, L, layer, N, P, nnz, dtype, stream)
    for sizes, text in (((7, 3, 3, 2, 1, 2, 5, 4, 0), b"multiple"), ((7, 3, 8, 2, 2, 2, 5, 4, 0), b"layer_idx"), ((7, 3, 8, 2, 1, 2, 5, 4, 2), b"dtype"),
                        ((-1, 3, 8, 2, 1, 2, 5, 4, 0), b"ntok"), ((7, 3, 8, 2, 1, 2, 0, 4, 0), b"P >= 1")):
        assert pf(*[X] * 8, *sizes, None) == -1 and text in err(), sizes
    assert pf(*[None] * 8, 7, 0, 8, 2, 1, 2, 5, 4, 0, None) == 0 and pf(*[None] * 8, 0, 3, 8, 2, 1, 2, 5, 4, 1, None) == 0      # B == 0; ntok == 0
    for i, (off, text) in enumerate([(8, b"16-byte"), (8, b"16-byte"), (2, b"4-byte"), (8, b"16-byte"), (2, b"4-byte"), (2, b"4-byte"), (2, b"4-byte"),
                                     (2, b"4-byte")]):
        ptrs = [X] * 8
        ptrs[i] = X + off
        assert pf(*ptrs, 7, 3, 8, 2, 1, 2, 5, 4, 1, None) == -1 and text in err(), i
        ptrs[i] = None                                                                    # every pointer but kv_param: NULL
        assert i == 4 or pf(*ptrs, 7, 3, 8, 2, 1, 2, 5, 4, 0, None) == -4, i
