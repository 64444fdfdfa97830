"""CPU tests of the prefill attention's boundary: kvcache.batch_prefill_i4 rejects a wrong dtype, rank, contiguity, a qo_indptr of the wrong
length, mismatched q / o, Nq % N != 0 and a bad layer with RuntimeError before anything is launched, and refuses CPU tensors LAST;
arcq_kv_batch_prefill returns its status codes without a GPU; PagedKVCacheI4.prefill_tables and the harness flag."""
import inspect

import pytest
import torch

from arcquant_amd import _lib, kvcache

F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
PAGES, L, N, P, B = 4, 2, 2, 5, 3


def _args(dtype=F16, nq=N, ntok=7):
    return dict(o=torch.zeros((ntok, nq, 128), dtype=dtype), q=torch.zeros((ntok, nq, 128), dtype=dtype), qo_indptr=torch.tensor([0, 1, 5, 7], dtype=I32),
                kv_data=torch.zeros((PAGES, L, 2, N, P, 64), dtype=U8), kv_param=torch.zeros((PAGES, L, 2, N, P, 2), dtype=F16),
                kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
                last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1)


def test_the_signature():
    assert list(inspect.signature(kvcache.batch_prefill_i4).parameters) == ["o", "q", "qo_indptr", "kv_data", "kv_param", "kv_indptr", "kv_indices",
                                                                            "last_page_offset", "layer_idx"]
    assert "arcq_kv_batch_prefill" in _lib.KV_SYMBOLS and hasattr(_lib.lib(), "arcq_kv_batch_prefill")


def test_valid_cpu_arguments_are_refused_last():
    for kwargs in (_args(F16), _args(BF16), _args(BF16, nq=4 * N), _args(F16, ntok=9)):      # (rows beyond qo_indptr[B] are allowed)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            kvcache.batch_prefill_i4(**kwargs)


def _broken():
    base, out = _args(), []
    for key, t in base.items():
        if not isinstance(t, torch.Tensor):
            continue
        wrong = dict(base)
        wrong[key] = t.to(torch.float32)
        out.append((f"{key} dtype", wrong, key))
        wrong = dict(base)
        wrong[key] = t.unsqueeze(0)
        out.append((f"{key} rank", wrong, key))
        if t.dim() >= 2:
            wrong = dict(base)
            wrong[key] = torch.cat([t, t], dim=-1)[..., : t.shape[-1]]
            assert not wrong[key].is_contiguous()
            out.append((f"{key} non-contiguous", wrong, "contiguous"))
    for n in (B, B + 2):
        wrong = dict(base)
        wrong["qo_indptr"] = torch.zeros(n, dtype=I32)
        out.append((f"qo_indptr of {n} entries", wrong, "qo_indptr has"))
    wrong = dict(base)
    wrong["o"] = torch.zeros((8, N, 128), dtype=F16)
    out.append(("o / q tokens", wrong, "o and q must be"))
    wrong = dict(base)
    wrong["o"] = torch.zeros((7, 2 * N, 128), dtype=F16)
    out.append(("o / q heads", wrong, "o and q must be"))
    wrong = dict(base)
    wrong["q"], wrong["o"] = torch.zeros((7, N, 64), dtype=F16), torch.zeros((7, N, 64), dtype=F16)
    out.append(("head dimension of q", wrong, "o and q must be"))
    out.append(("Nq % N", _args(nq=3), "not a multiple"))
    wrong = dict(base)
    wrong["kv_data"] = torch.zeros((PAGES, L, 2, N, P, 32), dtype=U8)
    out.append(("head dimension of the cache", wrong, "head dimension 128"))
    wrong = dict(base)
    wrong["kv_data"] = torch.zeros((PAGES, L, 2, N, P, 128), dtype=F16)
    out.append(("a 16-bit cache", wrong, "kv_data"))
    wrong = dict(base)
    wrong["kv_indptr"] = torch.tensor([0, 1, 2], dtype=I32)
    out.append(("kv_indptr length", wrong, "kv_indptr has"))
    wrong = dict(base)
    wrong["kv_param"] = torch.zeros((PAGES, L, 2, N, P + 1, 2), dtype=F16)
    out.append(("kv_param shape", wrong, "kv_param must be"))
    for layer in (L, -1):
        wrong = dict(base)
        wrong["layer_idx"] = layer
        out.append((f"layer_idx {layer}", wrong, "layer_idx"))
    return out


def test_bad_arguments_raise_runtime_error_before_the_device_check():
    cases = _broken()
    assert len(cases) >= 30
    for what, kwargs, fragment in cases:
        with pytest.raises(RuntimeError) as e:
            kvcache.batch_prefill_i4(**kwargs)
        assert "must live on the GPU" not in str(e.value), what
        assert fragment in str(e.value), (what, str(e.value))


def test_entry_point_validates_without_a_gpu():
    """Status codes of include/arcq.h: -1 shape, -2 unsupported, -4 NULL; every check precedes any HIP call, so a fake aligned pointer is
    never dereferenced."""
    lib = _lib.lib()
    pf, X = lib.arcq_kv_batch_prefill, 4096
    # (o, q, qo_indptr, kv_data, kv_param, kv_indptr, kv_indices, last, ntok, B, Nq, L, layer, N, P, nnz, format, dtype, stream)
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 3, 2, 1, 2, 5, 4, 0, 0, None) == -1 and b"multiple" in lib.arcq_last_error()
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 2, 2, 5, 4, 0, 0, None) == -1 and b"layer_idx" in lib.arcq_last_error()
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, -1, 2, 5, 4, 0, 0, None) == -1
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 1, 2, 5, 4, 0, 2, None) == -1 and b"dtype" in lib.arcq_last_error()
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 1, 2, 5, 4, 2, 0, None) == -1 and b"format" in lib.arcq_last_error()
    assert pf(X, X, X, X, X, X, X, X, -1, 3, 8, 2, 1, 2, 5, 4, 0, 0, None) == -1 and b"ntok" in lib.arcq_last_error()
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 1, 2, 0, 4, 0, 0, None) == -1              # P = 0
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 1, 2, 5, -1, 0, 0, None) == -1             # nnz
    assert pf(X, X, X, X, X, X, X, X, 7, 3, 8, 2, 1, 2, 5, 4, 1, 0, None) == -2 and b"ARCQ_KV_INT4" in lib.arcq_last_error()      # a 16-bit cache
    assert pf(None, None, None, None, None, None, None, None, 7, 0, 8, 2, 1, 2, 5, 4, 0, 0, None) == 0         # B == 0
    assert pf(None, None, None, None, None, None, None, None, 0, 3, 8, 2, 1, 2, 5, 4, 0, 1, None) == 0         # ntok == 0
    for i in range(8):                                                                       # every pointer: NULL
        ptrs = [X] * 8
        ptrs[i] = None
        assert pf(*ptrs, 7, 3, 8, 2, 1, 2, 5, 4, 0, 0, None) == -4, i
    for i, (off, text) in enumerate([(8, b"16-byte"), (8, b"16-byte"), (2, b"4-byte"), (8, b"16-byte"), (2, b"4-byte"), (2, b"4-byte"), (2, b"4-byte"),
                                     (2, b"4-byte")]):
        ptrs = [X] * 8
        ptrs[i] = X + off
        assert pf(*ptrs, 7, 3, 8, 2, 1, 2, 5, 4, 0, 1, None) == -1 and text in lib.arcq_last_error(), i


def test_prefill_tables():
    c = kvcache.PagedKVCacheI4(batch_size=3, page_size=5, max_seq_len=12, device="cpu", n_layers=2, num_heads=4)
    t = c.prefill_tables(11, 4)
    plain = c.tables(11)
    assert set(t) == set(plain) | {"qo_indptr"} and all(t[k].data_ptr() == plain[k].data_ptr() and t[k].shape == plain[k].shape for k in plain)
    assert t["qo_indptr"].dtype is I32 and t["qo_indptr"].tolist() == [0, 4, 8, 12]
    assert c.prefill_tables(7, 4)["qo_indptr"] is t["qo_indptr"], "built once per n_new"
    assert c.prefill_tables(7, 7)["qo_indptr"].tolist() == [0, 7, 14, 21]
    for length, n_new in ((5, 6), (5, 0), (13, 2)):
        with pytest.raises(RuntimeError):
            c.prefill_tables(length, n_new)


def test_the_harness_flag_needs_the_int4_cache():
    from arcquant_amd import e2e
    cfg = e2e.ModelConfig("toykv", num_layers=1, num_heads=16, hidden_size=2048, intermediate_size=4096, vocab_size=512)
    for kv_cache in ("bf16", None):
        with pytest.raises(ValueError, match="kv_paged_prefill"):
            e2e.DecoderModel(cfg, 1, 16, "cpu", fused=True, attention="cache", kv_paged_prefill=True, **({"kv_cache": kv_cache} if kv_cache else {}))
    assert "kv_paged_prefill" in inspect.signature(e2e.bench_decode).parameters and "kv_paged_prefill" in inspect.signature(e2e.bench_protocol).parameters
