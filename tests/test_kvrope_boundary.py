"""CPU tests of the RoPE boundary (arcquant_amd.kvrope, include/arcq_kv.h arcq_rope_qk / arcq_kv_rope_append_quantize /
arcq_kv_rope_init_quantize): signatures and symbols; a wrong dtype, rank, layout, stride, table shape, n_pos or Nq % N raises RuntimeError
before anything is launched and CPU tensors are refused LAST; the C entry points return their status codes without a GPU (fake aligned
pointers are never dereferenced: every check precedes the first HIP call); ``DecoderModel`` takes ``rope`` and refuses malformed tables."""
import ctypes
import inspect

import pytest
import torch

from arcquant_amd import _lib, e2e, kvcache, kvrope

F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
PAGES, L, N, P, B, ROPE_LEN = 4, 2, 2, 5, 3, 16


def test_signatures_and_symbols():
    def names(fn):
        return list(inspect.signature(fn).parameters)
    assert names(kvrope.rope_tables) == ["rope_len", "theta", "dtype", "device"]
    assert names(kvrope.rope_qk_) == ["q", "k", "positions", "cos", "sin"]
    tail = ["q_out", "q", "k", "v", "cos", "sin", "kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_offset"]
    assert names(kvrope.rope_append_kv_quantize_i4) == tail + ["layer_idx"]
    assert names(kvrope.rope_init_kv_quantize_i4) == tail + ["seqlen_indptr", "layer_idx"]
    for name in ("rope_tables", "rope_qk_", "rope_append_kv_quantize_i4", "rope_init_kv_quantize_i4"):
        assert getattr(kvcache, name) is getattr(kvrope, name), name           # re-exported, as batch_prefill_i4 is
    lib = _lib.lib()
    for sym, nargs in (("arcq_rope_qk", 14), ("arcq_kv_rope_append_quantize", 23), ("arcq_kv_rope_init_quantize", 25)):
        assert sym in _lib.KV_SYMBOLS and len(_lib.KV_SYMBOLS[sym][1]) == nargs and _lib.KV_SYMBOLS[sym][0] is ctypes.c_int
        assert getattr(lib, sym) is not None


def _args(dtype=F16, nq=N, sliced=False, init=False):
    """Valid (CPU) keyword arguments of the two writers; sliced: q, k, v are views of one [tokens, (nq + 2 N) * 128] buffer."""
    ntok = B + 2 if init else B
    a = dict(kv_data=torch.zeros((PAGES, L, 2, N, P, 64), dtype=U8), kv_param=torch.zeros((PAGES, L, 2, N, P, 2), dtype=F16),
             kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
             last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1, q_out=torch.zeros((ntok, nq, 128), dtype=dtype),
             cos=torch.ones((ROPE_LEN, 128), dtype=dtype), sin=torch.zeros((ROPE_LEN, 128), dtype=dtype))
    if sliced:
        a["q"], a["k"], a["v"] = torch.zeros((ntok, nq + 2 * N, 128), dtype=dtype).split([nq, N, N], dim=1)
        assert not a["q"].is_contiguous() and not a["k"].is_contiguous()
    else:
        a["q"], a["k"], a["v"] = torch.zeros((ntok, nq, 128), dtype=dtype), torch.zeros((ntok, N, 128), dtype=dtype), torch.zeros((ntok, N, 128), dtype=dtype)
    if init:
        a["seqlen_indptr"] = torch.tensor([0, 1, 3, 5], dtype=I32)
    return a


def _qk_args(dtype=F16, nq=2 * N, ntok=6, n_pos=3, sliced=False):
    a = dict(positions=torch.arange(n_pos, dtype=I32), cos=torch.ones((ROPE_LEN, 128), dtype=dtype), sin=torch.zeros((ROPE_LEN, 128), dtype=dtype))
    if sliced:
        a["q"], a["k"], _ = torch.zeros((ntok, nq + 2 * N, 128), dtype=dtype).split([nq, N, N], dim=1)
    else:
        a["q"], a["k"] = torch.zeros((ntok, nq, 128), dtype=dtype), torch.zeros((ntok, N, 128), dtype=dtype)
    return a


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("sliced", [False, True])
def test_valid_cpu_arguments_are_refused_last(dtype, sliced):
    for nq in (N, 4 * N):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            kvrope.rope_append_kv_quantize_i4(**_args(dtype, nq, sliced))
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            kvrope.rope_init_kv_quantize_i4(**_args(dtype, nq, sliced, init=True))
    for n_pos in (6, 3, 1):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            kvrope.rope_qk_(**_qk_args(dtype, n_pos=n_pos, sliced=sliced))
    a = _qk_args(dtype, sliced=sliced)
    a["k"] = None
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        kvrope.rope_qk_(**a)


def _broken_writes(init):
    base, out = _args(init=init), []
    for key, t in base.items():
        if not isinstance(t, torch.Tensor):
            continue
        wrong = dict(base)
        wrong[key] = t.to(torch.float32)
        out.append((f"{key} dtype", wrong, key))
        wrong = dict(base)
        wrong[key] = t.unsqueeze(0)
        out.append((f"{key} rank", wrong, key))
    for key in ("q_out", "kv_data", "kv_param", "cos", "sin"):          # these stay contiguous
        wrong = dict(base)
        wrong[key] = torch.cat([base[key], base[key]], dim=-1)[..., : base[key].shape[-1]]
        out.append((f"{key} non-contiguous", wrong, "contiguous"))
    for key in ("q", "k", "v"):
        t = base[key]
        wrong = dict(base)
        wrong[key] = torch.zeros((t.shape[0], 2 * t.shape[1], 128), dtype=t.dtype)[:, ::2]               # heads 256 apart
        out.append((f"{key} head stride", wrong, "contiguous heads"))
        wrong = dict(base)
        wrong[key] = torch.zeros((t.shape[0], t.shape[1] * 128 + 4), dtype=t.dtype)[:, :t.shape[1] * 128].view(t.shape[0], t.shape[1], 128)
        out.append((f"{key} token stride not a multiple of 8", wrong, "multiple of 8"))
        wrong = dict(base)
        wrong[key] = torch.zeros(t.shape[:-1] + (64,), dtype=t.dtype)
        out.append((f"{key} head dimension", wrong, "contiguous heads"))
    ntok = base["q"].shape[0]
    wrong = dict(base)
    wrong["v"] = torch.zeros((ntok, N * 128 + 8), dtype=F16)[:, :N * 128].view(ntok, N, 128)
    out.append(("k and v token strides differ", wrong, "one token stride"))
    wrong = dict(base)
    wrong["cos"] = torch.ones((ROPE_LEN, 64), dtype=F16)
    out.append(("cos width", wrong, "cos and sin must be"))
    wrong = dict(base)
    wrong["sin"] = torch.zeros((ROPE_LEN + 1, 128), dtype=F16)
    out.append(("cos against sin", wrong, "cos and sin must be"))
    wrong = dict(base)
    wrong["cos"], wrong["sin"] = torch.ones((0, 128), dtype=F16), torch.zeros((0, 128), dtype=F16)
    out.append(("rope_len < 1", wrong, "rope_len >= 1"))
    wrong = dict(base)
    wrong["kv_data"] = torch.zeros((PAGES, L, 2, N, P, 32), dtype=U8)
    out.append(("head dimension of the cache", wrong, "head dimension 128"))
    wrong = dict(base)
    wrong["kv_indptr"] = torch.tensor([0, 1, 2], dtype=I32)
    out.append(("kv_indptr length", wrong, "kv_indptr has"))
    wrong = dict(base)
    wrong["layer_idx"] = L
    out.append(("layer_idx", wrong, "layer_idx"))
    out.append(("Nq % N", _args(nq=3, init=init), "not a multiple"))
    wrong = dict(base)
    wrong["q_out"] = torch.zeros((ntok, 2 * N, 128), dtype=F16)
    out.append(("q_out against q", wrong, "q_out and q must be"))
    wrong = dict(base)
    wrong["k"], wrong["v"] = torch.zeros((ntok, N + 1, 128), dtype=F16), torch.zeros((ntok, N + 1, 128), dtype=F16)
    out.append(("kv heads of k", wrong, "k and v must be"))
    wrong = dict(base)
    wrong["k"], wrong["v"] = torch.zeros((ntok + 1, N, 128), dtype=F16), torch.zeros((ntok + 1, N, 128), dtype=F16)
    out.append(("tokens of k", wrong, "k and v must be"))
    wrong = dict(base)
    wrong["q"] = base["q"].to(BF16)
    out.append(("q and q_out dtypes differ", wrong, "q_out must be"))
    if init:
        wrong = dict(base)
        wrong["seqlen_indptr"] = torch.tensor([0, 1, 3], dtype=I32)
        out.append(("seqlen_indptr length", wrong, "seqlen_indptr has"))
    else:
        wrong = dict(base)
        wrong["q"], wrong["q_out"] = torch.zeros((B + 1, N, 128), dtype=F16), torch.zeros((B + 1, N, 128), dtype=F16)
        out.append(("one token per sequence", wrong, "q_out and q must be"))
    return out


@pytest.mark.parametrize("init", [False, True], ids=["append", "init"])
def test_bad_writer_arguments_raise_before_the_device_check(init):
    fn = kvrope.rope_init_kv_quantize_i4 if init else kvrope.rope_append_kv_quantize_i4
    cases = _broken_writes(init)
    assert len(cases) >= 45
    for what, kwargs, fragment in cases:
        with pytest.raises(RuntimeError) as e:
            fn(**kwargs)
        assert "must live on the GPU" not in str(e.value), what
        assert fragment in str(e.value), (what, str(e.value))


def test_bad_rope_qk_arguments_raise_before_the_device_check():
    base, cases = _qk_args(), []
    for key, t in base.items():
        wrong = dict(base)
        wrong[key] = t.to(torch.float64)
        cases.append((f"{key} dtype", wrong, key))
        wrong = dict(base)
        wrong[key] = t.unsqueeze(0)
        cases.append((f"{key} rank", wrong, key))
    wrong = dict(base)
    wrong["positions"] = torch.arange(4, dtype=I32)
    cases.append(("n_pos does not divide ntok", wrong, "do not divide"))
    wrong = dict(base)
    wrong["positions"] = torch.zeros(0, dtype=I32)
    cases.append(("n_pos < 1", wrong, "do not divide"))
    wrong = dict(base)
    wrong["k"] = torch.zeros((6, 3, 128), dtype=F16)
    cases.append(("Nq % N", wrong, "multiple"))
    wrong = dict(base)
    wrong["k"] = torch.zeros((5, N, 128), dtype=F16)
    cases.append(("tokens of k", wrong, "one token count"))
    wrong = dict(base)
    wrong["q"] = torch.zeros((6, 8, 128), dtype=F16)[:, ::2]
    cases.append(("q head stride", wrong, "contiguous heads"))
    wrong = dict(base)
    wrong["cos"] = torch.ones((ROPE_LEN, 128), dtype=BF16)
    cases.append(("cos of another dtype", wrong, "cos"))
    wrong = dict(base)
    wrong["sin"] = torch.zeros((ROPE_LEN, 256), dtype=F16)[:, ::2]
    cases.append(("sin non-contiguous", wrong, "contiguous"))
    for what, kwargs, fragment in cases:
        with pytest.raises(RuntimeError) as e:
            kvrope.rope_qk_(**kwargs)
        assert "must live on the GPU" not in str(e.value), what
        assert fragment in str(e.value), (what, str(e.value))


def test_rope_qk_entry_point_validates_without_a_gpu():
    """Status codes of include/arcq.h: -1 shape, -4 NULL."""
    lib = _lib.lib()
    X = 4096

    def call(q=X, k=X, qs=512, ks=256, pos=X, n_pos=3, cos=X, sin=X, rope_len=16, ntok=6, Nq=4, N=2, dtype=0):
        return lib.arcq_rope_qk(q, k, qs, ks, pos, n_pos, cos, sin, rope_len, ntok, Nq, N, dtype, None)

    assert call(dtype=2) == -1 and b"dtype" in lib.arcq_last_error()
    assert call(rope_len=0) == -1 and b"rope_len" in lib.arcq_last_error()
    assert call(n_pos=0) == -1 and b"n_pos" in lib.arcq_last_error()
    assert call(n_pos=4) == -1 and b"n_pos" in lib.arcq_last_error()
    assert call(Nq=3, qs=384) == -1 and b"multiple of N" in lib.arcq_last_error()
    assert call(Nq=0) == -1 and call(N=-1) == -1 and call(ntok=-1) == -1
    assert call(qs=511) == -1 and b"q_stride" in lib.arcq_last_error()
    assert call(qs=504) == -1 and call(qs=516) == -1 and call(ks=248) == -1 and call(ks=260) == -1
    # ntok == 0 before the pointers, behind the shape checks
    assert call(q=None, k=None, pos=None, cos=None, sin=None, ntok=0) == 0
    assert call(ntok=0, qs=8) == -1
    for name in ("q", "k", "pos", "cos", "sin"):
        assert call(**{name: None}) == -4 and b"NULL" in lib.arcq_last_error(), name
    for name in ("q", "k", "cos", "sin"):
        assert call(**{name: X + 8}) == -1 and b"16-byte" in lib.arcq_last_error(), name
    assert call(pos=X + 2) == -1 and b"4-byte" in lib.arcq_last_error()
    # N == 0: k is not looked at (NULL, misaligned, any stride) -- the remaining checks still run
    assert call(N=0, k=None, ks=0, q=None) == -4
    assert call(N=0, k=None, ks=0, cos=X + 8) == -1


@pytest.mark.parametrize("init", [False, True], ids=["append", "init"])
def test_writer_entry_points_validate_without_a_gpu(init):
    """Status codes of include/arcq.h: -1 shape, -2 unsupported, -4 NULL."""
    lib = _lib.lib()
    X = 4096

    def call(data=X, param=X, indptr=X, indices=X, last=X, q_out=1 << 20, q=X, k=X, v=X, qs=512, ks=256, cos=X, sin=X, rope_len=16, sl=X, ntok=5, B=3,
             Nq=4, L=2, layer=0, N=2, P=5, fmt=0, dtype=0):
        if init:
            return lib.arcq_kv_rope_init_quantize(data, param, indptr, indices, last, q_out, q, k, v, qs, ks, cos, sin, rope_len, sl, ntok, B, Nq, L, layer,
                                                  N, P, fmt, dtype, None)
        return lib.arcq_kv_rope_append_quantize(data, param, indptr, indices, last, q_out, q, k, v, qs, ks, cos, sin, rope_len, B, Nq, L, layer, N, P, fmt,
                                                dtype, None)

    assert call(layer=2) == -1 and b"layer_idx" in lib.arcq_last_error()
    assert call(layer=-1) == -1 and call(P=0) == -1 and call(L=0) == -1 and call(N=0) == -1 and call(B=-1) == -1
    assert call(fmt=2) == -1 and b"format" in lib.arcq_last_error()
    assert call(dtype=2) == -1 and b"dtype" in lib.arcq_last_error()
    assert call(Nq=3, qs=384) == -1 and b"multiple of N" in lib.arcq_last_error()
    assert call(Nq=0) == -1
    assert call(fmt=1) == -2 and b"ARCQ_KV_INT4" in lib.arcq_last_error()
    assert call(rope_len=0) == -1 and b"rope_len" in lib.arcq_last_error()
    assert call(qs=511) == -1 and b"q_stride" in lib.arcq_last_error()
    assert call(qs=504) == -1 and call(ks=248) == -1 and call(ks=260) == -1 and call(qs=516) == -1
    none = dict(data=None, param=None, indptr=None, indices=None, last=None, q_out=None, q=None, k=None, v=None, cos=None, sin=None, sl=None)
    assert call(**none, B=0) == 0                                         # B == 0 before the pointers ...
    assert call(B=0, qs=8) == -1                                          # ... but behind the shape checks
    if init:
        assert call(**none, ntok=0) == 0 and call(ntok=-1) == -1
    for name in ("data", "param", "indptr", "indices", "last", "q_out", "q", "k", "v", "cos", "sin") + (("sl",) if init else ()):
        assert call(**{name: None}) == -4 and b"NULL" in lib.arcq_last_error(), name
    for name in ("data", "q_out", "q", "k", "v", "cos", "sin"):
        assert call(**{name: X + 8}) == -1 and b"16-byte" in lib.arcq_last_error(), name
    for name in ("param", "indptr", "indices", "last") + (("sl",) if init else ()):
        assert call(**{name: X + 2}) == -1 and b"4-byte" in lib.arcq_last_error(), name
    # q_out: q itself when q is contiguous (a valid call: not made here, it would launch), otherwise apart from it
    ntok = 5 if init else 3
    assert call(q_out=X, q=X, qs=1024) == -1 and b"q_out" in lib.arcq_last_error()
    assert call(q_out=X + 1024, q=X, qs=512) == -1 and b"q_out" in lib.arcq_last_error()
    assert call(q_out=X + ntok * 1024 - 16, q=X, qs=512) == -1


def test_decoder_model_takes_rope_and_refuses_malformed_tables():
    names = list(inspect.signature(e2e.DecoderModel.__init__).parameters)
    assert names[-3:] == ["rope", "rope_theta", "rope_tables"]
    for fn in (e2e.bench_decode, e2e.bench_protocol):
        p = inspect.signature(fn).parameters
        assert p["rope"].default is False and p["rope_theta"].default == 1e6
    cfg = e2e.ModelConfig("toy", 1, 2, 256, 512, vocab_size=64)
    ok = (torch.ones((8, 128), dtype=BF16), torch.zeros((8, 128), dtype=BF16))
    bad = {"fp16 tables": (ok[0].to(F16), ok[1].to(F16)), "too few positions": (ok[0][:7], ok[1][:7]),
           "wrong width": (torch.ones((8, 64), dtype=BF16), torch.zeros((8, 64), dtype=BF16)), "not a pair": (ok[0],),
           "one malformed": (ok[0], torch.zeros((8, 128), dtype=torch.float32))}
    for what, tables in bad.items():
        with pytest.raises(ValueError, match="rope_tables"):
            e2e.DecoderModel(cfg, 1, 8, "cpu", rope=True, rope_tables=tables)
        assert what
    with pytest.raises(ValueError, match="rope_tables needs rope=True"):
        e2e.DecoderModel(cfg, 1, 8, "cpu", rope_tables=ok)
    with pytest.raises(ValueError, match="head dimension of 128"):
        e2e.DecoderModel(e2e.ModelConfig("toy", 1, 4, 256, 512, vocab_size=64), 1, 8, "cpu", rope=True)
