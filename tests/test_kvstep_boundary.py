"""CPU tests of the decode step's boundary (arcquant_amd.kvstep, include/arcq_kv.h arcq_kv_decode_step): a wrong dtype, rank, layout,
stride, Nq % N or table length raises RuntimeError before anything is launched and CPU tensors are refused LAST; the C entry point returns
its status codes without a GPU (fake aligned pointers are never dereferenced: every check precedes the first HIP call); the state holds
one int32 per (sequence, kv head, chunk of <= 4 query heads)."""
import pytest
import torch

from arcquant_amd import _lib, kvstep

F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
PAGES, L, N, P, B = 4, 2, 2, 5, 3


def _args(dtype=F16, nq=N, sliced=False):
    """Valid (CPU) arguments of decode_step_i4 by keyword; sliced: q, k, v are views of one [B, (nq + 2 N) * 128] buffer."""
    a = dict(kv_data=torch.zeros((PAGES, L, 2, N, P, 64), dtype=U8), kv_param=torch.zeros((PAGES, L, 2, N, P, 2), dtype=F16),
             kv_indptr=torch.tensor([0, 1, 2, 4], dtype=I32), kv_indices=torch.tensor([3, 0, 2, 1], dtype=I32),
             last_page_offset=torch.tensor([1, 5, 2], dtype=I32), layer_idx=1, o=torch.zeros((B, nq, 128), dtype=dtype))
    if sliced:
        a["q"], a["k"], a["v"] = torch.zeros((B, nq + 2 * N, 128), dtype=dtype).split([nq, N, N], dim=1)
        assert not a["q"].is_contiguous() and not a["k"].is_contiguous()
    else:
        a["q"], a["k"], a["v"] = torch.zeros((B, nq, 128), dtype=dtype), torch.zeros((B, N, 128), dtype=dtype), torch.zeros((B, N, 128), dtype=dtype)
    return a


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("nq", [N, 4 * N, 7 * N])
@pytest.mark.parametrize("sliced", [False, True])
def test_valid_cpu_arguments_are_refused_last(dtype, nq, sliced):
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        kvstep.decode_step_i4(**_args(dtype, nq, sliced))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        kvstep.decode_step_i4(**_args(dtype, nq, sliced), state=kvstep.DecodeStepState(B, nq, N, "cpu"))


def _broken():
    """(what, mutated keyword arguments, message fragment)."""
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
    for key in ("o", "kv_data", "kv_param"):                 # these stay contiguous
        wrong = dict(base)
        wrong[key] = torch.cat([base[key], base[key]], dim=-1)[..., : base[key].shape[-1]]
        out.append((f"{key} non-contiguous", wrong, "contiguous"))
    for key in ("q", "k", "v"):
        t = base[key]
        wrong = dict(base)
        wrong[key] = torch.zeros(t.shape[:-1] + (256,), dtype=t.dtype)[..., ::2]                       # elements two apart
        out.append((f"{key} element stride", wrong, "contiguous heads"))
        wrong = dict(base)
        wrong[key] = torch.zeros((t.shape[0], 2 * t.shape[1], 128), dtype=t.dtype)[:, ::2]               # heads 256 apart
        out.append((f"{key} head stride", wrong, "contiguous heads"))
        wrong = dict(base)
        wrong[key] = torch.zeros((t.shape[0], t.shape[1] * 128 + 4), dtype=t.dtype)[:, :t.shape[1] * 128].view(t.shape[0], t.shape[1], 128)
        assert wrong[key].stride(0) % 8 == 4
        out.append((f"{key} token stride not a multiple of 8", wrong, "multiple of 8"))
        wrong = dict(base)
        wrong[key] = torch.zeros(t.shape[:-1] + (64,), dtype=t.dtype)
        out.append((f"{key} head dimension", wrong, "contiguous heads"))
    wrong = dict(base)
    wrong["v"] = torch.zeros((B, N * 128 + 8), dtype=F16)[:, :N * 128].view(B, N, 128)
    out.append(("k and v token strides differ", wrong, "one token stride"))
    wrong = dict(base)
    wrong["kv_data"] = torch.zeros((PAGES, L, 2, N, P, 32), dtype=U8)
    out.append(("head dimension of the cache", wrong, "head dimension 128"))
    wrong = dict(base)
    wrong["kv_indptr"] = torch.tensor([0, 1, 2], dtype=I32)
    out.append(("kv_indptr length", wrong, "kv_indptr has"))
    wrong = dict(base)
    wrong["kv_param"] = torch.zeros((PAGES, L, 2, N, P + 1, 2), dtype=F16)
    out.append(("kv_param shape", wrong, "kv_param must be"))
    wrong = dict(base)
    wrong["layer_idx"] = L
    out.append(("layer_idx", wrong, "layer_idx"))
    out.append(("Nq % N", _args(nq=3), "not a multiple"))
    wrong = dict(base)
    wrong["q"], wrong["o"] = torch.zeros((B + 1, N, 128), dtype=F16), torch.zeros((B + 1, N, 128), dtype=F16)
    out.append(("batch of q", wrong, "o and q must be"))
    wrong = dict(base)
    wrong["o"] = torch.zeros((B, 2 * N, 128), dtype=F16)
    out.append(("o against q", wrong, "o and q must be"))
    wrong = dict(base)
    wrong["k"], wrong["v"] = torch.zeros((B, N + 1, 128), dtype=F16), torch.zeros((B, N + 1, 128), dtype=F16)
    out.append(("kv heads of k", wrong, "k and v must be"))
    wrong = dict(base)
    wrong["k"], wrong["v"] = torch.zeros((B + 1, N, 128), dtype=F16), torch.zeros((B + 1, N, 128), dtype=F16)
    out.append(("one token per sequence", wrong, "k and v must be"))
    wrong = dict(base)
    wrong["q"] = base["q"].to(BF16)
    out.append(("q and o dtypes differ", wrong, "o must be"))
    wrong = dict(base)
    wrong["state"] = torch.zeros(64, dtype=I32)
    out.append(("state type", wrong, "DecodeStepState"))
    wrong = dict(base)
    wrong["state"] = kvstep.DecodeStepState(B + 1, N, N, "cpu")
    out.append(("state of another batch", wrong, "state was built for"))
    return out


def test_bad_arguments_raise_runtime_error_before_the_device_check():
    cases = _broken()
    assert len(cases) >= 40
    for what, kwargs, fragment in cases:
        with pytest.raises(RuntimeError) as e:
            kvstep.decode_step_i4(**kwargs)
        assert "must live on the GPU" not in str(e.value), what          # (the device check comes last: these fail earlier)
        assert fragment in str(e.value), (what, str(e.value))


def test_state_arguments():
    s = kvstep.DecodeStepState(3, 14, 2, "cpu")
    assert s.counters.dtype is I32 and s.counters.numel() == 3 * 2 * 2 and not s.counters.any()
    assert s.workspace.dtype is torch.float32 and s.workspace.numel() == 3 * 14 * 32 * 130
    for bad in ((0, 2, 2), (1, 3, 2), (1, 2, 0)):
        with pytest.raises(RuntimeError):
            kvstep.DecodeStepState(*bad, "cpu")


@pytest.mark.parametrize("g", [1, 4, 7])
def test_state_scratch_covers_the_most_slices_a_call_can_use(g):
    """DecodeStepState sizes its record scratch for 32 slices per sequence: no table size makes the workspace query ask for more."""
    lib = _lib.lib()
    for b, n in ((1, 1), (1, 28), (4, 28), (64, 8)):
        s = kvstep.DecodeStepState(b, g * n, n, "cpu")
        for p in (1, 5, 16, 256):
            for nnz in (1, b, 64 * b, 4096 * b, 10 ** 6, (2 ** 31 - 1) // p):
                assert lib.arcq_kv_decode_workspace_bytes(b, g * n, n, nnz, p) <= s.workspace.numel() * 4, (b, n, p, nnz)
    assert kvstep._MAX_SLICES * kvstep._RECORD * 4 == 32 * 130 * 4


@pytest.mark.parametrize("g", [1, 2, 4, 7])
def test_state_bytes(g):
    """One int32 per (sequence, kv head, chunk): a chunk holds min(g, 4) query heads of a kv head."""
    lib = _lib.lib()
    chunks = -(-g // min(g, 4))
    for b, n in ((1, 1), (3, 2), (4, 28)):
        assert lib.arcq_kv_decode_step_state_bytes(b, g * n, n) == 4 * b * n * chunks
    assert lib.arcq_kv_decode_step_state_bytes(0, g, 1) == 0 and lib.arcq_kv_decode_step_state_bytes(2, 3, 2) == 0


def test_entry_point_validates_without_a_gpu():
    """Status codes of include/arcq.h: -1 shape, -2 unsupported, -4 NULL, -5 workspace."""
    lib = _lib.lib()
    X = 4096
    step = lib.arcq_kv_decode_step

    def call(o=X, q=X, k=X, v=X, qs=256, ks=256, data=X, param=X, indptr=X, indices=X, last=X, B=3, Nq=2, L=2, layer=0, N=2, P=5, nnz=4, fmt=0,
             dtype=0, ws=None, ws_bytes=0, state=None, state_bytes=0):
        return step(o, q, k, v, qs, ks, data, param, indptr, indices, last, B, Nq, L, layer, N, P, nnz, fmt, dtype, ws, ws_bytes, state, state_bytes, None)

    # geometry, dtype, Nq % N, nnz
    assert call(layer=2) == -1 and b"layer_idx" in lib.arcq_last_error()
    assert call(layer=-1) == -1 and call(P=0) == -1 and call(L=0) == -1 and call(N=0) == -1 and call(B=-1) == -1
    assert call(fmt=2) == -1 and b"format" in lib.arcq_last_error()
    assert call(dtype=2) == -1 and b"dtype" in lib.arcq_last_error()
    assert call(Nq=3, qs=384) == -1 and b"multiple of N" in lib.arcq_last_error()
    assert call(Nq=0) == -1
    assert call(nnz=-1) == -1 and b"nnz" in lib.arcq_last_error()
    assert call(nnz=2 ** 31) == -1
    # the format: the step quantises, so int4 only -- and that is said before the strides are looked at
    assert call(fmt=1) == -2 and b"ARCQ_KV_INT4" in lib.arcq_last_error()
    assert call(fmt=1, qs=8) == -2
    # strides: at least a token's heads, multiples of 8 elements
    assert call(qs=255) == -1 and b"q_stride" in lib.arcq_last_error()
    assert call(qs=248) == -1 and call(ks=248) == -1 and call(ks=260) == -1 and call(qs=260) == -1
    # B == 0 before the pointers
    assert call(o=None, q=None, k=None, v=None, data=None, param=None, indptr=None, indices=None, last=None, B=0) == 0
    assert call(B=0, qs=8) == -1                                           # ... but behind the shape checks
    # NULLs
    for name in ("o", "q", "k", "v", "data", "param", "indptr", "indices", "last"):
        assert call(**{name: None}) == -4, name
        assert b"NULL" in lib.arcq_last_error()
    # alignment: 16 bytes for o, q, k, v, kv_data; 4 for the rest
    for name in ("o", "q", "k", "v", "data"):
        assert call(**{name: X + 8}) == -1 and b"16-byte" in lib.arcq_last_error(), name
    for name in ("param", "indptr", "indices", "last"):
        assert call(**{name: X + 2}) == -1 and b"4-byte" in lib.arcq_last_error(), name
    # two slices per sequence: B = 2, N = 1, 20 pages of 16 each -> the workspace and the state are needed
    long = dict(B=2, Nq=4, N=1, P=16, nnz=40, qs=512, ks=128)
    need, cnt = lib.arcq_kv_decode_workspace_bytes(2, 4, 1, 40, 16), lib.arcq_kv_decode_step_state_bytes(2, 4, 1)
    assert need == 2 * 4 * 2 * 130 * 4 and cnt == 8
    assert call(**long, ws=X + 2, ws_bytes=need, state=X, state_bytes=cnt) == -1 and b"4-byte" in lib.arcq_last_error()
    assert call(**long, ws=X, ws_bytes=need, state=X + 2, state_bytes=cnt) == -1 and b"4-byte" in lib.arcq_last_error()
    assert call(**long, ws=None, ws_bytes=need, state=X, state_bytes=cnt) == -5
    assert call(**long, ws=X, ws_bytes=need - 4, state=X, state_bytes=cnt) == -5 and b"workspace" in lib.arcq_last_error()
    assert call(**long, ws=X, ws_bytes=need, state=None, state_bytes=cnt) == -5
    assert call(**long, ws=X, ws_bytes=need, state=X, state_bytes=cnt - 4) == -5 and b"state" in lib.arcq_last_error()
