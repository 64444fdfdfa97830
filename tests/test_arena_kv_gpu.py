"""Arena tests of the KV-cache C-ABI (``-m gpu``, include/arcq_kv.h): every arcq_kv_* entry point with its operands between poisoned guards
(tests/arena.py), bit-exact against the same call on tight allocations.

Writers: kv_data / kv_param are in-place operands; every byte outside the targeted rows is don't-care -- it holds the poison, must still
hold it afterwards and must not influence what is written.  Decode: kv_data / kv_param are inputs whose bytes outside the valid positions
of the referenced pages of the layer asked for are don't-care: other layers, unreferenced pages and the entries >= last_page_offset of a
last page.  That is the test of the page-tail guard, so the lengths end mid-page, at a page's last slot and at a page's first one."""
import numpy as np
import pytest
import torch

from tests import kv_reference as R
from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
L, N = 2, 2
KV_INT4, KV_16BIT = 0, 1


def _L():
    from arcquant_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(lens, P, seed):
    pages, indptr, indices, last = R.make_tables(lens, P, seed)
    return pages, (indptr, indices, last), {"indptr": In(_dev(indptr), 4), "indices": In(_dev(indices), 4), "last": In(_dev(last), 4)}


def _byte_mask(rows: np.ndarray, row_bytes: int) -> torch.Tensor:
    """bool [pages, L, 2, N, P] of rows -> bool over the bytes of the tensor."""
    return torch.from_numpy(np.repeat(rows.reshape(-1), row_bytes))


def _target_rows(shape5, tabs, new, layer):
    """The rows a writer fills: the last new[b] positions of sequence b, K and V, every head, in `layer`."""
    indptr, indices, last = tabs
    m = np.zeros(shape5, dtype=bool)
    for b, T in enumerate(R.seq_lens(indptr, last, shape5[4])):
        for pos in range(int(T) - new[b], int(T)):
            page, e = R.locate(indptr, indices, b, pos, shape5[4])
            m[page, layer, :, :, e] = True
    return m


@pytest.mark.parametrize("P,lens", [(16, (1, 15, 16)), (5, (6, 17, 10))])
@pytest.mark.parametrize("fmt", [KV_INT4, KV_16BIT])
def test_kv_copy_writers(P, lens, fmt):
    """arcq_kv_init (whole sequences, then their last positions only) and arcq_kv_append."""
    lib = _L()
    B, row = len(lens), 64 if fmt == KV_INT4 else 256
    for layer in range(L):
        pages, tabs, tin = _tables(lens, P, 3 + layer)
        shape5 = (pages, L, 2, N, P)
        g = torch.Generator(device=DEV).manual_seed(P + layer)
        data0 = torch.randint(0, 256, shape5 + (row,), generator=g, device=DEV, dtype=U8)
        param0 = torch.randint(0, 256, shape5 + (4,), generator=g, device=DEV, dtype=U8)
        for new in (list(lens), [1, 2, min(lens[2], 7)], None):
            n_new = [1] * B if new is None else new
            sl = np.concatenate([[0], np.cumsum(n_new)]).astype(np.int32)
            ntok = int(sl[-1])
            ins = dict(tin)
            for name, width in (("k", row), ("v", row), ("kp", 4), ("vp", 4)):
                ins[name] = In(torch.randint(0, 256, (ntok, N, width), generator=g, device=DEV, dtype=U8), 16 if width == row else 4)
            if new is not None:
                ins["sl"] = In(_dev(sl), 4)
            keep = ~_target_rows(shape5, tabs, n_new, layer)
            outs = {"data": Out(data0.shape, U8, 16, dont_care=_byte_mask(keep, row), init=data0),
                    "param": Out(param0.shape, U8, 4, dont_care=_byte_mask(keep, 4), init=param0)}

            def call(o):
                if new is None:
                    return lib.arcq_kv_append(_p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), _p(o["k"]), _p(o["v"]),
                                              _p(o["kp"]), _p(o["vp"]), B, L, layer, N, P, fmt, _stream())
                return lib.arcq_kv_init(_p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), _p(o["k"]), _p(o["v"]), _p(o["kp"]),
                                        _p(o["vp"]), _p(o["sl"]), ntok, B, L, layer, N, P, fmt, _stream())
            run_in_arenas(call, ins, outs, device=DEV)


@pytest.mark.parametrize("P,lens", [(16, (1, 15, 16)), (5, (6, 17, 10))])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_kv_quantising_writers(P, lens, dtype):
    """arcq_kv_init_quantize and arcq_kv_append_quantize."""
    lib = _L()
    B, code = len(lens), 0 if dtype is F16 else 1
    for layer in range(L):
        pages, tabs, tin = _tables(lens, P, 5 + layer)
        shape5 = (pages, L, 2, N, P)
        g = torch.Generator(device=DEV).manual_seed(P + layer + 1)
        data0 = torch.randint(0, 256, shape5 + (64,), generator=g, device=DEV, dtype=U8)
        param0 = torch.randint(0, 256, shape5 + (4,), generator=g, device=DEV, dtype=U8)
        for new in (list(lens), [1, 2, min(lens[2], 7)], None):
            n_new = [1] * B if new is None else new
            sl = np.concatenate([[0], np.cumsum(n_new)]).astype(np.int32)
            ntok = int(sl[-1])
            ins = dict(tin)
            for name in ("k", "v"):
                ins[name] = In((torch.randn((ntok, N, 128), generator=g, device=DEV) * 3).to(dtype), 16)
            if new is not None:
                ins["sl"] = In(_dev(sl), 4)
            keep = ~_target_rows(shape5, tabs, n_new, layer)
            outs = {"data": Out(data0.shape, U8, 16, dont_care=_byte_mask(keep, 64), init=data0),
                    "param": Out(param0.shape, U8, 4, dont_care=_byte_mask(keep, 4), init=param0)}

            def call(o):
                if new is None:
                    return lib.arcq_kv_append_quantize(_p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), _p(o["k"]),
                                                       _p(o["v"]), B, L, layer, N, P, KV_INT4, code, _stream())
                return lib.arcq_kv_init_quantize(_p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), _p(o["k"]), _p(o["v"]),
                                                 _p(o["sl"]), ntok, B, L, layer, N, P, KV_INT4, code, _stream())
            run_in_arenas(call, ins, outs, device=DEV)


# lengths that end mid-page, at a page's last slot and at a page's first; the last case splits the sequences (workspace + combine)
DECODE = [(16, (1, 15, 16), N), (16, (17, 50, 32), N), (5, (6, 17, 10), N), (16, (600, 515), 1)]
# the ragged batches of tests/kv_reference.CASES (ragged, odd, empty): a wave streams three or four blocks, and the clamped loads of the
# last one are where a stray read would show; slices without work; a sequence of 1, of 2 and of no positions
RAGGED = [(16, (1000, 1, 33, 2), 1), (16, (700, 1, 67), 1), (16, (1000, 0, 33, 0), 1)]
# slices per sequence (kv_decode_splits), the same at every group width used here
SLICES = {(1, 15, 16): 1, (17, 50, 32): 1, (6, 17, 10): 1, (600, 515): 4, (300, 260): 2, (1000, 1, 33, 2): 2, (700, 1, 67): 2, (1000, 0, 33, 0): 2}


def expected_workspace_bytes(lens, Nq):
    S = SLICES[tuple(lens)]
    return 0 if S == 1 else len(lens) * Nq * S * 130 * 4


@pytest.mark.parametrize("P,lens,n_heads", DECODE)
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("fmt,dtype", [(KV_INT4, F16), (KV_INT4, BF16), (KV_16BIT, F16), (KV_16BIT, BF16)], ids=["i4-f16", "i4-bf16", "16-f16", "16-bf16"])
def test_kv_batch_decode_reads_valid_positions_only(P, lens, n_heads, g, fmt, dtype):
    """The output is bit-identical under all three poisons in every byte decode must not read."""
    _decode_in_arenas(P, lens, n_heads, g, fmt, dtype)


@pytest.mark.parametrize("P,lens,n_heads", RAGGED)
@pytest.mark.parametrize("g", [2, 7])
@pytest.mark.parametrize("fmt,dtype", [(KV_INT4, F16), (KV_INT4, BF16), (KV_16BIT, F16), (KV_16BIT, BF16)], ids=["i4-f16", "i4-bf16", "16-f16", "16-bf16"])
def test_kv_batch_decode_of_ragged_batches_reads_valid_positions_only(P, lens, n_heads, g, fmt, dtype):
    want = _decode_in_arenas(P, lens, n_heads, g, fmt, dtype)
    for b, T in enumerate(lens):
        assert T or not want["o"].view(len(lens), -1)[b].any(), "a sequence without positions gives zeros"


def _decode_in_arenas(P, lens, n_heads, g, fmt, dtype):
    lib = _L()
    B, Nq, layer, code = len(lens), g * n_heads, 1, 0 if dtype is F16 else 1
    pages, tabs, tin = _tables(lens, P, 9)
    shape5 = (pages, L, 2, n_heads, P)
    gen = torch.Generator(device=DEV).manual_seed(P + sum(lens))
    if fmt == KV_INT4:
        data = torch.randint(0, 256, shape5 + (64,), generator=gen, device=DEV, dtype=U8)
        row_bytes = 64
    else:
        data = (torch.randn(shape5 + (128,), generator=gen, device=DEV) * 3).to(dtype)
        row_bytes = 256
    # (scale, zero) of plausible magnitude
    param = torch.stack([torch.rand(shape5, generator=gen, device=DEV) * 0.5 + 0.1, torch.rand(shape5, generator=gen, device=DEV) * 4], dim=-1).to(F16)
    unread = ~R.valid_row_mask(shape5, *tabs, layer)
    ins = dict(tin)
    ins["q"] = In(torch.randn((B, Nq, 128), generator=gen, device=DEV).to(dtype), 16)
    ins["data"] = In(data, 16, dont_care=_byte_mask(unread, row_bytes))
    # a 16-bit cache's parameters are never applied: every byte of them is don't-care
    ins["param"] = In(param, 4, dont_care=_byte_mask(unread if fmt == KV_INT4 else np.ones_like(unread), 4))
    nnz = int(tabs[1].shape[0])
    ws_bytes = int(lib.arcq_kv_decode_workspace_bytes(B, Nq, n_heads, nnz, P))
    assert ws_bytes == expected_workspace_bytes(lens, Nq), "the slice count of this case changed"
    scratch = {"ws": Out((ws_bytes // 4,), torch.float32, 4)} if ws_bytes else {}

    def call(o):
        return lib.arcq_kv_batch_decode(_p(o["o"]), _p(o["q"]), _p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), B, Nq, L,
                                        layer, n_heads, P, nnz, fmt, code, _p(o.get("ws")), ws_bytes, _stream())
    want = run_in_arenas(call, ins, {"o": Out((B, Nq, 128), dtype, 16)}, scratch, device=DEV)
    assert torch.isfinite(want["o"].view(dtype).float()).all()
    return want
