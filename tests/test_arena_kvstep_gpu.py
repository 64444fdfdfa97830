"""Arena test of arcq_kv_decode_step (``-m gpu``, include/arcq_kv.h): the one-launch decode step with its operands between poisoned guards
(tests/arena.py), bit-exact against the same call on tight allocations.

kv_data / kv_param are in-place operands.  The step writes the K and V rows of position T - 1 of every sequence in the layer asked for and
reads positions 0 .. T - 2.  Of the bytes outside the written rows

  - those tests/kv_reference.valid_row_mask calls unread (other layers, unreferenced pages, entries past a sequence's end) are don't-care:
    they hold the poison, must still hold it afterwards and must not influence the result;
  - the rows the step reads keep their values and are compared with the tight run's, i.e. must come back unchanged

so every byte outside the written rows is checked for being left alone, one way or the other.  (Declaring the rows that are read don't-care
as well would poison the step's own input: the arena demands that a don't-care byte holds the poison before and after the call.)  The
written rows themselves start as poison too: the step must not read what the page held there.  q, k, v are inputs, the record workspace is
scratch, and the counters are an output without don't-care bytes that starts zeroed and must come back zeroed."""
import numpy as np
import pytest
import torch

from tests import kv_reference as R
from tests.arena import In, Out, run_in_arenas
from tests.test_arena_kv_gpu import DECODE, RAGGED, _byte_mask, _L, _p, _stream, _tables, _target_rows, expected_workspace_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8 = torch.float16, torch.bfloat16, torch.uint8
L = 2
KV_INT4 = 0


@pytest.mark.parametrize("P,lens,n_heads", DECODE + [(16, (300, 260), 1)])
@pytest.mark.parametrize("g", [1, 4, 7])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_kv_decode_step_reads_and_writes_its_rows_only(P, lens, n_heads, g, dtype):
    _step_in_arenas(P, lens, n_heads, g, dtype)


@pytest.mark.parametrize("P,lens,n_heads", RAGGED)
@pytest.mark.parametrize("g", [2, 7])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_kv_decode_step_of_ragged_batches_reads_and_writes_its_rows_only(P, lens, n_heads, g, dtype):
    """Deep loops (the clamped tail loads of a wave's third or fourth block), idle slices, sequences of 1, 2 and no positions."""
    want = _step_in_arenas(P, lens, n_heads, g, dtype)
    for b, T in enumerate(lens):
        assert T or not want["o"].view(len(lens), -1)[b].any(), "a sequence without positions gives zeros"


def _step_in_arenas(P, lens, n_heads, g, dtype):
    lib = _L()
    B, Nq, layer, code = len(lens), g * n_heads, 1, 0 if dtype is F16 else 1
    pages, tabs, tin = _tables(lens, P, 9)
    shape5 = (pages, L, 2, n_heads, P)
    gen = torch.Generator(device=DEV).manual_seed(P + sum(lens) + g)
    data = torch.randint(0, 256, shape5 + (64,), generator=gen, device=DEV, dtype=U8)
    # (scale, zero) of plausible magnitude
    param = torch.stack([torch.rand(shape5, generator=gen, device=DEV) * 0.5 + 0.1, torch.rand(shape5, generator=gen, device=DEV) * 4], dim=-1).to(F16)
    written = _target_rows(shape5, tabs, [min(T, 1) for T in lens], layer)
    unread = ~R.valid_row_mask(shape5, *tabs, layer)                   # (the lengths include the new position: the written rows are "valid")
    assert not (written & unread).any() and written.sum() == 2 * n_heads * sum(T > 0 for T in lens)
    ins = dict(tin)
    for name, heads in (("q", Nq), ("k", n_heads), ("v", n_heads)):
        ins[name] = In((torch.randn((B, heads, 128), generator=gen, device=DEV) * (1 if name == "q" else 3)).to(dtype), 16)
    outs = {"o": Out((B, Nq, 128), dtype, 16),
            "data": Out(data.shape, U8, 16, dont_care=_byte_mask(unread, 64), init=data, poison=_byte_mask(unread | written, 64)),
            "param": Out(param.shape, F16, 4, dont_care=_byte_mask(unread, 4), init=param, poison=_byte_mask(unread | written, 4))}
    nnz = int(tabs[1].shape[0])
    ws_bytes = int(lib.arcq_kv_decode_workspace_bytes(B, Nq, n_heads, nnz, P))
    assert ws_bytes == expected_workspace_bytes(lens, Nq), "the slice count of this case changed"
    st_bytes = int(lib.arcq_kv_decode_step_state_bytes(B, Nq, n_heads))
    scratch = {"ws": Out((ws_bytes // 4,), torch.float32, 4)} if ws_bytes else {}
    outs["state"] = Out((st_bytes // 4,), torch.int32, 4, init=torch.zeros(st_bytes // 4, dtype=torch.int32, device=DEV))

    def call(o):
        return lib.arcq_kv_decode_step(_p(o["o"]), _p(o["q"]), _p(o["k"]), _p(o["v"]), Nq * 128, n_heads * 128, _p(o["data"]), _p(o["param"]),
                                       _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), B, Nq, L, layer, n_heads, P, nnz, KV_INT4, code,
                                       _p(o.get("ws")), ws_bytes, _p(o["state"]), st_bytes, _stream())
    want = run_in_arenas(call, ins, outs, scratch, device=DEV)
    assert torch.isfinite(want["o"].view(dtype).float()).all()
    assert st_bytes == 4 * B * n_heads * R.decode_chunks(g) and not want["state"].any(), "the counters did not come back zeroed"
    # the tight run changed the written rows and nothing else
    keep = torch.from_numpy(~np.repeat(written.reshape(-1), 64))
    assert torch.equal(want["data"].cpu()[keep], data.reshape(-1).cpu()[keep])
    keep = torch.from_numpy(~np.repeat(written.reshape(-1), 4))
    assert torch.equal(want["param"].cpu()[keep], param.reshape(-1).view(U8).cpu()[keep])
    return want
