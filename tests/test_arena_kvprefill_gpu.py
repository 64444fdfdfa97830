"""Arena test of arcq_kv_batch_prefill (``-m gpu``, include/arcq_kv.h): every operand between poisoned guards (tests/arena.py), the
output bit-identical to the same call on tight allocations under the three poisons in every byte the call must not read -- the other
layer, pages no sequence owns, entries of a last page at or beyond last_page_offset, the page of a sequence without positions -- and
nothing written outside the rows of o that belong to a sequence.  The case is ``chunk`` of tests/kv_prefill_reference.py: chunk lengths
on both sides of a tile, a whole-sequence prefill, a sequence without query tokens and one without positions (both spellings)."""
import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R
from tests.arena import In, Out, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8 = torch.float16, torch.bfloat16, torch.uint8
KV_INT4 = 0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return t.data_ptr()


@pytest.mark.parametrize("case", ["chunk", "chunk1"])
@pytest.mark.parametrize("g", [1, 4, 7])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_kv_batch_prefill_reads_valid_positions_only(case, g, dtype):
    from arcquant_amd import _lib
    lib = _lib.lib()
    spec, lens, new, qo, pages, tabs = PR.case_geometry(case)
    P, N, L, layer = spec["P"], spec["N"], PR.L, PR.LAYER
    B, Nq, code = len(lens), g * N, 0 if dtype is F16 else 1
    ntok = int(qo[-1]) + PR.PAD_ROWS
    shape5 = (pages, L, 2, N, P)
    gen = torch.Generator(device=DEV).manual_seed(P + sum(lens) + g)
    data = torch.randint(0, 256, shape5 + (64,), generator=gen, device=DEV, dtype=U8)
    param = torch.stack([torch.rand(shape5, generator=gen, device=DEV) * 0.5 + 0.1, torch.rand(shape5, generator=gen, device=DEV) * 4], dim=-1).to(F16)
    unread = ~R.valid_row_mask(shape5, *tabs, layer)
    assert unread[:, 0].all() and unread[:, layer].any() and not unread[:, layer].all()
    ins = {"indptr": In(_dev(tabs[0]), 4), "indices": In(_dev(tabs[1]), 4), "last": In(_dev(tabs[2]), 4), "qo": In(_dev(qo), 4),
           "q": In(torch.randn((ntok, Nq, 128), generator=gen, device=DEV).to(dtype), 16),
           "data": In(data, 16, dont_care=torch.from_numpy(np.repeat(unread.reshape(-1), 64))),
           "param": In(param, 4, dont_care=torch.from_numpy(np.repeat(unread.reshape(-1), 4)))}
    # rows of o at or beyond qo_indptr[B] belong to no sequence: they must keep the poison
    no_row = torch.zeros((ntok, Nq * 128 * 2), dtype=torch.bool)
    no_row[int(qo[-1]):] = True
    nnz = int(tabs[1].shape[0])

    def call(o):
        return lib.arcq_kv_batch_prefill(_p(o["o"]), _p(o["q"]), _p(o["qo"]), _p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]),
                                         _p(o["last"]), ntok, B, Nq, L, layer, N, P, nnz, KV_INT4, code, torch.cuda.current_stream().cuda_stream)
    want = run_in_arenas(call, ins, {"o": Out((ntok, Nq, 128), dtype, 16, dont_care=no_row.reshape(-1))}, device=DEV)
    rows = want["o"].view(dtype).view(ntok, Nq, 128)[:int(qo[-1])]
    assert torch.isfinite(rows.float()).all()
