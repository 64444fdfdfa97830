"""Arena tests of the RoPE entry points (``-m gpu``, include/arcq_kv.h): arcq_rope_qk, arcq_kv_rope_append_quantize and
arcq_kv_rope_init_quantize with their operands between poisoned guards (tests/arena.py), bit-exact against the same call on tight
allocations.

cos / sin have exactly ``rope_len`` = longest-sequence rows, so the last table row is used and the byte behind it is the guard.  Writers:
kv_data / kv_param are in-place operands whose bytes outside the targeted rows are don't-care; q_out is an output whose rows of tokens
without a position (an empty sequence, rows at or beyond seqlen_indptr[B]) are don't-care: they must still hold the poison.  arcq_rope_qk
works in place: q and k are in-place outputs of which every byte is rewritten; as slices of one buffer, the v columns and the spare
elements of each row are don't-care."""
import numpy as np
import pytest
import torch

from tests import rope_reference as RR
from tests.arena import In, Out, run_in_arenas
from tests.test_arena_kv_gpu import _byte_mask, _dev, _L, _p, _stream, _tables, _target_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8 = torch.float16, torch.bfloat16, torch.uint8
L = 2
KV_INT4 = 0


@pytest.mark.parametrize("P,lens,new,N,g", [(3, (1, 3, 7), None, 2, 1), (1, (1, 2, 5, 9, 0), None, 1, 4), (4, (4, 1, 5, 20), (0, 1, 5, 8), 2, 2)],
                         ids=["append", "append-empty", "init"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_rope_writers_read_and_write_their_rows_only(P, lens, new, N, g, dtype):
    lib = _L()
    B, Nq, layer, code = len(lens), N * g, 1, 0 if dtype is F16 else 1
    n_new = [min(1, T) for T in lens] if new is None else list(new)
    sl = np.concatenate([[0], np.cumsum([1] * B if new is None else n_new)]).astype(np.int32)
    ntok = int(sl[-1]) + (0 if new is None else 2)
    rope_len = max(lens)
    pages, tabs, tin = _tables(lens, P, 7)
    shape5 = (pages, L, 2, N, P)
    gen = torch.Generator(device=DEV).manual_seed(P + sum(lens))
    data0 = torch.randint(0, 256, shape5 + (64,), generator=gen, device=DEV, dtype=U8)
    param0 = torch.randint(0, 256, shape5 + (4,), generator=gen, device=DEV, dtype=U8)
    cos, sin = RR.rope_tables(rope_len, 1e4, dtype)
    ins = dict(tin)
    ins["cos"], ins["sin"] = In(cos.to(DEV), 16), In(sin.to(DEV), 16)
    for name, heads in (("q", Nq), ("k", N), ("v", N)):
        ins[name] = In(RR.rows(ntok, heads, dtype, 5 + heads).to(DEV), 16)
    if new is not None:
        ins["sl"] = In(_dev(sl), 4)
    keep = ~_target_rows(shape5, tabs, n_new, layer)
    # q_out rows of tokens without a position are left alone
    unwritten = np.ones(ntok, dtype=bool)
    for b in range(B):
        cnt = int(sl[b + 1] - sl[b])
        for j in range(cnt):
            unwritten[sl[b] + j] = lens[b] - cnt + j < 0
    assert unwritten.any() == (new is not None or 0 in lens)
    outs = {"q_out": Out((ntok, Nq, 128), dtype, 16, dont_care=torch.from_numpy(np.repeat(unwritten, Nq * 256))),
            "data": Out(data0.shape, U8, 16, dont_care=_byte_mask(keep, 64), init=data0),
            "param": Out(param0.shape, U8, 4, dont_care=_byte_mask(keep, 4), init=param0)}

    def call(o):
        head = (_p(o["data"]), _p(o["param"]), _p(o["indptr"]), _p(o["indices"]), _p(o["last"]), _p(o["q_out"]), _p(o["q"]), _p(o["k"]), _p(o["v"]),
                Nq * 128, N * 128, _p(o["cos"]), _p(o["sin"]), rope_len)
        tail = (B, Nq, L, layer, N, P, KV_INT4, code, _stream())
        if new is None:
            return lib.arcq_kv_rope_append_quantize(*head, *tail)
        return lib.arcq_kv_rope_init_quantize(*head, _p(o["sl"]), ntok, *tail)
    want = run_in_arenas(call, ins, outs, device=DEV)
    written = torch.from_numpy(~np.repeat(unwritten, Nq * 256))
    assert torch.isfinite(want["q_out"].cpu()[written].view(dtype).float()).all()


@pytest.mark.parametrize("n_pos", [6, 3, 1])
@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_rope_qk_reads_and_writes_its_rows_only(dtype, sliced, n_pos):
    lib = _L()
    ntok, Nq, N, rope_len, code = 6, 4, 2, 12, 0 if dtype is F16 else 1
    positions = {6: (5, 0, 9, 2, 7, 11), 3: (9, 10, 11), 1: (11,)}[n_pos]
    cos, sin = RR.rope_tables(rope_len, 1e6, dtype)
    ins = {"cos": In(cos.to(DEV), 16), "sin": In(sin.to(DEV), 16), "pos": In(torch.tensor(positions, dtype=torch.int32, device=DEV), 4)}
    q, k = RR.rows(ntok, Nq, dtype, 21).to(DEV), RR.rows(ntok, N, dtype, 22).to(DEV)
    if sliced:                 # one [ntok, (Nq + 2 N) * 128 + 8] buffer: the v columns and the 8 spare elements of a row are don't-care
        width = (Nq + 2 * N) * 128 + 8
        buf = torch.zeros((ntok, width), dtype=dtype, device=DEV)
        buf[:, :Nq * 128], buf[:, Nq * 128:(Nq + N) * 128] = q.view(ntok, -1), k.view(ntok, -1)
        dc = np.zeros((ntok, width), dtype=bool)
        dc[:, (Nq + N) * 128:] = True
        outs = {"buf": Out(buf.shape, dtype, 16, dont_care=torch.from_numpy(np.repeat(dc.reshape(-1), 2)), init=buf)}

        def call(o):
            base = o["buf"].data_ptr()
            return lib.arcq_rope_qk(base, base + Nq * 256, width, width, _p(o["pos"]), n_pos, _p(o["cos"]), _p(o["sin"]), rope_len, ntok, Nq, N, code,
                                    _stream())
    else:
        outs = {"q": Out(q.shape, dtype, 16, init=q), "k": Out(k.shape, dtype, 16, init=k)}

        def call(o):
            return lib.arcq_rope_qk(_p(o["q"]), _p(o["k"]), Nq * 128, N * 128, _p(o["pos"]), n_pos, _p(o["cos"]), _p(o["sin"]), rope_len, ntok, Nq, N, code,
                                    _stream())
    want = run_in_arenas(call, ins, outs, device=DEV)
    # and the tight run is the reference's rotation
    per_token = np.array(positions)[np.arange(ntok) % n_pos]
    ref_q = RR.apply_rope(q.cpu(), per_token, cos, sin)
    got = want["buf"].view(dtype).view(ntok, -1)[:, :Nq * 128] if sliced else want["q"].view(dtype).view(ntok, -1)
    assert torch.equal(got.cpu().view(torch.int16), ref_q.view(ntok, -1).view(torch.int16))
