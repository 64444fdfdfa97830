"""GPU tests of the RoPE entry points (``-m gpu``; arcquant_amd.kvrope, include/arcq_kv.h): byte-exact throughout against torch eager on
the CPU (tests/rope_reference.py) and the quantiser's reference (tests/kv_reference.py).

Inputs are seeded normal values times per-row magnitudes 2^-12 .. 2^4, so that fp16 products land on the subnormal grid; the tables have
exactly as many rows as the longest sequence has positions, so the last table row is used.  The caches start as 0xA5 bytes in both layers
of L = 2 and are compared WHOLE: every byte outside the written rows must still be 0xA5."""
import functools

import numpy as np
import pytest
import torch

from arcquant_amd import kvcache, kvrope
from tests import kv_reference as R
from tests import rope_reference as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
L, FILL = 2, 0xA5

# name -> P, lens (positions per sequence, the new ones included), new (tokens per sequence; None: append), N, g, extra rows of q / k / v
CASES = {
    "append-p3": dict(P=3, lens=(1, 3, 7), new=None, N=2, g=1, extra=0),            # position 0, a page-exact end, mid-page; 18 rows
    "append-p1-empty": dict(P=1, lens=(1, 2, 5, 9, 0), new=None, N=1, g=4, extra=0),   # a sequence without positions writes nothing
    "append-p16": dict(P=16, lens=(16, 17), new=None, N=3, g=2, extra=0),
    "init-p4": dict(P=4, lens=(4, 1, 5, 20), new=(0, 1, 5, 8), N=2, g=2, extra=2),  # two rows beyond seqlen_indptr[B] keep their fill
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, dtype, theta):
    """Inputs and expected bytes of one case, on the CPU.  Built once and shared; nothing may modify it."""
    c = CASES[name]
    P, lens, N, Nq = c["P"], c["lens"], c["N"], c["N"] * c["g"]
    B = len(lens)
    new = [1] * B if c["new"] is None else list(c["new"])
    sl = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    ntok = int(sl[-1]) + c["extra"]
    rope_len = max(lens)
    cos, sin = RR.rope_tables(rope_len, theta, dtype)
    seed = len(name) + P + (dtype is F16)
    q, k, v = RR.rows(ntok, Nq, dtype, seed), RR.rows(ntok, N, dtype, seed + 100), RR.rows(ntok, N, dtype, seed + 200)
    pos, valid = np.zeros(ntok, dtype=np.int64), np.zeros(ntok, dtype=bool)
    for b in range(B):
        for j in range(new[b]):
            p = lens[b] - new[b] + j
            if p >= 0:
                pos[sl[b] + j], valid[sl[b] + j] = p, True
    assert pos.max() == rope_len - 1, "the last table row is used"
    qr, kr = RR.apply_rope(q, pos, cos, sin), RR.apply_rope(k, pos, cos, sin)        # (rows that are not valid: position 0, never compared)
    q_want = torch.full((ntok, Nq, 128), FILL, dtype=U8).repeat_interleave(2, dim=-1).view(dtype).clone()
    q_want[torch.from_numpy(valid)] = qr[torch.from_numpy(valid)]
    pages, indptr, indices, last = R.make_tables(lens, P, seed)
    data = np.full((pages, L, 2, N, P, 64), FILL, dtype=np.uint8)
    param = np.full((pages, L, 2, N, P, 4), FILL, dtype=np.uint8).view(np.float16)
    layer = len(name) % L
    kq, kp = R.quantize_i4(kr)
    vq, vp = R.quantize_i4(v)
    R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None if c["new"] is None else sl, layer)
    return dict(P=P, N=N, Nq=Nq, B=B, ntok=ntok, rope_len=rope_len, cos=cos, sin=sin, q=q, k=k, v=v, kr=kr, q_want=q_want, valid=valid,
                tables=(indptr, indices, last), sl=None if c["new"] is None else sl, pages=pages, layer=layer, data=data, param=param)


def _fresh_cache(c):
    data = torch.full((c["pages"], L, 2, c["N"], c["P"], 64), FILL, dtype=U8, device=DEV)
    param = torch.full((c["pages"], L, 2, c["N"], c["P"], 4), FILL, dtype=U8, device=DEV).view(F16)
    return data, param


def _filled(shape, dtype):
    return torch.full(tuple(shape) + (2,), FILL, dtype=U8, device=DEV).view(dtype).squeeze(-1)


def _tabs(c):
    indptr, indices, last = c["tables"]
    return dict(kv_indptr=_dev(indptr), kv_indices=_dev(indices), last_page_offset=_dev(last))


def _write(c, q_out, q, k, v, data, param, tabs):
    cos, sin = c["cos"].to(DEV), c["sin"].to(DEV)
    if c["sl"] is None:
        kvrope.rope_append_kv_quantize_i4(q_out, q, k, v, cos, sin, data, param, **tabs, layer_idx=c["layer"])
    else:
        kvrope.rope_init_kv_quantize_i4(q_out, q, k, v, cos, sin, data, param, **tabs, seqlen_indptr=_dev(c["sl"]), layer_idx=c["layer"])


def _operands(c, sliced):
    """q, k, v on the device: three contiguous tensors, or slices of one [ntok, (Nq + 2 N) * 128] buffer (returned too)."""
    if not sliced:
        return c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV), None
    buf = torch.cat([c["q"], c["k"], c["v"]], dim=1).to(DEV).view(c["ntok"], -1)
    q, k, v = buf.view(c["ntok"], c["Nq"] + 2 * c["N"], 128).split([c["Nq"], c["N"], c["N"]], dim=1)
    assert not q.is_contiguous() or c["ntok"] == 1
    return q, k, v, buf


def _assert_bytes(got, want, what):
    g, w = got.cpu().contiguous().view(U8).reshape(-1), want.contiguous().view(U8).reshape(-1)
    bad = (g != w).nonzero().reshape(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} bytes differ, first at {int(bad[0])}"


@pytest.mark.parametrize("theta", [1e4, 1e6], ids=["theta1e4", "theta1e6"])
@pytest.mark.parametrize("sliced", [False, True], ids=["separate", "sliced"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_rope_write_is_byte_exact(name, dtype, sliced, theta):
    c = _case(name, dtype, theta)
    q, k, v, buf = _operands(c, sliced)
    before = None if buf is None else buf.clone()
    data, param = _fresh_cache(c)
    q_out = _filled((c["ntok"], c["Nq"], 128), dtype)
    tabs = _tabs(c)
    _write(c, q_out, q, k, v, data, param, tabs)
    torch.cuda.synchronize()
    # q_out = apply_rope(q); rows of tokens without a position (an empty sequence, rows beyond seqlen_indptr[B]) keep their fill
    assert c["valid"].all() == (name in ("append-p3", "append-p16")), "the case lost its rows without a position"
    _assert_bytes(q_out, c["q_want"], "q_out")
    # pages and parameters: write_rows(quantize_i4(apply_rope(k)), quantize_i4(v)); every other byte of both layers still 0xA5
    _assert_bytes(data, torch.from_numpy(c["data"]), "kv_data")
    _assert_bytes(param, torch.from_numpy(c["param"]), "kv_param")
    assert int((torch.from_numpy(c["data"]) != FILL).sum()) > 0
    # the inputs are inputs
    if before is not None:
        assert torch.equal(buf, before), "q / k / v modified"
    # the same pages out of the existing writers fed the reference's rotated k
    data2, param2 = _fresh_cache(c)
    kr, vv = c["kr"].to(DEV), c["v"].to(DEV)
    if c["sl"] is None:
        kvcache.append_kv_quantize_i4(data2, param2, **tabs, k=kr, v=vv, layer_idx=c["layer"])
    else:
        kvcache.init_kv_quantize_i4(data2, param2, **tabs, k=kr, v=vv, seqlen_indptr=_dev(c["sl"]), layer_idx=c["layer"])
    torch.cuda.synchronize()
    assert torch.equal(data, data2) and torch.equal(param.view(torch.int16), param2.view(torch.int16))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_q_out_may_be_q_itself(dtype):
    c = _case("append-p3", dtype, 1e4)
    q, k, v, _ = _operands(c, False)
    data, param = _fresh_cache(c)
    _write(c, q, q, k, v, data, param, _tabs(c))
    torch.cuda.synchronize()
    _assert_bytes(q, c["q_want"], "q rotated in place")
    _assert_bytes(data, torch.from_numpy(c["data"]), "kv_data")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_equivalence_with_rope_qk_then_the_existing_writer(dtype):
    """The guarantee of include/arcq_kv.h on the device alone: arcq_rope_qk, then arcq_kv_init_quantize and a copy of q."""
    c = _case("init-p4", dtype, 1e6)
    q, k, v, _ = _operands(c, True)
    tabs, cos, sin = _tabs(c), c["cos"].to(DEV), c["sin"].to(DEV)
    data, param = _fresh_cache(c)
    q_out = _filled((c["ntok"], c["Nq"], 128), dtype)
    _write(c, q_out, q, k, v, data, param, tabs)
    pos = np.zeros(c["ntok"], dtype=np.int32)
    sl, lens = c["sl"], CASES["init-p4"]["lens"]
    for b in range(c["B"]):
        for j in range(sl[b + 1] - sl[b]):
            pos[sl[b] + j] = lens[b] - (sl[b + 1] - sl[b]) + j
    q2, k2 = q.contiguous(), k.contiguous()
    kvrope.rope_qk_(q2, k2, _dev(pos), cos, sin)
    data2, param2 = _fresh_cache(c)
    kvcache.init_kv_quantize_i4(data2, param2, **tabs, k=k2, v=v.contiguous(), seqlen_indptr=_dev(sl), layer_idx=c["layer"])
    torch.cuda.synchronize()
    n = int(sl[-1])
    assert torch.equal(q_out[:n].view(torch.int16), q2[:n].view(torch.int16))
    assert torch.equal(data, data2) and torch.equal(param.view(torch.int16), param2.view(torch.int16))


# ---- rope_qk_
QK = dict(ntok=6, q_len=3, Nq=4, N=2)
QK_POS = {6: (5, 0, 9, 2, 7, 11), 3: (9, 10, 11), 1: (11,)}              # rope_len = 12: the last row is used by each


@pytest.mark.parametrize("k_none", [False, True], ids=["qk", "q-only"])
@pytest.mark.parametrize("n_pos", [6, 3, 1])
@pytest.mark.parametrize("views", [False, True], ids=["contiguous", "views"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_rope_qk_in_place(dtype, views, n_pos, k_none):
    ntok, Nq, N = QK["ntok"], QK["Nq"], QK["N"]
    cos, sin = RR.rope_tables(12, 1e4 if n_pos != 3 else 1e6, dtype)
    q, k, v = RR.rows(ntok, Nq, dtype, 11 + n_pos), RR.rows(ntok, N, dtype, 12 + n_pos), RR.rows(ntok, N, dtype, 13)
    positions = np.array(QK_POS[n_pos], dtype=np.int32)
    per_token = positions[np.arange(ntok) % n_pos]
    want_q, want_k = RR.apply_rope(q, per_token, cos, sin), (k if k_none else RR.apply_rope(k, per_token, cos, sin))
    if views:                  # slices of one buffer whose rows carry 8 spare elements behind v: nothing but the q and k rows may change
        width = (Nq + 2 * N) * 128
        buf = torch.full((ntok, width + 8, 2), FILL, dtype=U8).view(dtype).squeeze(-1)
        buf[:, :width] = torch.cat([q, k, v], dim=1).view(ntok, width)
        buf = buf.to(DEV)
        qd, kd, _ = buf[:, :width].unflatten(1, (Nq + 2 * N, 128)).split([Nq, N, N], dim=1)
        assert qd.stride(0) == width + 8 and not qd.is_contiguous()
    else:
        qd, kd = q.to(DEV), k.to(DEV)
    kvrope.rope_qk_(qd, None if k_none else kd, _dev(positions), cos.to(DEV), sin.to(DEV))
    torch.cuda.synchronize()
    _assert_bytes(qd, want_q, "q")
    _assert_bytes(kd, want_k, "k")
    if views:
        rest = buf.cpu()[:, (Nq + N) * 128:]
        want_rest = torch.full((ntok, N * 128 + 8, 2), FILL, dtype=U8).view(dtype).squeeze(-1)
        want_rest[:, :N * 128] = v.view(ntok, N * 128)
        _assert_bytes(rest, want_rest, "the bytes between the strided rows")


def test_captured_rope_append_replays_to_the_eager_bytes():
    c = _case("append-p3", BF16, 1e6)
    q, k, v, _ = _operands(c, True)
    tabs, cos, sin = _tabs(c), c["cos"].to(DEV), c["sin"].to(DEV)
    data, param = _fresh_cache(c)
    q_out = _filled((c["ntok"], c["Nq"], 128), BF16)

    def step():
        kvrope.rope_append_kv_quantize_i4(q_out, q, k, v, cos, sin, data, param, **tabs, layer_idx=c["layer"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step()
    torch.cuda.synchronize()
    for _ in range(2):
        data.fill_(FILL)
        param.view(U8).fill_(FILL)
        q_out.view(U8).fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        _assert_bytes(q_out, c["q_want"], "q_out (replay)")
        _assert_bytes(data, torch.from_numpy(c["data"]), "kv_data (replay)")
        _assert_bytes(param, torch.from_numpy(c["param"]), "kv_param (replay)")
