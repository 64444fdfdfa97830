"""GPU tests of arcquant_amd.kvstep.decode_step_i4 (include/arcq_kv.h arcq_kv_decode_step): the one-launch decode step must leave the
pages, the parameters and ``o`` exactly as append_kv_quantize_i4 + batch_decode_i4 leave them (compared as integers), must equal the
numpy restatement of the format (tests/kv_reference.py) on a sentinel-filled cache and lie within the fp32 bound of
tests/test_kvcache_gpu.py of an fp64 attention over those pages, must hand its counters back zeroed, and must not depend on what the page
held at the position it writes.

All lengths include the new token.  The slice counts S follow from the launcher's heuristic and are asserted through
arcq_kv_decode_workspace_bytes, so a change of it is noticed here:

    p16a p16b p5a p5b   S = 1   T = 1; the step opens a new page (P + 1); the step lands on a page's last slot (P, 2P)
    idle  (300, 260)    S = 2   idle waves; the wave that owns T - 1 is not the last wave
    alone (257, 289)    S = 2   the owning wave's range is the new position alone: it reads nothing from the page
    long  (1100, 700)   S = 7

g = 7 gives two chunks of query heads per kv head, the second with three heads: only chunk 0 may write the row."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_reference as R
from tests.test_kvcache_gpu import SENTINEL, _cache_tensors, _dev, _rows, lens_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
L = 2
CASES = {
    "p16a": (16, lens_for(16)[0], 2, 1), "p16b": (16, lens_for(16)[1], 2, 1), "p5a": (5, lens_for(5)[0], 2, 1), "p5b": (5, lens_for(5)[1], 2, 1),
    "idle": (16, (300, 260), 1, 2), "alone": (16, (257, 289), 1, 2), "long": (16, (1100, 700), 1, 7),
}
GS = [1, 4, 7]
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])


def _mods():
    from arcquant_amd import _lib, kvcache, kvstep
    return _lib.lib(), kvcache, kvstep


def _shorter(lens, P, indptr, indices):
    """The tables of the same sequences one position shorter (a sequence of one position becomes empty)."""
    lens0 = [n - 1 for n in lens]
    cnt0 = [(n + P - 1) // P for n in lens0]
    ip0 = np.concatenate([[0], np.cumsum(cnt0)]).astype(np.int32)
    idx0 = np.concatenate([indices[indptr[b]:indptr[b] + cnt0[b]] for b in range(len(lens))]).astype(np.int32)
    last0 = np.array([n - (c - 1) * P for n, c in zip(lens0, cnt0)], dtype=np.int32)
    assert (R.seq_lens(ip0, last0, P) == np.asarray(lens0)).all()
    return lens0, ip0, idx0, last0


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """Tables, the earlier positions' rows and a cache (both layers) initialised to lengths - 1, built once and never modified."""
    _, kv, _ = _mods()
    P, lens, n_heads, S = CASES[name]
    B = len(lens)
    pages, indptr, indices, last = R.make_tables(lens, P, seed=len(name) + P)
    lens0, ip0, idx0, last0 = _shorter(lens, P, indptr, indices)
    gen = torch.Generator().manual_seed(P + sum(lens))
    sl0 = np.concatenate([[0], np.cumsum(lens0)]).astype(np.int32)
    past_k = (torch.randn(L, int(sl0[-1]), n_heads, 128, generator=gen) * 3).to(dtype)
    past_v = (torch.randn(L, int(sl0[-1]), n_heads, 128, generator=gen) * 3).to(dtype)
    data, param = _cache_tensors(pages, P, "i4", n_heads, L)
    for layer in range(L):
        kv.init_kv_quantize_i4(data, param, _dev(ip0), _dev(idx0), _dev(last0), past_k[layer].to(DEV), past_v[layer].to(DEV), _dev(sl0), layer)
    # this token's rows: the quantiser's edge rows (constant, tiny range, +-65504 in fp16) among them, without the overflowing one
    k = _rows(B, dtype, 11 + P, n_heads, overflow=False)
    v = (torch.randn(B, n_heads, 128, generator=gen) * 3).to(dtype)
    return dict(P=P, lens=lens, N=n_heads, S=S, B=B, pages=pages, np_tables=(indptr, indices, last), np_tables0=(ip0, idx0, last0), sl0=sl0,
                tab=dict(kv_indptr=_dev(indptr), kv_indices=_dev(indices), last_page_offset=_dev(last)), nnz=len(indices),
                data=data, param=param, past_k=past_k, past_v=past_v, k=k, v=v, gen_seed=P + sum(lens))


def _q(c, g, dtype):
    gen = torch.Generator().manual_seed(c["gen_seed"] + g)
    return torch.randn(c["B"], g * c["N"], 128, generator=gen).to(dtype)


def _check_splits(c, g):
    lib = _mods()[0]
    Nq = g * c["N"]
    want = 0 if c["S"] == 1 else c["B"] * Nq * c["S"] * 130 * 4
    assert lib.arcq_kv_decode_workspace_bytes(c["B"], Nq, c["N"], c["nnz"], c["P"]) == want, "the slice count of this case changed"


def _ints(t):
    return t.contiguous().view(torch.int16).cpu()


def _chain(c, q, k, v, layer):
    """append_kv_quantize_i4 + batch_decode_i4 on a copy of the case's cache -> (o, data, param) as integers."""
    kv = _mods()[1]
    data, param = c["data"].clone(), c["param"].clone()
    kv.append_kv_quantize_i4(data, param, **c["tab"], k=k.to(DEV), v=v.to(DEV), layer_idx=layer)
    o = torch.full(q.shape, float("nan"), dtype=q.dtype, device=DEV)
    kv.batch_decode_i4(o, q.to(DEV), data, param, **c["tab"], layer_idx=layer)
    return _ints(o), data.cpu(), _ints(param)


def _sliced(q, k, v):
    """q, k, v as slices of one [B, (Nq + 2 N) * 128] buffer on the device."""
    B, Nq, N = q.shape[0], q.shape[1], k.shape[1]
    buf = torch.cat([q, k, v], dim=1).to(DEV).reshape(B, (Nq + 2 * N) * 128)
    qq, kk, vv = buf.view(B, Nq + 2 * N, 128).split([Nq, N, N], dim=1)
    assert qq.stride(0) == (Nq + 2 * N) * 128 and kk.data_ptr() == buf.data_ptr() + Nq * 256
    return qq, kk, vv


def _step(c, q, k, v, layer, sliced=False, state=None, data=None, param=None):
    step = _mods()[2]
    data, param = (c["data"].clone(), c["param"].clone()) if data is None else (data, param)
    qq, kk, vv = _sliced(q, k, v) if sliced else (q.to(DEV), k.to(DEV), v.to(DEV))
    o = torch.full(q.shape, float("nan"), dtype=q.dtype, device=DEV)
    step.decode_step_i4(o, qq, kk, vv, data, param, **c["tab"], layer_idx=layer, state=state)
    return _ints(o), data.cpu(), _ints(param)


def _same(got, want, what):
    for a, b, name in zip(got, want, ("o", "kv_data", "kv_param")):
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} places"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("g", GS)
@DTYPES
def test_step_equals_the_chain_bit_for_bit(case, g, dtype):
    c = _case(case, dtype)
    _check_splits(c, g)
    q, layer = _q(c, g, dtype), 1
    want = _chain(c, q, c["k"], c["v"], layer)
    _same(_step(c, q, c["k"], c["v"], layer), want, "contiguous q, k, v")
    _same(_step(c, q, c["k"], c["v"], layer, sliced=True), want, "slices of one projection output")


@pytest.mark.parametrize("case", ["p16a", "long"])
@pytest.mark.parametrize("g", GS)
@DTYPES
def test_step_against_the_references(case, g, dtype):
    """Pages: R.quantize_i4 + R.write_rows on a sentinel-filled cache (the right rows changed and no others).  o: within R.decode_bound of
    the fp64 attention over those pages; a sequence of one position gives the dequantised new V row rounded once, exactly."""
    c = _case(case, dtype)
    _check_splits(c, g)
    P, n_heads, B, layer = c["P"], c["N"], c["B"], 1
    data = np.full((c["pages"], L, 2, n_heads, P, 64), SENTINEL, dtype=np.uint8)
    param = np.zeros((c["pages"], L, 2, n_heads, P, 2), dtype=np.float16)
    param.view(np.uint8)[...] = SENTINEL
    for ly in range(L):
        (kq, kp), (vq, vp) = R.quantize_i4(c["past_k"][ly]), R.quantize_i4(c["past_v"][ly])
        R.write_rows(data, param, *c["np_tables0"], kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), c["sl0"], ly)
    (kq, kp), (vq, vp) = R.quantize_i4(c["k"]), R.quantize_i4(c["v"])
    R.write_rows(data, param, *c["np_tables"], kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None, layer)
    q = _q(c, g, dtype)
    o, got_d, got_p = _step(c, q, c["k"], c["v"], layer, sliced=True)
    assert np.array_equal(got_d.numpy(), data), f"kv_data: {(got_d.numpy() != data).sum()} bytes differ"
    assert np.array_equal(got_p.numpy().view(np.uint16), param.view(np.uint16).reshape(got_p.shape)), "kv_param differs"
    ref, (spa, qa) = R.paged_attention_f64(q.double().numpy(), data, param, *c["np_tables"], layer)
    got = o.view(dtype).double().numpy()
    bound = R.decode_bound(ref, spa, qa, 2.0 ** -11 if dtype is F16 else 2.0 ** -8)
    err = np.abs(got - ref)
    print(f"{case} {dtype} g={g}: max err/bound = {float((err / bound).max()):.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"max err / bound = {float((err / bound).max())}"
    for b, T in enumerate(c["lens"]):
        if T != 1:
            continue
        for h in range(g * n_heads):
            want = torch.from_numpy(R.dequantize_f32(vq[b, h // g].numpy()[None], vp[b, h // g].numpy()[None])[0]).to(dtype)
            assert torch.equal(o.view(dtype)[b, h], want), (b, h)
    assert case != "p16a" or 1 in c["lens"]


@pytest.mark.parametrize("g", GS)
@DTYPES
def test_state_is_handed_back_zeroed(g, dtype):
    """One DecodeStepState through three calls: all zero after each, a repeated call gives the same bits (the append is idempotent), and
    a call on another layer matches that layer's chain."""
    step = _mods()[2]
    c = _case("long", dtype)
    _check_splits(c, g)
    q = _q(c, g, dtype)
    state = step.DecodeStepState(c["B"], g * c["N"], c["N"], DEV)
    assert state.counters.numel() == c["B"] * c["N"] * (2 if g == 7 else 1)
    data, param = c["data"].clone(), c["param"].clone()
    first = _step(c, q, c["k"], c["v"], 1, sliced=True, state=state, data=data, param=param)
    assert not state.counters.cpu().any(), "counters left non-zero"
    _same(first, _chain(c, q, c["k"], c["v"], 1), "first call")
    second = _step(c, q, c["k"], c["v"], 1, sliced=True, state=state, data=data, param=param)
    assert not state.counters.cpu().any()
    _same(second, first, "second call, same state and inputs")
    third = _step(c, q, c["v"], c["k"], 0, state=state)
    assert not state.counters.cpu().any()
    _same(third, _chain(c, q, c["v"], c["k"], 0), "third call, another layer")


@pytest.mark.parametrize("case", ["p16a", "p5b", "alone", "long"])
@pytest.mark.parametrize("g", GS)
@DTYPES
def test_result_does_not_depend_on_the_old_row(case, g, dtype):
    """Position T - 1 of the pages -- codes and parameters, K and V, every head -- filled with 0x00, 0xFF and 0x7F before the call."""
    c = _case(case, dtype)
    q, layer = _q(c, g, dtype), 1
    indptr, indices, last = c["np_tables"]
    runs = []
    for fill in (0x00, 0xFF, 0x7F):
        data, param = c["data"].clone(), c["param"].clone()
        for b, T in enumerate(c["lens"]):
            page, e = R.locate(indptr, indices, b, T - 1, c["P"])
            data[page, layer, :, :, e] = fill
            param.view(torch.uint8)[page, layer, :, :, e] = fill
        runs.append(_step(c, q, c["k"], c["v"], layer, data=data, param=param))
    _same(runs[1], runs[0], "0xFF against 0x00")
    _same(runs[2], runs[0], "0x7F against 0x00")
    _same(runs[0], _chain(c, q, c["k"], c["v"], layer), "against the chain")
