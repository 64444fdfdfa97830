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
    ragged odd five single empty empty1   the ragged batches of tests/kv_reference.CASES: a wave streams 3 - 5 blocks, so the new row lands
                        in a buffer the loop has reloaded; T = 1 and T = 2 under S > 1; slices in which all four waves idle; sequences
                        without positions (both spellings), for which the step writes nothing and gives zeros

g = 7 gives two chunks of query heads per kv head, the second with three heads: only chunk 0 may write the row.  g = 2 is the two-head
instantiation, g = 3 one chunk with a repeated, unstored head, g = 8 two full chunks."""
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
RAGGED = ["ragged", "odd", "five", "single", "empty", "empty1"]
CASES = {
    "p16a": (16, lens_for(16)[0], 2, 1), "p16b": (16, lens_for(16)[1], 2, 1), "p5a": (5, lens_for(5)[0], 2, 1), "p5b": (5, lens_for(5)[1], 2, 1),
    "idle": (16, (300, 260), 1, 2), "alone": (16, (257, 289), 1, 2), "long": (16, (1100, 700), 1, 7),
    **{name: (R.CASES[name]["P"], R.CASES[name]["lens"], R.CASES[name]["N"], R.CASES[name]["S"])
       for name in RAGGED},
}
GS = [1, 2, 3, 4, 7, 8]
DTYPES = pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])


def _mods():
    from arcquant_amd import _lib, kvcache, kvstep
    return _lib.lib(), kvcache, kvstep


def _shorter(lens, P, indptr, indices):
    """The tables of the same sequences one position shorter (a sequence of one position becomes empty; one without positions stays as
    it is spelled)."""
    lens0 = [max(n - 1, 0) for n in lens]
    cnt0 = [(n0 + P - 1) // P if n else int(indptr[b + 1] - indptr[b]) for b, (n, n0) in enumerate(zip(lens, lens0))]
    ip0 = np.concatenate([[0], np.cumsum(cnt0)]).astype(np.int32)
    idx0 = np.concatenate([indices[indptr[b]:indptr[b] + cnt0[b]] for b in range(len(lens))]).astype(np.int32)
    last0 = np.array([n0 - (c - 1) * P if n else 0 for n, n0, c in zip(lens, lens0, cnt0)], dtype=np.int32)
    assert (R.seq_lens(ip0, last0, P) == np.asarray(lens0)).all()
    return lens0, ip0, idx0, last0


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """Tables, the earlier positions' rows and a cache (both layers) initialised to lengths - 1, built once and never modified."""
    _, kv, _ = _mods()
    P, lens, n_heads, S = CASES[name]
    B = len(lens)
    pages, indptr, indices, last = R.make_tables(lens, P, seed=len(name) + P, empty_pages=R.CASES.get(name, {}).get("empty_pages", 0))
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


def test_a_case_puts_the_new_row_on_a_reloaded_buffer():
    """The owning wave's last block is its third or later in ragged, five and single: new_row patches a buffer the loop has refilled."""
    for name in ("ragged", "five", "single"):
        P, lens, _, S = CASES[name]
        T = max(lens)
        t0 = [a for a, b in R.wave_ranges(T, S, 32).reshape(-1, 2) if a < b and b == T][0]
        assert (T - 1 - t0) // 32 >= 2, name


@pytest.mark.parametrize("case", ["p16a", "long", "ragged", "odd", "empty", "empty1"])
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
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{case} {dtype} g={g}: max err/bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"max err / bound = {worst}"
    for b, T in enumerate(c["lens"]):
        if T == 0:                                             # (the bound is 0 there: exact zeros)
            assert not o[b].any(), b
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
    _three_calls_on_one_state("long", g, dtype)


@pytest.mark.parametrize("g", GS)
@DTYPES
def test_state_is_handed_back_zeroed_by_a_ragged_batch(g, dtype):
    """The same with slices in which every wave idles and sequences of one and two positions: their workgroups draw tickets as well."""
    _three_calls_on_one_state("ragged", g, dtype)


def _three_calls_on_one_state(case, g, dtype):
    step = _mods()[2]
    c = _case(case, dtype)
    _check_splits(c, g)
    q = _q(c, g, dtype)
    state = step.DecodeStepState(c["B"], g * c["N"], c["N"], DEV)
    assert state.counters.numel() == c["B"] * c["N"] * R.decode_chunks(g)
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


@pytest.mark.parametrize("case", ["p16a", "p5b", "alone", "long", "ragged", "odd"])
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


@pytest.mark.parametrize("case", ["empty", "empty1"])
@pytest.mark.parametrize("g", GS)
@DTYPES
def test_a_sequence_without_positions_is_left_alone(case, g, dtype):
    """Sequences 1 and 3 hold nothing (no pages | one page, last_page_offset 0): their o rows are zero, the counters come back zero, and
    the only bytes of the cache and the parameters that changed are the rows of position T - 1 of the other two, in the layer asked for."""
    step = _mods()[2]
    c = _case(case, dtype)
    _check_splits(c, g)
    assert c["lens"][1] == 0 and c["lens"][3] == 0 and c["S"] > 1
    q, layer = _q(c, g, dtype), 1
    state = step.DecodeStepState(c["B"], g * c["N"], c["N"], DEV)
    o, data, param = _step(c, q, c["k"], c["v"], layer, sliced=True, state=state)
    assert not state.counters.cpu().any(), "counters left non-zero"
    assert not o[1].any() and not o[3].any() and o[0].any() and o[2].any()
    indptr, indices, last = c["np_tables"]
    touched = np.zeros(tuple(c["data"].shape[:5]), dtype=bool)
    for b, T in enumerate(c["lens"]):
        if T:
            page, e = R.locate(indptr, indices, b, T - 1, c["P"])
            touched[page, layer, :, :, e] = True
    keep = torch.from_numpy(~touched)
    assert torch.equal(data[keep], c["data"].cpu()[keep]), "kv_data changed outside the two new rows"
    assert torch.equal(param[keep], _ints(c["param"])[keep]), "kv_param changed outside the two new rows"
    for b in (1, 3):                                           # the page an empty sequence names (empty1) is untouched as a whole
        for page in indices[indptr[b]:indptr[b + 1]]:
            assert torch.equal(data[page], c["data"].cpu()[page]) and torch.equal(param[page], _ints(c["param"])[page])
