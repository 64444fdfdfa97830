"""GPU tests of arcquant_amd.kvcache (include/arcq_kv.h): the four writers byte for byte against the numpy restatement of the format
(tests/kv_reference.py) on a sentinel-filled cache, and the decode attention element-wise against an fp64 attention over the same pages
with a bound computed from the inputs:

    |got - ref| <= u |ref| + (2 Delta + 2^-20) sum_t p_t a_td,   a_td = c_td s_t + |z_t|,   Delta = 130 * 2^-24 * sm_scale * max_t sum_d |q_d| a_td

u = half an ulp of the output dtype (one rounding of the result); the second term is the worst-case fp32 dot-product error of a score
(either algebraic form), carried through the softmax, plus the exp term.  For randn inputs it is ~1e-3 relative; a nibble, page or head
mix-up is O(1).  A length-1 sequence must return the dequantised V row rounded once: exact equality.

The decode cases include the ragged batches of tests/kv_reference.CASES (deep loops, idle slices, T = 1 | 2 under S > 1, sequences without
positions, an over-provisioned table) at every group width, and inputs with controlled scores -- uniform, ramps and the range-edge probes
-- for which one position too few, too many or misplaced is an O(1) error."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16, BF16, U8, I32 = torch.float16, torch.bfloat16, torch.uint8, torch.int32
L, N, B = 2, 2, 3
SENTINEL = 0xA5


def lens_for(P):
    """1, P - 1, P (last_page_offset == P) | P + 1 (an append opens a new page), several pages ending mid-page, 2P (ends at a page's last
    slot): unequal within each batch."""
    return [(1, max(P - 1, 1), P), (P + 1, 3 * P + 2, 2 * P)]


def _kv():
    from arcquant_amd import kvcache
    return kvcache


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(lens, P, seed):
    pages, indptr, indices, last = R.make_tables(lens, P, seed)
    return pages, indptr, indices, last, dict(kv_indptr=_dev(indptr), kv_indices=_dev(indices), last_page_offset=_dev(last))


def _sentinel_cache(pages, P, row, n_heads=N, layers=L):
    data = np.full((pages, layers, 2, n_heads, P, row), SENTINEL, dtype=np.uint8)
    param = np.full((pages, layers, 2, n_heads, P, 2), SENTINEL, dtype=np.uint8)
    return data, param


def _rows(ntok, dtype, seed, n_heads=N, overflow=True):
    """randn * 3 rows with the quantiser's edge rows in front: constant, tiny range, +-65504 (fp16)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(ntok, n_heads, 128, generator=g) * 3).to(dtype)
    flat = x.view(-1, 128)
    flat[0] = 1.5
    if flat.shape[0] > 1:
        flat[1] = torch.linspace(0, 4e-6, 128).to(dtype)
    if dtype is F16 and flat.shape[0] > 4:
        flat[2, 3] = 65504
        flat[3, 7] = -65504
        if overflow:                                          # the range overflows fp16: scale = inf, inf / inf -> code 0
            flat[4, 1], flat[4, 2] = 65504, -65504
    return x


def _append_lens(lens, mode):
    return list(lens) if mode == "all" else [min(n, a) for n, a in zip(lens, (1, 2, 10 ** 9))]


def _check_cache(data_t, param_t, want_data, want_param):
    got_d, got_p = data_t.cpu().numpy().view(np.uint8), param_t.cpu().numpy().view(np.uint8)
    assert np.array_equal(got_d, want_data.view(np.uint8)), f"kv_data: {(got_d != want_data.view(np.uint8)).sum()} bytes differ"
    assert np.array_equal(got_p, want_param.view(np.uint8)), f"kv_param: {(got_p != want_param.view(np.uint8)).sum()} bytes differ"


@pytest.mark.parametrize("P", [16, 5])
@pytest.mark.parametrize("fmt", ["i4", "f16"])
def test_init_and_append_copy_rows(P, fmt):
    """init_kv_* (whole sequences and the last few positions only) and append_kv_*: the cache equals the reference's byte for byte, so the
    right rows changed and no others."""
    kv = _kv()
    row = 64 if fmt == "i4" else 256
    init, append = (kv.init_kv_i4, kv.append_kv_i4) if fmt == "i4" else (kv.init_kv_f16, kv.append_kv_f16)
    for li, lens in enumerate(lens_for(P)):
        for layer in range(L):
            pages, indptr, indices, last, tab = _tables(lens, P, 10 * li + layer)
            for mode in ("all", "tail"):
                new = _append_lens(lens, mode)
                sl = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
                ntok = int(sl[-1]) + 2                                       # (rows past seqlen_indptr[B] belong to no sequence)
                rng = np.random.default_rng(ntok + P)
                k, v = rng.integers(0, 256, (ntok, N, row), dtype=np.uint8), rng.integers(0, 256, (ntok, N, row), dtype=np.uint8)
                kp, vp = rng.integers(0, 256, (ntok, N, 4), dtype=np.uint8), rng.integers(0, 256, (ntok, N, 4), dtype=np.uint8)
                d4, _ = _sentinel_cache(pages, P, row)
                p4 = np.full((pages, L, 2, N, P, 4), SENTINEL, dtype=np.uint8)         # (scale, zero) as 4 raw bytes
                R.write_rows(d4, p4, indptr, indices, last, k, v, kp, vp, sl, layer)
                dt, pt = _cache_tensors(pages, P, fmt)
                init(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], _as(k, fmt), _as(v, fmt), _dev(kp).view(F16),
                     _dev(vp).view(F16), _dev(sl), layer)
                _check_cache(dt, pt, d4, p4)
            # append: one token per sequence at seq_len - 1
            rng = np.random.default_rng(P + li)
            k, v = rng.integers(0, 256, (B, N, row), dtype=np.uint8), rng.integers(0, 256, (B, N, row), dtype=np.uint8)
            kp, vp = rng.integers(0, 256, (B, N, 4), dtype=np.uint8), rng.integers(0, 256, (B, N, 4), dtype=np.uint8)
            d4, _ = _sentinel_cache(pages, P, row)
            p4 = np.full((pages, L, 2, N, P, 4), SENTINEL, dtype=np.uint8)
            R.write_rows(d4, p4, indptr, indices, last, k, v, kp, vp, None, layer)
            dt, pt = _cache_tensors(pages, P, fmt)
            append(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], _as(k, fmt), _as(v, fmt), _dev(kp).view(F16), _dev(vp).view(F16),
                   layer)
            _check_cache(dt, pt, d4, p4)


def _cache_tensors(pages, P, fmt, n_heads=N, layers=L):
    data = torch.full((pages, layers, 2, n_heads, P, 64 if fmt == "i4" else 256), SENTINEL, dtype=U8, device=DEV)
    param = torch.full((pages, layers, 2, n_heads, P, 4), SENTINEL, dtype=U8, device=DEV).view(F16)
    return (data if fmt == "i4" else data.view(F16)), param


def _as(a, fmt):
    t = _dev(a)
    return t if fmt == "i4" else t.view(F16)


@pytest.mark.parametrize("P", [16, 5])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_quantising_writers_are_byte_exact(P, dtype):
    """append_kv_quantize_i4 and init_kv_quantize_i4 against the torch formula on a CPU tensor of the input dtype + the reference writer:
    randn * 3 rows, the constant row, the tiny-range row and (fp16) rows holding 65504, -65504 and both."""
    kv = _kv()
    for li, lens in enumerate(lens_for(P)):
        for layer in range(L):
            pages, indptr, indices, last, tab = _tables(lens, P, 20 * li + layer)
            for mode in ("all", "tail", "append"):
                new = [1] * B if mode == "append" else _append_lens(lens, mode)
                sl = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
                ntok = int(sl[-1]) + (0 if mode == "append" else 1)
                k, v = _rows(ntok, dtype, 3 * ntok + P), _rows(ntok, dtype, 5 * ntok + P).flip(0).contiguous()
                (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
                d4, _ = _sentinel_cache(pages, P, 64)
                p4 = np.full((pages, L, 2, N, P, 2), 0, dtype=np.float16)
                p4.view(np.uint8)[...] = SENTINEL
                R.write_rows(d4, p4, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None if mode == "append" else sl, layer)
                dt, pt = _cache_tensors(pages, P, "i4")
                if mode == "append":
                    kv.append_kv_quantize_i4(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], k.to(DEV), v.to(DEV), layer)
                else:
                    kv.init_kv_quantize_i4(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], k.to(DEV), v.to(DEV), _dev(sl), layer)
                _check_cache(dt, pt, d4, p4)


# ---- decode
#   name: P, lens, kv heads, slices per sequence S (kv_decode_splits; asserted through arcq_kv_decode_workspace_bytes), and for the ragged
#   cases of tests/kv_reference.py (what each reaches: there and DESIGN.md 11) empty_pages / pad of the tables
DECODE_CASES = {
    "p16a": dict(P=16, lens=lens_for(16)[0], N=N, S=1), "p16b": dict(P=16, lens=lens_for(16)[1], N=N, S=1),
    "p5a": dict(P=5, lens=lens_for(5)[0], N=N, S=1), "p5b": dict(P=5, lens=lens_for(5)[1], N=N, S=1),
    "long": dict(P=16, lens=(1100, 700), N=1, S=7),   # B = 2, N = 1: every split-and-merge path (slices per sequence, waves per slice, the combine)
    **R.CASES,
}
GS = list(R.G_ALL)
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


def _check_splits(B, Nq, n_heads, nnz, P, S):
    from arcquant_amd import _lib
    want = 0 if S == 1 else B * Nq * S * 130 * 4
    assert _lib.lib().arcq_kv_decode_workspace_bytes(B, Nq, n_heads, nnz, P) == want, "the slice count of this case changed"


@functools.lru_cache(maxsize=None)
def _decode_pages(case, fmt, dtype):
    """Cache contents of one case (quantised randn * 3 rows), built once and shared by every g (nothing below modifies them)."""
    spec = DECODE_CASES[case]
    P, lens, n_heads = spec["P"], spec["lens"], spec["N"]
    layer = 1
    # the path a ragged case claims: blocks the busiest wave streams (the rest of the claims: tests/test_kv_reference.py, without a GPU)
    assert "per" not in spec or R.blocks_per_wave(max(lens), spec["S"], 32) == spec["per"]
    pages, indptr, indices, last = R.case_tables(spec, seed=len(case) + P)
    gen = torch.Generator().manual_seed(P + sum(lens))
    ntok = sum(lens)
    sl = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k, v = (torch.randn(ntok, n_heads, 128, generator=gen) * 3).to(dtype), (torch.randn(ntok, n_heads, 128, generator=gen) * 3).to(dtype)
    param = np.zeros((pages, L, 2, n_heads, P, 2), dtype=np.float16)
    param.view(np.uint8)[...] = SENTINEL
    if fmt == "i4":
        (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
        data = np.full((pages, L, 2, n_heads, P, 64), SENTINEL, dtype=np.uint8)
        R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), sl, layer)
        data_t = _dev(data)
    else:
        data = np.full((pages, L, 2, n_heads, P, 128), np.nan)
        ones = np.ones((ntok, n_heads, 2), dtype=np.float16)
        R.write_rows(data, param, indptr, indices, last, k.double().numpy(), v.double().numpy(), ones, ones, sl, layer)
        data_t = torch.from_numpy(data).to(dtype).to(DEV)                # (the unwritten rows stay NaN: reading one is loud)
    return dict(P=P, lens=lens, N=n_heads, S=spec["S"], layer=layer, data=data_t, param=_dev(param), indptr=_dev(indptr), indices=_dev(indices),
                last=_dev(last), first_v=(v[0] if fmt != "i4" else None), np_tables=(indptr, indices, last), np_data=data, np_param=param,
                gen_state=gen.get_state())


@functools.lru_cache(maxsize=None)
def _decode_case(case, fmt, dtype, g):
    """The pages of a case + q and the fp64 reference for g query heads per kv head."""
    c = _decode_pages(case, fmt, dtype)
    gen = torch.Generator()
    gen.set_state(c["gen_state"])
    q = torch.randn(len(c["lens"]), g * c["N"], 128, generator=gen).to(dtype)
    ref, (spa, qa) = R.paged_attention_f64(q.double().numpy(), c["np_data"], c["np_param"], *c["np_tables"], c["layer"], i4=fmt == "i4")
    return dict(c, q=q.to(DEV), ref=ref, spa=spa, qa=qa)


def _decode(c, fmt, dtype):
    kv = _kv()
    B, Nq = c["q"].shape[:2]
    _check_splits(B, Nq, c["N"], c["indices"].numel(), c["P"], c["S"])
    o = torch.full_like(c["q"], float("nan"))
    fn = kv.batch_decode_i4 if fmt == "i4" else kv.batch_decode_f16
    fn(o, c["q"], c["data"], c["param"], c["indptr"], c["indices"], c["last"], c["layer"])
    return o


def _ratio(got, c, u, n=0):
    """max |got - ref| / bound; an element whose bound is 0 (a sequence without positions) must be exactly the reference's."""
    err, bound = np.abs(got - c["ref"]), R.decode_bound(c["ref"], c["spa"], c["qa"], u, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max()), float(err.max())


@pytest.mark.parametrize("case", list(DECODE_CASES))
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fmt", ["i4", "16bit"])
def test_batch_decode_within_the_fp32_bound(case, g, dtype, fmt):
    c = _decode_case(case, fmt, dtype, g)
    o = _decode(c, fmt, dtype)
    got = o.double().cpu().numpy()
    bound = R.decode_bound(c["ref"], c["spa"], c["qa"], U[dtype])
    err = np.abs(got - c["ref"])
    worst = _ratio(got, c, U[dtype])[0]
    print(f"{case} {fmt} {dtype} g={g}: max err/bound = {worst:.3f}, max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"max err / bound = {worst}"
    n_heads = c["N"]
    for b, T in enumerate(c["lens"]):
        if T == 0:                                             # a sequence without positions: zeros (the bound is 0 there as well)
            assert not o[b].cpu().view(torch.int16).any(), b
        # a length-1 sequence: the dequantised V row (the 16-bit cache: the V row itself), rounded once
        if T != 1:
            continue
        for h in range(g * n_heads):
            if fmt == "i4":
                vr, vp = R.gather_rows(c["np_data"], c["np_param"], *c["np_tables"], c["layer"], b, h // g, 1)
                want = torch.from_numpy(R.dequantize_f32(vr, vp)[0]).to(dtype)
            else:
                vr, _ = R.gather_rows(c["np_data"], c["np_param"], *c["np_tables"], c["layer"], b, h // g, 1)
                want = torch.from_numpy(vr[0]).to(dtype)
                assert b != 0 or torch.equal(want, c["first_v"][h // g])
            assert torch.equal(o[b, h].cpu(), want), (b, h)


def _upload(c, fmt, dtype):
    data = _dev(c["data"]) if fmt == "i4" else torch.from_numpy(c["data"]).to(dtype).to(DEV)
    indptr, indices, last = c["tables"]
    return dict(P=c["P"], N=c["N"], S=c["S"], layer=c["layer"], data=data, param=_dev(c["param"]), indptr=_dev(indptr), indices=_dev(indices),
                last=_dev(last), q=torch.from_numpy(c["q"]).to(dtype).to(DEV))


@pytest.mark.parametrize("case", ["ragged", "odd", "single"])
@pytest.mark.parametrize("profile", ["uniform", "ramp_up", "ramp_down"])
@pytest.mark.parametrize("g", [2, 7])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fmt", ["i4", "16bit"])
def test_batch_decode_controlled_scores(case, profile, g, dtype, fmt):
    """The cache written from codes and (scale, zero) pairs (tests/kv_reference.profile_rows).  uniform: q = 0, every position weighs
    1 / T and the bound is the rounding of o plus the accumulation term alone (kv_reference.accumulation_chain, derived from the kernel's
    structure), so one position too few or too many is hundreds of bounds away (tests/test_kv_reference.py).  ramps: the scores rise
    (every block raises the running maximum and rescales l, the zero sum and the accumulators) or fall (the far blocks underflow)."""
    c = R.profile_case(case, profile, fmt == "i4", dtype, g)
    assert torch.equal(torch.from_numpy(c["q"]).to(dtype).double(), torch.from_numpy(c["q"]))
    got = _decode(_upload(c, fmt, dtype), fmt, dtype).double().cpu().numpy()
    n = c["n"] if profile == "uniform" else 0
    worst, err = _ratio(got, c, U[dtype], n)
    print(f"{case} {profile} {fmt} {dtype} g={g}: max err/bound = {worst:.3f} (without the accumulation term: {_ratio(got, c, U[dtype])[0]:.3f}), "
          f"max |err| = {err:.3e}")
    assert np.isfinite(got).all()
    assert worst <= 1.0, f"max err / bound = {worst}"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("fmt", ["i4", "16bit"])
def test_batch_decode_range_edge_probes(dtype, fmt):
    """One launch: ten sequences that name the same pages, seven query heads each, every (sequence, head) a spike at another position --
    every multiple of the block, the position before each, 0, T - 2, T - 1 -- whose fp64 score leads by more than 30, so o is the
    target's dequantised V row and a dropped, masked or misaddressed row at any wave-range or block edge is an O(1) error."""
    c = R.probe_case(fmt == "i4", dtype)
    assert R.spike_gap(c) >= 30.0
    edges = set(R.wave_ranges(c["T"], c["S"], c["block"]).reshape(-1).tolist()) - {c["T"]}
    targets = set(c["targets"].reshape(-1).tolist())
    assert edges <= targets and {e - 1 for e in edges if e} <= targets and {0, c["T"] - 2, c["T"] - 1} <= targets
    o = _decode(_upload(c, fmt, dtype), fmt, dtype)
    got = o.double().cpu().numpy()
    worst, err = _ratio(got, c, U[dtype])
    want = torch.from_numpy(c["want"]).to(dtype)
    exact = int((o.cpu().view(torch.int16) == want.view(torch.int16)).all(-1).sum())
    print(f"probes {fmt} {dtype}: S = {c['S']}, max err/bound = {worst:.3f}, max |err| = {err:.3e}, {exact} of {want.shape[0] * want.shape[1]} rows "
          f"equal the target's V row bit for bit")
    assert np.abs(c["ref"] - c["want"]).max() < 1e-9
    assert np.isfinite(got).all()
    assert worst <= 1.0, f"max err / bound = {worst}"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_fused_quantising_append_equals_the_torch_flow(dtype):
    """append_kv_quantize_i4 + batch_decode_i4 == the torch quantiser + append_kv_i4 + batch_decode_i4, bit for bit (cache and output)."""
    kv = _kv()
    P, lens, layer = 5, lens_for(5)[1], 0
    pages, indptr, indices, last, tab = _tables(lens, P, 77)
    gen = torch.Generator().manual_seed(5)
    sl = np.concatenate([[0], np.cumsum([n - 1 for n in lens])]).astype(np.int32)
    past = (torch.randn(int(sl[-1]), N, 128, generator=gen) * 3).to(dtype)
    k, v = _rows(B, dtype, 11, overflow=False), (torch.randn(B, N, 128, generator=gen) * 3).to(dtype)     # (a NaN's cast to uint8 is the platform's)
    q = torch.randn(B, 4 * N, 128, generator=gen).to(dtype).to(DEV)
    outs, caches = [], []
    for fused in (True, False):
        dt, pt = _cache_tensors(pages, P, "i4")
        # the earlier positions: tables of the sequences one token shorter
        lens0 = [n - 1 for n in lens]
        cnt0 = [(n + P - 1) // P for n in lens0]
        ip0 = np.concatenate([[0], np.cumsum(cnt0)]).astype(np.int32)
        idx0 = np.concatenate([indices[indptr[b]:indptr[b] + cnt0[b]] for b in range(B)]).astype(np.int32)
        last0 = np.array([n - (c - 1) * P for n, c in zip(lens0, cnt0)], dtype=np.int32)
        kv.init_kv_quantize_i4(dt, pt, _dev(ip0), _dev(idx0), _dev(last0), past.to(DEV), past.flip(0).contiguous().to(DEV), _dev(sl), layer)
        if fused:
            kv.append_kv_quantize_i4(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], k.to(DEV), v.to(DEV), layer)
        else:
            kq, ks, kz = kv.asym_quantize_and_pack_i4(k)
            vq, vs, vz = kv.asym_quantize_and_pack_i4(v)
            kp, vp = torch.cat([ks, kz], -1).to(F16), torch.cat([vs, vz], -1).to(F16)
            kv.append_kv_i4(dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], kq.to(DEV), vq.to(DEV), kp.to(DEV), vp.to(DEV), layer)
        o = torch.empty_like(q)
        kv.batch_decode_i4(o, q, dt, pt, tab["kv_indptr"], tab["kv_indices"], tab["last_page_offset"], layer)
        outs.append(o.view(torch.int16).cpu())
        caches.append((dt.cpu(), pt.view(torch.int16).cpu()))
    assert torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1])
    assert torch.equal(outs[0], outs[1])
