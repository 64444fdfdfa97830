"""CPU tests of tests/kv_reference.py, the restatement of the paged KV-cache format the GPU tests compare with: nibble order, the offset
formulas of page.cuh against a brute-force 6-D index, and the quantiser's edge rows, settled against torch itself."""
import numpy as np
import pytest
import torch

from arcquant_amd import kvcache
from tests import kv_reference as R


def test_pack_unpack_roundtrip_and_nibble_order():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, size=(5, 3, 128), dtype=np.uint8)
    packed = R.pack_codes(codes)
    assert packed.shape == (5, 3, 64) and np.array_equal(R.unpack_codes(packed), codes)
    one = np.zeros(128, dtype=np.uint8)
    one[6], one[7] = 3, 9                                   # byte 3: element 6 low, element 7 high
    assert R.pack_codes(one)[3] == 0x93 and R.pack_codes(one).sum() == 0x93
    # the library's torch pair agrees with the numpy one
    q = torch.from_numpy(packed)
    s, z = torch.full((5, 3, 1), 0.5, dtype=torch.float16), torch.full((5, 3, 1), 2.0, dtype=torch.float16)
    want = R.dequantize_f32(packed, torch.cat([s, z], -1).numpy())
    assert np.array_equal(kvcache.unpack_i4_and_asym_dequantize(q, s.float(), z.float()).numpy(), want)


@pytest.mark.parametrize("row", [64, 128, 2])
def test_offsets_match_a_brute_force_index(row):
    pages, L, N, P = 3, 2, 3, 5
    flat = np.arange(pages * L * 2 * N * P * row).reshape(pages, L, 2, N, P, row)
    for page in range(pages):
        for layer in range(L):
            for head in range(N):
                for e in (0, 1, P - 1):
                    for f in (0, row - 1):
                        assert R.k_elem_offset(page, head, e, f, L, layer, N, P, row) == flat[page, layer, 0, head, e, f]
                        assert R.v_elem_offset(page, head, e, f, L, layer, N, P, row) == flat[page, layer, 1, head, e, f]


def test_sequence_lengths_and_locate():
    P = 5
    indptr, indices, last = [0, 1, 3, 6], [4, 0, 2, 5, 1, 3], [5, 1, 3]
    assert R.seq_lens(indptr, last, P).tolist() == [5, 6, 13]
    assert R.locate(indptr, indices, 1, 5, P) == (2, 0) and R.locate(indptr, indices, 2, 12, P) == (3, 2) and R.locate(indptr, indices, 0, 4, P) == (4, 4)


def _edge_rows(dtype):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(64, 128, generator=g) * 3).to(dtype)
    x[0] = 1.5                                               # constant row: range 0 -> clamp
    x[1] = 0
    x[2] = torch.linspace(0, 4e-6, 128).to(dtype)            # range below 1e-5
    x[3] = 1.0
    x[3, 5] = 1.0 + (2.0 ** -10 if dtype is torch.float16 else 2.0 ** -7)       # one ulp of range
    if dtype is torch.float16:
        x[4, 3], x[5, 7] = 65504, -65504
        x[6, 1], x[6, 2] = 65504, -65504                     # the range overflows fp16: scale = inf
    return x


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantiser_edge_rows_against_torch(dtype):
    """The rule is what torch computes; the stepwise form (every operation rounded to the input dtype, the Scalar 1e-5 included) is what
    the kernel implements.  They agree byte for byte, the degenerate rows included, and so does the library's torch quantiser."""
    x = _edge_rows(dtype)
    packed, param = R.quantize_i4(x)
    packed2, param2 = R.quantize_i4_stepwise(x)
    assert torch.equal(packed, packed2)
    assert torch.equal(param.view(torch.int16), param2.view(torch.int16))
    ours, scale, zero = kvcache.asym_quantize_and_pack_i4(x)
    finite = torch.isfinite(scale[:, 0])                     # (a NaN's cast to uint8 is the platform's; the reference defines it as 0)
    assert torch.equal(ours[finite], packed[finite]) and torch.equal(torch.cat([scale, zero], -1).to(torch.float16).view(torch.int16), param.view(torch.int16))
    # constant row: the clamp decides -- scale = dtype(1e-5) / 15, every code 0
    assert packed[0].eq(0).all() and float(param[0, 0]) > 0 and float(param[0, 1]) == -1.5
    # a range below 1e-5 is quantised with the clamped scale: codes stay below 15
    assert int(R.unpack_codes(packed[2].numpy()).max()) < 15
    assert float(param[2, 0]) == float(param[0, 0])
    # an ordinary row reaches both ends
    c = R.unpack_codes(packed[10].numpy())
    assert c.min() == 0 and c.max() == 15
    # round trip error of an ordinary row: half a step
    back = R.dequantize_f32(packed[10].numpy(), param[10].numpy())
    step = float(param[10, 0])
    assert np.abs(back - x[10].float().numpy()).max() <= 0.5 * step * 1.02 + 2.0 ** -7 * float(x[10].abs().max())


def test_writers_and_attention_walk_the_tables():
    """write_rows places the last tokens of a sequence; the fp64 attention over one position returns the dequantised V row."""
    P, L, N = 5, 2, 2
    data = np.full((4, L, 2, N, P, 64), 0xEE, dtype=np.uint8)
    param = np.full((4, L, 2, N, P, 2), 7.0, dtype=np.float16)
    indptr, indices, last = np.array([0, 2, 3]), np.array([3, 1, 0]), np.array([2, 1])
    x = (torch.randn(4, N, 128) * 3).to(torch.float16)
    kq, kp = R.quantize_i4(x)
    vq, vp = R.quantize_i4(-x)
    written = R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), np.array([0, 3, 4]), 1)
    assert written == [(3, 4), (1, 0), (1, 1), (0, 0)]       # sequence 0: positions 4, 5, 6 of 7; sequence 1: position 0
    assert (data[:, 0] == 0xEE).all() and (data[2] == 0xEE).all() and (data[0, 1, :, :, 1:] == 0xEE).all()
    q = np.random.default_rng(1).standard_normal((2, 2 * N, 128))
    out, (spa, qa) = R.paged_attention_f64(q, data, param, indptr, indices, last, 1)
    want = R.dequantize_f32(vq[3].numpy(), vp[3].numpy()).astype(np.float64)
    assert np.array_equal(out[1, 0], want[0]) and np.array_equal(out[1, 1], want[0]) and np.array_equal(out[1, 3], want[1])
    assert (R.decode_bound(out, spa, qa, 2.0 ** -11) > 0).all()


# ---- the partition restated, the ragged cases, the input profiles: everything the GPU tests of decode lean on, checked without a GPU
F16, BF16 = torch.float16, torch.bfloat16
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


@pytest.mark.parametrize("empty_pages", [0, 1])
def test_a_sequence_without_positions_gives_zeros(empty_pages):
    """Both spellings of include/arcq_kv.h: no pages | one page, last_page_offset 0.  Rows of zeros, bound terms of zero."""
    P, lens = 5, (7, 0, 3, 0)
    pages, indptr, indices, last = R.make_tables(lens, P, seed=1, empty_pages=empty_pages)
    assert last.tolist() == [2, 0, 3, 0] and np.diff(indptr).tolist() == [2, empty_pages, 1, empty_pages]
    assert R.seq_lens(indptr, last, P).tolist() == list(lens)
    rows = R.profile_rows("uniform", lens, 2, seed=0)
    data, param = R.rows_to_cache(pages, 2, P, (indptr, indices, last), lens, 1, *rows, True, F16)
    kr, kp = R.gather_rows(data, param, indptr, indices, last, 1, 1, 0, 0)
    assert kr.shape == (0, 64) and kp.shape == (0, 2)
    q = np.random.default_rng(0).standard_normal((4, 4, 128))
    out, (spa, qa) = R.paged_attention_f64(q, data, param, indptr, indices, last, 1)
    for b in (1, 3):
        assert not out[b].any() and not spa[b].any() and not qa[b].any()
    assert not R.decode_bound(out, spa, qa, 2.0 ** -11, n=40)[[1, 3]].any()
    assert out[0].any() and out[2].any()
    assert not R.paged_attention_f32(q, data, param, indptr, indices, last, 1)[[1, 3]].any()
    assert not R.valid_row_mask(data.shape, indptr, indices, last, 1)[indices[indptr[1]:indptr[2]]].any()


@pytest.mark.parametrize("block", [32, 16])
def test_wave_ranges_tile_the_sequence(block):
    for T in (0, 1, 2, 31, 32, 33, 600, 1000, 1100):
        for S in (1, 2, 7, 10):
            r = R.wave_ranges(T, S, block).reshape(-1, 2)
            busy = r[r[:, 0] < r[:, 1]]
            assert (busy[:, 0] % block == 0).all() and (r[:, 0] <= r[:, 1]).all()
            assert busy[:, 0].tolist() == ([0] + busy[:-1, 1].tolist() if len(busy) else []) and (busy[-1, 1] if len(busy) else 0) == T


def _nnz(spec):
    return len(R.case_tables(spec, 0)[2])


@pytest.mark.parametrize("case", list(R.CASES))
def test_cases_reach_the_paths_they_claim(case):
    """Pure arithmetic on the launcher's formulas: S at every group width, blocks per wave, idle slices, T = 1 | 2 under S > 1."""
    spec = R.CASES[case]
    P, lens, N, S = spec["P"], spec["lens"], spec["N"], spec["S"]
    for g in R.G_ALL:
        assert R.decode_splits(len(lens), g * N, N, _nnz(spec), P) == S, g
    assert R.blocks_per_wave(max(lens), S, 32) == spec["per"]
    busy = {T: (np.diff(R.wave_ranges(T, S, 32), axis=-1)[..., 0] > 0) for T in lens}
    if case in ("ragged", "ragged5", "empty", "empty1"):
        assert spec["per"] >= 4 and S > 1                                   # two full trips of the double-buffered loop
        assert all(not busy[T][1:].any() for T in lens if T <= 33)          # the short sequences leave slice 1 fully idle
    if case == "ragged":
        assert {1, 2} <= set(lens)
    if case == "odd":
        assert spec["per"] == 3                                             # the last block of a full wave sits in the reloaded buffer
    if case == "five":
        assert spec["per"] >= 5 and N > 1 and S > 1
    if case == "single":
        assert spec["per"] >= 5 and S == 1
    if case == "ragged5":
        assert P == 5                                                       # a 32-position block spans 6 - 7 pages
    if case == "padded":
        assert S == 10 and not busy[300][3:].any() and not busy[40][1:].any() and _nnz(spec) == 19 + 3 + 150
    if case.startswith("empty"):
        assert not busy[0].any()
    # the 16-bit kernel streams 16-position blocks: the deep cases are deeper still
    assert R.blocks_per_wave(max(lens), S, 16) >= spec["per"]


def test_a_step_case_puts_the_new_row_on_a_reloaded_buffer():
    """The wave that owns position T - 1 streams it in its third or later block: block index >= 2 is a buffer load_block filled twice."""
    deep = []
    for case, spec in R.CASES.items():
        T = max(spec["lens"])
        r = R.wave_ranges(T, spec["S"], 32).reshape(-1, 2)
        t0 = [a for a, b in r if a < b and b == T][0]
        if (T - 1 - t0) // 32 >= 2:
            deep.append(case)
    assert {"ragged", "five", "single"} <= set(deep), deep                  # (odd's owner holds the last 28 positions alone)


def _worst(got, c, u, n=0):
    err, bound = np.abs(got - c["ref"]), R.decode_bound(c["ref"], c["spa"], c["qa"], u, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


def _block_maxima(c, b, block):
    indptr, indices, last = c["tables"]
    kr, kp = R.gather_rows(c["data"], c["param"], indptr, indices, last, 1, b, 0, 0)
    K = R.dequantize_f32(kr, kp).astype(np.float64) if c["data"].dtype == np.uint8 else kr
    sc = (K @ c["q"][b].T) * R.SM_SCALE
    return np.stack([sc[t:t + block].max(0) for t in range(0, len(sc), block)])


@pytest.mark.parametrize("i4", [True, False], ids=["i4", "16bit"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_profiles_are_what_they_claim_and_fp32_meets_the_bound(i4, dtype):
    """uniform: every score 0.  ramps: the block maximum moves by several units per block, the same way throughout.  A plain fp32
    attention, rounded once to the output dtype, stays inside the bound for every profile on every case it runs on: the reference alone
    meets the condition the kernel is held to.  (n = T for this one: numpy's summation order is its own; no chain is longer than T.)"""
    block = 32 if i4 else 16
    for case in ("ragged", "odd", "single"):
        for profile in ("uniform", "ramp_up", "ramp_down"):
            c = R.profile_case(case, profile, i4, dtype, 2)
            T = max(c["lens"])
            if profile == "uniform":
                assert not c["q"].any() and not c["qa"].any()
            else:
                full = _block_maxima(c, 0, block)[:T // block]               # (a partial last block moves by less)
                step = np.diff(full, axis=0) * (1 if profile == "ramp_up" else -1)
                assert step.min() >= (4.0 if i4 else 2.0), step.min()
                assert np.abs(_block_maxima(c, 0, block)).max() > 150          # exp(-150) is below fp32: the far blocks underflow
            got = torch.from_numpy(R.paged_attention_f32(c["q"], c["data"], c["param"], *c["tables"], 1, i4)).to(dtype).double().numpy()
            n = np.array(c["lens"], dtype=np.float64).reshape(-1, 1, 1) if profile == "uniform" else 0
            worst = _worst(got, c, U[dtype], n)
            print(f"fp32 numpy, {case} {profile} {'i4' if i4 else '16bit'} {dtype}: max err/bound = {worst:.3f} "
                  f"(n = 0: {_worst(got, c, U[dtype]):.3f}, n of the kernel: {_worst(got, c, U[dtype], c['n']):.3f})")
            assert worst <= 1.0
    c = R.probe_case(i4, dtype)
    got = torch.from_numpy(R.paged_attention_f32(c["q"], c["data"], c["param"], *c["tables"], 1, i4)).to(dtype).double().numpy()
    print(f"fp32 numpy, probes {'i4' if i4 else '16bit'} {dtype}: max err/bound = {_worst(got, c, U[dtype]):.3f}")
    assert _worst(got, c, U[dtype]) <= 1.0


@pytest.mark.parametrize("i4", [True, False], ids=["i4", "16bit"])
def test_randn_cases_fp32_meets_the_bound(i4):
    """The ragged cases with the quantised randn rows the GPU test uses, g = 2, float16."""
    for case, spec in R.CASES.items():
        P, lens, N = spec["P"], spec["lens"], spec["N"]
        pages, indptr, indices, last = R.case_tables(spec, seed=3)
        gen = torch.Generator().manual_seed(P)
        k, v = ((torch.randn(sum(lens), N, 128, generator=gen) * 3).to(F16) for _ in range(2))
        q = torch.randn(len(lens), 2 * N, 128, generator=gen).to(F16).double().numpy()
        if i4:
            (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
            rows = (R.unpack_codes(kq.numpy()), kp.numpy(), R.unpack_codes(vq.numpy()), vp.numpy())
            data, param = R.rows_to_cache(pages, 2, P, (indptr, indices, last), lens, 1, *rows, True, F16)
        else:
            data, param = np.full((pages, 2, 2, N, P, 128), np.nan), np.ones((pages, 2, 2, N, P, 2), dtype=np.float16)
            ones, sl = np.ones((sum(lens), N, 2), dtype=np.float16), np.concatenate([[0], np.cumsum(lens)])
            R.write_rows(data, param, indptr, indices, last, k.double().numpy(), v.double().numpy(), ones, ones, sl, 1)
        ref, (spa, qa) = R.paged_attention_f64(q, data, param, indptr, indices, last, 1, i4=i4)
        got = torch.from_numpy(R.paged_attention_f32(q, data, param, indptr, indices, last, 1, i4)).to(F16).double().numpy()
        worst = _worst(got, dict(ref=ref, spa=spa, qa=qa), U[F16])
        print(f"fp32 numpy, {case} randn {'i4' if i4 else '16bit'}: max err/bound = {worst:.3f}")
        assert worst <= 1.0
        for b, T in enumerate(lens):
            assert T or not got[b].any()


def _mutate(c, b, drop=None, twice=None):
    """The fp64 reference of sequence b, head 0 of a case with N = 1 with one position removed or counted twice."""
    indptr, indices, last = c["tables"]
    i4 = c["data"].dtype == np.uint8
    kr, kp = R.gather_rows(c["data"], c["param"], indptr, indices, last, 1, b, 0, 0)
    vr, vp = R.gather_rows(c["data"], c["param"], indptr, indices, last, 1, b, 0, 1)
    K, V = (R.dequantize_f32(kr, kp).astype(np.float64), R.dequantize_f32(vr, vp).astype(np.float64)) if i4 else (kr, vr)
    idx = list(range(len(K)))
    if drop is not None:
        idx.remove(drop)
    if twice is not None:
        idx.append(twice)
    sc = (K[idx] @ c["q"][b, 0]) * R.SM_SCALE
    p = np.exp(sc - sc.max())
    return (p / p.sum()) @ V[idx]


@pytest.mark.parametrize("i4", [True, False], ids=["i4", "16bit"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_the_new_inputs_have_teeth(i4, dtype):
    """uniform at T = 1000: leaving out a position, or counting one twice, at the first and the last edge of a wave range breaks the bound
    (with the accumulation term in it) in at least one element -- the kind of error randn inputs hide under a 3.6 % bound.  spike:
    leaving out the target breaks it by orders of magnitude, and so does reading the neighbour's row in its place.  Counting a position
    twice cannot move a spike's result -- the target's weight is 1 either way -- so that mutation is uniform's to catch."""
    block = 32 if i4 else 16
    c = R.profile_case("ragged", "uniform", i4, dtype, 1)
    T = c["lens"][0]
    busy = [(a, b) for a, b in R.wave_ranges(T, c["S"], block).reshape(-1, 2) if a < b]
    edges = [busy[0][0], busy[0][1] - 1, busy[0][1], busy[-1][0], T - 1]
    ref, bound = c["ref"][0, 0], R.decode_bound(c["ref"], c["spa"], c["qa"], U[dtype], c["n"])[0, 0]
    assert np.allclose(_mutate(c, 0), ref, rtol=0, atol=1e-12)
    for t in edges:
        for kind in ("drop", "twice"):
            factor = float((np.abs(_mutate(c, 0, **{kind: t}) - ref) / bound).max())
            print(f"uniform {'i4' if i4 else '16bit'} {dtype}: {kind} position {t}: error / bound = {factor:.1f}")
            assert factor > 10, (kind, t, factor)
    c = R.probe_case(i4, dtype)
    gap = R.spike_gap(c)
    print(f"spike {'i4' if i4 else '16bit'}: the target's score leads by at least {gap:.1f}")
    assert gap >= 30.0
    assert np.abs(c["ref"] - c["want"]).max() < 1e-9                       # o = the target's V row
    pos = R.probe_positions(c["T"], block)
    edge_set = set(R.wave_ranges(c["T"], c["S"], block).reshape(-1).tolist()) - {c["T"]}
    assert edge_set <= set(pos) and {e - 1 for e in edge_set if e} <= set(pos) and len(set(c["targets"].reshape(-1).tolist())) == len(pos)
    bound = R.decode_bound(c["ref"], c["spa"], c["qa"], U[dtype])
    for h in (0, 1, c["targets"].shape[1] - 1):
        t = int(c["targets"][0, h])
        cc = dict(c, q=c["q"][:, h:h + 1])
        factor = float((np.abs(_mutate(cc, 0, drop=t) - c["ref"][0, h]) / bound[0, h]).max())
        nb = t + 1 if t + 1 < c["T"] else t - 1
        V_nb = _mutate(cc, 0, drop=t, twice=nb)                            # row t misaddressed: the neighbour's K and V in its place
        factor_nb = float((np.abs(V_nb - c["ref"][0, h]) / bound[0, h]).max())
        print(f"spike {'i4' if i4 else '16bit'} {dtype} at {t}: drop: error / bound = {factor:.0f}, neighbour's row: {factor_nb:.0f}")
        assert factor > 10 and factor_nb > 10

