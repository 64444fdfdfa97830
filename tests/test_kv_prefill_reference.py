"""CPU tests of tests/kv_prefill_reference.py: the fp64 causal prefill attention over the pages against the decode reference (one query
token per sequence), against a dense causal softmax (from an empty cache), its handling of sequences without query tokens or without
positions, and the claims of the shared GPU cases (what they straddle, which tile geometries the wide groups reach, how far a spike's
target leads).  The teeth: a numpy fp32 restatement of the algorithm meets every bound the GPU tests apply on every new case, and the
same restatement with one mistake (a position dropped or doubled, the mask one position off, V codes in the unswapped order, a
neighbour's row, a head stored one off) overshoots the bound by a factor of 10 or more under the profile that claims to catch it."""
import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R

F16, BF16 = torch.float16, torch.bfloat16
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}


def _pages(lens, P, N, seed, empty_pages=0):
    pages, indptr, indices, last = R.make_tables(lens, P, seed, empty_pages=empty_pages)
    gen = torch.Generator().manual_seed(seed)
    ntok = sum(lens)
    sl = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    k, v = (torch.randn(ntok, N, 128, generator=gen) * 3).to(torch.float16), (torch.randn(ntok, N, 128, generator=gen) * 3).to(torch.float16)
    (kq, kp), (vq, vp) = R.quantize_i4(k), R.quantize_i4(v)
    data = np.full((pages, 2, 2, N, P, 64), 0xA5, dtype=np.uint8)
    param = np.zeros((pages, 2, 2, N, P, 2), dtype=np.float16)
    param.view(np.uint8)[...] = 0xA5
    R.write_rows(data, param, indptr, indices, last, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), sl, 1)
    return data, param, (indptr, indices, last), gen


def test_one_query_token_per_sequence_is_the_decode_reference():
    lens, P, N, g = (37, 1, 16, 5), 5, 2, 3
    data, param, tables, gen = _pages(lens, P, N, 3)
    q = torch.randn(len(lens), g * N, 128, generator=gen).double().numpy()
    want, (wspa, wqa) = R.paged_attention_f64(q, data, param, *tables, 1)
    got, (spa, qa) = PR.paged_prefill_f64(q, np.arange(len(lens) + 1), data, param, *tables, 1)
    assert np.array_equal(got, want) and np.array_equal(spa, wspa) and np.array_equal(qa, wqa)


def test_from_an_empty_cache_it_is_a_dense_causal_softmax():
    lens, P, N, g = (19, 7), 4, 2, 2
    data, param, tables, gen = _pages(lens, P, N, 5)
    qo = np.concatenate([[0], np.cumsum(lens)])
    q = torch.randn(sum(lens), g * N, 128, generator=gen).double().numpy()
    got, _ = PR.paged_prefill_f64(q, qo, data, param, *tables, 1)
    for b, T in enumerate(lens):
        for n in range(N):
            kr, kp = R.gather_rows(data, param, *tables, 1, b, n, 0)
            vr, vp = R.gather_rows(data, param, *tables, 1, b, n, 1)
            K, V = R.dequantize_f32(kr, kp).astype(np.float64), R.dequantize_f32(vr, vp).astype(np.float64)
            for h in range(n * g, (n + 1) * g):
                s = (q[qo[b]:qo[b + 1], h] @ K.T) * R.SM_SCALE                 # [T, T]
                s = np.where(np.tril(np.ones((T, T), dtype=bool)), s, -np.inf)
                p = np.exp(s - s.max(-1, keepdims=True))
                want = (p / p.sum(-1, keepdims=True)) @ V
                assert np.abs(got[qo[b]:qo[b + 1], h] - want).max() < 1e-12


def test_a_chunk_attends_over_the_positions_before_it():
    """The last 6 of 21 positions: query i sees 16 + i positions, so it equals the decode reference over a sequence cut there."""
    T, n, P = 21, 6, 4
    data, param, tables, gen = _pages((T,), P, 1, 9)
    q = torch.randn(n, 2, 128, generator=gen).double().numpy()
    got, (spa, qa) = PR.paged_prefill_f64(q, np.array([0, n]), data, param, *tables, 1)
    indptr, indices, last = tables
    for i in range(n):
        end = T - n + i + 1
        cnt = (end + P - 1) // P
        cut = (np.array([0, cnt], dtype=np.int32), indices[:cnt], np.array([end - (cnt - 1) * P], dtype=np.int32))
        want, (wspa, wqa) = R.paged_attention_f64(q[i:i + 1], data, param, *cut, 1)
        assert np.array_equal(got[i], want[0]) and np.array_equal(spa[i], wspa[0]) and np.array_equal(qa[i], wqa[0])


def test_sequences_without_query_tokens_or_positions_give_no_rows():
    for empty_pages in (0, 1):
        lens = (12, 9, 0)
        data, param, tables, gen = _pages(lens, 4, 1, 11, empty_pages=empty_pages)
        qo = np.array([0, 3, 3, 3])                                         # n = 3, 0, 0; two rows beyond qo[B]
        q = torch.randn(5, 2, 128, generator=gen).double().numpy()
        got, (spa, qa) = PR.paged_prefill_f64(q, qo, data, param, *tables, 1)
        assert np.abs(got[:3]).min() > 0 and not got[3:].any() and not spa[3:].any() and not qa[3:].any()
        bound = PR.prefill_bound(got, spa, qa, 2.0 ** -11, np.zeros((5, 1, 1)))
        assert not bound[3:].any()


def test_the_shared_cases_straddle_the_tile_sizes():
    """Whatever the kernel's tile sizes are among 16 / 32 / 64 / 128: of the chunk lengths n and the chunk starts T - n, some value lies
    on a multiple or just beyond one (a tile that is full, or has one or two rows), and some value lies well inside a tile."""
    ns = [n for c in PR.PREFILL_CASES.values() for _, n in c["seqs"]]
    starts = [T - n for c in PR.PREFILL_CASES.values() for T, n in c["seqs"] if n]
    for m in (16, 32, 64, 128):
        r = {v % m for v in ns + starts if v >= m}
        assert r & {0, 1, 2} and any(2 < x < m - 1 for x in r), (m, sorted(r))
    # (40, 0) and (0, 0): sequences without query tokens, the second without positions, under both spellings
    assert PR.PREFILL_CASES["chunk"]["seqs"][3:] == ((40, 0), (0, 0)) and PR.PREFILL_CASES["chunk1"]["empty_pages"] == 1
    for case in PR.PREFILL_CASES:
        _, lens, new, qo, pages, tables = PR.case_geometry(case)
        assert list(R.seq_lens(tables[0], tables[2], PR.PREFILL_CASES[case]["P"])) == lens and all(n <= T for T, n in zip(lens, new))
        assert max(lens) <= 1000 and max(new) <= 130
    # "group" under the wide groups (PR.tile_geometry / PR.wave_lasts restate the launcher, for these assertions only)
    seqs = PR.PREFILL_CASES["group"]["seqs"]
    assert [PR.tile_geometry(g)[1] for g in PR.WIDE_GS] == [16, 8, 4, 2, 1, 1]
    assert any(n == T and n > 32 for T, n in seqs) and (1, 1) in seqs                 # n_b = T_b: from an empty cache, long and shortest
    for g in PR.WIDE_GS:
        hc, tpt, chunks = PR.tile_geometry(g)
        if tpt > 1:        # a partial last tile behind a full one
            assert chunks == 1 and any(n > tpt and n % tpt for _, n in seqs), g
        elif g == 128:     # one token per tile, every slot live
            assert (hc, chunks) == (128, 1)
        else:              # two chunks, the second partial in its HEADS: 2 of 128 slots live
            assert (hc, chunks) == (128, 2) and g - hc == 2
        lasts = [row for T, n in seqs for row in PR.wave_lasts(T, n, g)]
        live = [sorted({w for w in row if w >= 0}) for row in lasts]
        if g <= 64:        # a tile whose waves have different wave_last (g = 32: a wave is one token; g = 64: a token is two waves)
            assert any(len(s) > 1 for s in live), g
            assert any(-1 in row and max(row) >= 32 for row in lasts), g             # and one with idle waves beside a wave that loops
        else:              # one token per tile: the four waves agree
            assert all(len(s) == 1 and -1 not in row for s, row in zip(live, lasts)), g
        if g == 32:
            assert all(len(set(row) - {-1}) == sum(w >= 0 for w in row) for row in lasts)      # wtl0 == wtl1: no two waves share a token
        if g == 64:
            assert all(row[0] == row[1] and row[2] == row[3] for row in lasts)
        # a kv block that one LIVE wave of a tile skips while another visits it (tb <= wave_last): reached at g = 16 and 32 here, and by
        # "tiles" at g = 7, where the interior probes run too; at g = 8 and 64 the tiles of this case do not cross a block edge mid-tile
        crossing = any(s[0] // 32 < s[-1] // 32 for s in live)
        assert crossing == (g in (16, 32)), g
    assert any(s[0] // 32 < s[-1] // 32 for T, n in PR.PREFILL_CASES["tiles"]["seqs"]
               for s in [sorted({w for w in row if w >= 0}) for row in PR.wave_lasts(T, n, 7)])


def test_wave_lasts_restate_the_slots():
    """PR.wave_lasts against a slot-by-slot count: wave w of a tile holds slots 32 w .. 32 w + 31, slot r is token r / hc."""
    for g in (1, 7, 8, 32, 64, 128, 130):
        hc, tpt, _ = PR.tile_geometry(g)
        for T, n in ((70, 40), (33, 33), (1, 1), (300, 130)):
            rows = PR.wave_lasts(T, n, g)
            assert len(rows) == (n + tpt - 1) // tpt
            for x, row in enumerate(rows):
                for w in range(4):
                    toks = [x * tpt + r // hc for r in range(32 * w, 32 * w + 32) if r // hc < tpt and x * tpt + r // hc < n]
                    assert row[w] == (T - n + max(toks) if toks else -1), (g, T, n, x, w)


def _emulate(c, dtype, mutate=None):
    return PR.prefill_f32_emulated(c["q"].double().numpy(), c["qo"], c["data"], c["param"], *c["tables"], PR.LAYER, dtype, mutate)


def _ratio(got, c, bound):
    n_rows = int(c["qo"][-1])
    return float((np.abs(got - c["ref"])[:n_rows] / bound[:n_rows]).max())


def _profile_bound(c, profile, dtype):
    if profile == "uniform":
        return PR.uniform_bound(c["ref"], U[dtype])
    return PR.prefill_bound(c["ref"], c["spa"], c["qa"], U[dtype], c["T_rows"])


@pytest.mark.parametrize("kind", ["uniform", "ramps", "probes", "randn"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_the_emulation_meets_every_bound_of_the_new_cases(kind, dtype):
    """The condition that the inputs leave an honest implementation inside the bounds the GPU tests apply: the unmutated fp32 emulation
    on every profile run, every probe run and the wide-group randn runs.  Measured here (max error / bound): uniform 0.977 - 0.996 (the
    rounding of the result alone: half an ulp is u |ref| just above a power of two), ramp_up 0.02 - 0.18, ramp_down 0.01 - 0.15, probes 0
    (every row IS its target's V row), randn "group" 0.11 - 0.14 in fp16 and 0.23 - 0.27 in bf16."""
    if kind == "uniform":
        for case, g in PR.UNIFORM_RUNS:
            c = PR.profile_case(case, "uniform", dtype, g)
            PR.uniform_premises(c)
            r = _ratio(_emulate(c, dtype), c, _profile_bound(c, "uniform", dtype))
            print(f"uniform {case} g={g} {dtype}: {r:.3f}")
            assert r <= 1.0, (case, g, r)
    elif kind == "ramps":
        for case, profile, g in PR.RAMP_RUNS:
            c = PR.profile_case(case, profile, dtype, g)
            r = _ratio(_emulate(c, dtype), c, _profile_bound(c, profile, dtype))
            print(f"{profile} {case} g={g} {dtype}: {r:.3f}")
            assert r <= 1.0, (case, profile, g, r)
    elif kind == "probes":
        for case, g in PR.PROBE_RUNS:
            c = PR.probe_case(case, dtype, g)
            got = _emulate(c, dtype)
            r = _ratio(got, c, PR.prefill_bound(c["ref"], c["spa"], c["qa"], U[dtype], c["T_rows"]))
            print(f"probes {case} g={g} {dtype}: {r:.3f}")
            assert r <= 1.0 and PR.probe_rows_ok(got, c, dtype, U[dtype]).all(), (case, g, r)
    else:
        for g in PR.WIDE_GS:
            c = PR.case_inputs("group", dtype, g)
            r = _ratio(_emulate(c, dtype), c, PR.prefill_bound(c["ref"], c["spa"], c["qa"], U[dtype], c["T_rows"]))
            print(f"randn group g={g} {dtype}: {r:.3f}")
            assert r <= 1.0, (g, r)


def test_the_ramps_do_what_they_claim():
    """ramp_up: the running maximum of a query rises in every block up to its own.  ramp_down: it settles in block 0, and in fp16 the
    rounded weights p s pass through the subnormal range (below 2^-14) before they vanish."""
    for case in ("tiles", "deep"):
        for profile in ("ramp_up", "ramp_down"):
            c = PR.profile_case(case, profile, F16, 2)
            T, n = c["lens"][0], c["new"][0]
            kr, kp = R.gather_rows(c["data"], c["param"], *c["tables"], PR.LAYER, 0, 0, 0)
            K = R.dequantize_f32(kr, kp).astype(np.float64)
            for h in (0, 1):
                sc = (K @ c["q"][0, h].double().numpy()) * R.SM_SCALE * np.log2(np.e)          # base 2, all T positions
                block_max = np.array([sc[t:t + 32].max() for t in range(0, T, 32)])
                if profile == "ramp_up":
                    assert (np.diff(block_max) > 0).all() and (np.diff(block_max)[:-1] > 8.0).all(), (case, h)      # (the last block is partial)
                else:
                    assert (np.diff(block_max) < -8.0).all() and block_max[0] == sc[0], (case, h)
                    p = np.exp2(sc - sc[0])
                    assert ((p * 0.5 < 2.0 ** -14) & (p * 0.125 > 2.0 ** -24)).sum() >= 8, (case, h)


TEETH = {       # profile -> the mutations it claims; the position of drop / double: a block's last (31) and a block's first (160)
    "uniform": [(m, t) for m in ("drop", "double") for t in (31, 160)] + [("mask_late", None), ("mask_early", None), ("unswapped", None)],
    "ramp_up": [("drop", 31), ("double", 31), ("mask_late", None), ("mask_early", None), ("unswapped", None)],
    "ramp_down": [("mask_late", None), ("mask_early", None), ("unswapped", None)],
}


@pytest.mark.parametrize("profile", list(TEETH))
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_the_profiles_have_teeth(profile, dtype):
    """Each mutation of the emulation overshoots the profile's bound by a factor >= 10 at one element or more, on "tiles" (T = 300,
    n = 130; 129 from empty; one query over 257) at g = 2 (both betas).  Measured: uniform 5.4e5 - 4.2e7 for all seven; ramp_up drop at 31
    28 (bf16) / 104 (fp16), double at 31 16 / 64, the masks 83 - 964, the position order 71 / 299; ramp_down the masks 64 - 277, the
    position order 21 / 70.  NOT caught, and not claimed: a position dropped or doubled well below the diagonal under a ramp (ramp_up at 160:
    2 - 7; ramp_down anywhere: the clean 0.07 - 0.15) -- its weight is e^-(tens) there; that mistake is uniform's to catch."""
    c = PR.profile_case("tiles", profile, dtype, 2)
    bound = _profile_bound(c, profile, dtype)
    assert _ratio(_emulate(c, dtype), c, bound) <= 1.0
    for mutate in TEETH[profile]:
        r = _ratio(_emulate(c, dtype, mutate), c, bound)
        print(f"{profile} {dtype} {mutate}: error / bound = {r:.3g}")
        assert r >= 10.0, (profile, mutate, r)


@pytest.mark.parametrize("case,g", [("tiles", 7), ("group", 16), ("group", 130)])
def test_the_probes_have_teeth(case, g):
    """Reading the neighbouring V row in a target's place, or storing head h's result to head h ^ 1, fails the V-row assertion (on nearly
    every row, not on one), and so does each mistake the profiles catch when it touches a target."""
    c = PR.probe_case(case, F16, g)
    ok = PR.probe_rows_ok(_emulate(c, F16), c, F16, U[F16])
    assert ok.all()
    for mutate in (("neighbour", None), ("head_xor_1", None), ("unswapped", None), ("mask_early", None), ("drop", 31), ("drop", 32)):
        bad = ~PR.probe_rows_ok(_emulate(c, F16, mutate), c, F16, U[F16])
        print(f"probes {case} g={g} {mutate}: {int(bad.sum())} of {bad.size} rows fail")
        assert bad.any(), mutate
        if mutate[0] in ("neighbour", "head_xor_1"):
            assert bad.mean() > 0.8, mutate


def test_probe_targets_lead_by_more_than_sixty():
    for case, g in PR.PROBE_RUNS:
        c = PR.probe_case(case, F16, g)
        assert c["gap"] > 60.0, (case, g, c["gap"])
        qd = c["q"].double()
        assert torch.equal(qd, qd.round()) and float(qd.abs().max()) == 15.0 and not qd[c["own"] < 0].any()      # exact in fp16 and bf16
        assert torch.equal(PR.probe_case(case, BF16, g)["q"].double(), qd)
        n_rows = int(c["qo"][-1])
        assert np.abs(c["ref"][:n_rows] - c["want"][:n_rows]).max() < 1e-9              # the output is the target's V row
        tg, own = c["targets"][:n_rows], c["own"][:n_rows]
        assert (tg >= 0).all() and (tg <= own[:, None]).all()
        # every block edge below the diagonal is some head's target: each multiple of 32 and the position before it, up to the longest own
        hit = set(tg.ravel().tolist())
        top = int(own.max())
        assert {t for t in range(32, top + 1, 32)} | {t - 1 for t in range(32, top + 1, 32)} | {0} <= hit, (case, g)
        # neighbouring heads and neighbouring tokens point at different rows (where the query has more than one position to point at)
        many = own >= 1
        assert (tg[many, :-1] != tg[many, 1:]).all()
        same_seq = np.diff(np.searchsorted(c["qo"], np.arange(n_rows), side="right")) == 0
        # of two neighbouring tokens the heads that point at own - 1 or own always differ; the others do unless gN is a multiple of the
        # length of pos (g = 130: 260 heads over 4 or 5 positions): most (row, head) pairs differ from the next token's, not all
        pair = same_seq & many[:-1]
        assert (tg[:-1][pair] != tg[1:][pair]).mean() > 0.5, (case, g)


def test_spike_targets_lead_by_more_than_sixty():
    for case in ("chunk", "tiles"):
        for mode in ("diagonal", "masked"):
            c = PR.spike_case(case, torch.float16, 1, mode)
            assert c["gap"] > 60.0, (case, mode, c["gap"])
            qd = c["q"].double()
            assert torch.equal(qd, qd.round()) and float(qd.abs().max()) == 15.0 and not qd[c["own"] < 0].any()      # exact in fp16 and bf16
            # the queries cover own positions at a multiple of 16, 32, 64 and 128 and one below, where the sequences reach them
            own = set(c["own"][c["own"] >= 0].tolist())
            for m in (16, 32, 64, 128):
                if max(c["lens"]) > m:
                    assert any(t % m == 0 for t in own if t) and any(t % m == m - 1 for t in own), (case, m)
            rows = np.flatnonzero(c["own"] >= 0)
            if mode == "diagonal":      # the output is the target's V row
                for r in rows:
                    b = int(np.searchsorted(c["qo"], r, side="right") - 1)
                    assert np.abs(c["ref"][r, 0] - c["V"][c["start"][b] + c["targets"][r], 0]).max() < 1e-9
            else:                        # the masked target's V row is far from the reference: a leak is an O(1) error
                far = 0
                for r in rows:
                    b = int(np.searchsorted(c["qo"], r, side="right") - 1)
                    if c["targets"][r] != c["own"][r]:
                        far += np.abs(c["ref"][r, 0] - c["V"][c["start"][b] + c["targets"][r], 0]).max() > 0.5
                assert far >= 0.9 * (len(rows) - sum(1 for n in c["new"] if n))
