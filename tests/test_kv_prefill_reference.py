"""CPU tests of tests/kv_prefill_reference.py: the fp64 causal prefill attention over the pages against the decode reference (one query
token per sequence), against a dense causal softmax (from an empty cache), its handling of sequences without query tokens or without
positions, and the claims of the shared GPU cases (what they straddle, how far a spike's target leads)."""
import numpy as np
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R


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
