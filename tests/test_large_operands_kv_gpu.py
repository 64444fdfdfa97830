"""The paged KV cache with page ids across the 2 GiB and 4 GiB byte marks (``-m gpu``; DESIGN.md 5.2: ``kv_row`` is 64-bit from
``(size_t)page`` on, and nothing but these runs holds it there).

A cache of L = 2 layers, N = 8 kv heads and P = 16 entries has 32 KiB of ``kv_data`` per page; 140 000 pages are 4.27 GiB (and 273 MiB
of ``kv_param``).  Every scenario runs twice: on a compact cache whose pages are 0 .. n - 1, and on the large one with the SAME
sequences mapped onto page ids that include 0, 1, 65535, 65536, 65537 (the 2 GiB mark), 131071, 131072, 131073 (the 4 GiB mark),
139999 and seeded others.  The existing tests tie the compact run to tests/kv_reference.py; here

  * attention outputs and the rotated ``q_out`` of the large run must be bit-equal to the compact run's,
  * every page of the large cache that the map names must equal the compact cache's page, ``kv_data`` and ``kv_param``,
  * every other byte of all 4.27 GiB (and of kv_param) must still be the 0xA5 it started as,
  * the decode step's arrival counters must come back zeroed.

A page id narrowed to 32 bits of BYTES (or a page * L * 2 * N * P * 64 product formed in ``int``) writes page 131072 + k over page k
or reads it from there: the id map's targets then differ from the compact pages, or a byte outside them is no longer 0xA5.

The scenario, per 16-bit type, on ragged sequences (1 .. 1100 positions, so that the decode kernels slice the long ones): layer 0
arcq_kv_init_quantize, arcq_kv_batch_prefill, arcq_kv_batch_decode, arcq_kv_append_quantize, arcq_kv_decode_step,
arcq_kv_rope_append_quantize; layer 1 arcq_kv_init, arcq_kv_append, arcq_kv_rope_init_quantize, arcq_kv_batch_decode."""
import numpy as np
import pytest
import torch

from tests import bigmem as BM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L_, N_, P_, NQ = 2, 8, 16, 32
PAGES = 140_000
PAGE_BYTES = L_ * 2 * N_ * P_ * 64
MARKS = [0, 1, 65535, 65536, 65537, 131071, 131072, 131073, PAGES - 1]
LENS = (1, 15, 16, 17, 700, 1100)          # before the scenario's three further positions
B_ = len(LENS)
FILL = 0xA5


def _tables(extra, pages_of):
    """Tables of sequences of LENS[b] + extra positions over the page lists ``pages_of[b]`` (a prefix of each)."""
    indptr, indices, last = [0], [], []
    for b, n in enumerate(LENS):
        T = n + extra
        cnt = (T + P_ - 1) // P_
        indices += pages_of[b][:cnt]
        indptr.append(len(indices))
        last.append(T - (cnt - 1) * P_)
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    return dict(kv_indptr=dev(indptr), kv_indices=dev(indices), last_page_offset=dev(last))


def _scenario(dtype, data, param, pages_of):
    """Runs every entry point once; returns the attention outputs / q_out (in call order) and the decode step's counters."""
    from arcquant_amd import kvcache as kv, kvprefill, kvrope, kvstep
    g = torch.Generator().manual_seed(77)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 3).to(dtype).to(DEV)
    outs = []

    def out_of(fn, like, *args, **kw):          # the call's first argument is its output
        o = torch.full_like(like, float("nan"))
        fn(o, *args, **kw)
        outs.append(o)

    t0, t1, t2, t3 = (_tables(e, pages_of) for e in range(4))
    sl = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int32, device=DEV)
    ntok = int(sl[-1])
    # ---- layer 0: the quantising path
    kv.init_kv_quantize_i4(data, param, **t0, k=rnd(ntok, N_, 128), v=rnd(ntok, N_, 128), seqlen_indptr=sl, layer_idx=0)
    q = rnd(ntok, NQ, 128)
    out_of(kvprefill.batch_prefill_i4, q, q, sl, data, param, **t0, layer_idx=0)
    q = rnd(B_, NQ, 128)
    out_of(kv.batch_decode_i4, q, q, data, param, **t0, layer_idx=0)
    kv.append_kv_quantize_i4(data, param, **t1, k=rnd(B_, N_, 128), v=rnd(B_, N_, 128), layer_idx=0)
    state = kvstep.DecodeStepState(B_, NQ, N_, DEV)
    q = rnd(B_, NQ, 128)
    out_of(kvstep.decode_step_i4, q, q, rnd(B_, N_, 128), rnd(B_, N_, 128), data, param, **t2, layer_idx=0, state=state)
    cos, sin = kvrope.rope_tables(2048, dtype=dtype, device=DEV)
    q = rnd(B_, NQ, 128)
    out_of(kvrope.rope_append_kv_quantize_i4, q, q, rnd(B_, N_, 128), rnd(B_, N_, 128), cos, sin, data, param, **t3, layer_idx=0)
    out_of(kv.batch_decode_i4, q, q, data, param, **t3, layer_idx=0)
    # ---- layer 1: the copying writers, then RoPE + quantise over the last two positions of every sequence
    gi = torch.Generator().manual_seed(78)
    codes = lambda n: torch.randint(0, 256, (n, N_, 64), generator=gi, dtype=torch.uint8).to(DEV)
    # (scale, zero) pairs that are finite fp16: scale in [0.05, 0.45], zero in [0, 8]
    params = lambda n: torch.stack([torch.rand(n, N_, generator=gi) * 0.4 + 0.05, torch.rand(n, N_, generator=gi) * 8], dim=-1).to(torch.float16).to(DEV)
    kv.init_kv_i4(data, param, **t0, k=codes(ntok), v=codes(ntok), k_param=params(ntok), v_param=params(ntok), seqlen_indptr=sl, layer_idx=1)
    kv.append_kv_i4(data, param, **t1, k=codes(B_), v=codes(B_), k_param=params(B_), v_param=params(B_), layer_idx=1)
    sl2 = torch.arange(0, 2 * B_ + 1, 2, dtype=torch.int32, device=DEV)
    q = rnd(2 * B_, NQ, 128)
    out_of(kvrope.rope_init_kv_quantize_i4, q, q, rnd(2 * B_, N_, 128), rnd(2 * B_, N_, 128), cos, sin, data, param, **t3, seqlen_indptr=sl2, layer_idx=1)
    q = rnd(B_, NQ, 128)
    out_of(kv.batch_decode_i4, q, q, data, param, **t3, layer_idx=1)
    torch.cuda.synchronize()
    return outs, state.counters


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pages_across_the_2gib_and_4gib_marks(dtype):
    from arcquant_amd import _lib
    BM.need(PAGES * PAGE_BYTES + PAGES * PAGE_BYTES // 16 + (1 << 30))
    # ---- the sequences' pages: compact ids 0 .. n - 1 in a seeded order, and the map onto the large cache
    rng = np.random.default_rng(5)
    counts = [(n + 3 + P_ - 1) // P_ for n in LENS]
    n = sum(counts)
    order = rng.permutation(n).tolist()
    compact_of, at = [], 0
    for c in counts:
        compact_of.append(order[at:at + c])
        at += c
    others = rng.choice(np.setdiff1d(np.arange(PAGES), MARKS), n - len(MARKS), replace=False)
    large_ids = rng.permutation(np.concatenate([MARKS, others])).tolist()          # compact page i -> large page large_ids[i]
    large_of = [[large_ids[i] for i in seq] for seq in compact_of]
    assert len(set(large_ids)) == n and set(MARKS) <= set(large_ids)
    # vacuity, on the CPU: the cache and the mapped ids cross the marks they name
    assert PAGES * PAGE_BYTES > 1 << 32 and PAGE_BYTES == 32768
    assert 65536 * PAGE_BYTES == 1 << 31 and 131072 * PAGE_BYTES == 1 << 32 and (PAGES - 1) * PAGE_BYTES > 1 << 32
    assert sum(i * PAGE_BYTES >= 1 << 32 for i in large_ids) >= 3 and sum(1 << 31 <= i * PAGE_BYTES < 1 << 32 for i in large_ids) >= 3
    # the long sequences are sliced (S > 1): the decode step uses its counters
    nnz = sum((x + 2 + P_ - 1) // P_ for x in LENS)
    assert _lib.lib().arcq_kv_decode_workspace_bytes(B_, NQ, N_, nnz, P_) > 0

    def cache(pages):
        return (torch.full((pages, L_, 2, N_, P_, 64), FILL, dtype=torch.uint8, device=DEV),
                torch.full((pages, L_, 2, N_, P_, 4), FILL, dtype=torch.uint8, device=DEV).view(torch.float16))

    cd, cp = cache(n)
    want, cnt_c = _scenario(dtype, cd, cp, compact_of)
    ld, lp = cache(PAGES)
    assert ld.numel() == PAGES * PAGE_BYTES
    got, cnt_l = _scenario(dtype, ld, lp, large_of)

    assert not bool(cnt_c.any()) and not bool(cnt_l.any()), "the decode step left arrival counters set"
    assert len(got) == len(want) == 7
    for i, (a, b) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(b.float()).any()), f"output {i} of the compact run holds NaN"
        assert len(torch.unique(b.view(torch.int16))) > 1000, f"output {i} of the compact run is degenerate"
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"output {i} differs between the compact and the large cache"
    # every compact page was written on both layers (so every mapped page of the large cache owes bytes)
    cdb, cpb = cd.view(n, -1), cp.view(torch.uint8).view(n, -1)
    assert bool((cdb != FILL).any(dim=1).all()) and bool((cpb != FILL).any(dim=1).all())
    ids = torch.tensor(large_ids, device=DEV)
    ldb, lpb = ld.view(PAGES, -1), lp.view(torch.uint8).view(PAGES, -1)
    for name, big, small in (("kv_data", ldb, cdb), ("kv_param", lpb, cpb)):
        diff = (big[ids] != small).any(dim=1)
        if bool(diff.any()):
            i = int(diff.nonzero()[0])
            off = int((big[large_ids[i]] != small[i]).nonzero()[0])
            raise AssertionError(f"{name}: page {large_ids[i]} of the large cache differs from page {i} of the compact one first at byte {off} of the "
                                 f"page, byte offset {large_ids[i] * big.shape[1] + off} of {big.numel()}")
        # ... and every OTHER byte is still 0xA5: blank the mapped pages, then the whole buffer must be the fill
        big[ids] = FILL
        flat = big.view(-1)
        for o in range(0, flat.numel(), 1 << 28):
            bad = flat[o:o + (1 << 28)] != FILL
            if bool(bad.any()):
                at_ = o + int(bad.nonzero()[0])
                raise AssertionError(f"{name}: byte offset {at_} (page {at_ // big.shape[1]}, which no sequence owns) was written")
    del ld, lp
    BM.release()
