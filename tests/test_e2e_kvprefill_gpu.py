"""The harness's opt-in prefill attention over the int4 pages (``DecoderModel(kv_cache="int4", kv_paged_prefill=True)``, ``-m gpu``): the toy
decoder of tests/test_e2e_kv_gpu.py (one layer, bs = 3) takes a 9-token prompt as 5 + 4 tokens, the second call at position 5.  The pages
must equal the reference quantisation (tests/kv_reference.py) of the k / v each call produced, written where the call's positions are;
each call's attention output must lie within the bound of tests/test_kvprefill_gpu.py of the fp64 causal attention over the model's own
pages; a decode step follows; without the flag a multi-token call beyond position 0 still raises.

Split against whole, byte for byte: layer 0's k / v of a token depend on that token alone, provided the projection computes a row the
same way whatever the call's row count is.  The MXFP4 model is the one that promises it here: its activation quantiser has no
per-tensor scale and every call of this test (15, 12 and 27 rows) takes the same GEMM kernel, whose rows do not see each other.  The
NVFP4 model switches kernels at 16 rows, so for it the pages are compared with the calls' own k / v only."""
import numpy as np
import pytest
import torch

from tests import kv_prefill_reference as PR
from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BSZ, FIRST, SECOND = 3, 5, 4
U_BF16 = 2.0 ** -8


def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toykv", num_layers=1, num_heads=16, hidden_size=2048, intermediate_size=4096, vocab_size=512,
                                attention_bias=True, mlp_bias=True)


def _np_tables(t):
    return t["kv_indptr"].cpu().numpy(), t["kv_indices"].cpu().numpy(), t["last_page_offset"].cpu().numpy()


def _rows(x):
    return x.detach().cpu().reshape(-1, x.shape[-2], 128)


def _check_call(m, tr, pos, n_new, data, param):
    """One traced multi-token call: its k / v quantised into (data, param) at positions pos .. pos + n_new - 1 must give the model's pages,
    and its attention output must be within the bound of the fp64 causal attention over them."""
    assert tr["layer"] == 0 and tr["pos"] == pos and tr["n_new"] == n_new
    (kq, kp), (vq, vp) = R.quantize_i4(_rows(tr["k"])), R.quantize_i4(_rows(tr["v"]))
    tabs = _np_tables(m.kvc.tables(pos + n_new))
    qo = np.arange(BSZ + 1) * n_new
    R.write_rows(data, param, *tabs, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), qo, 0)
    assert np.array_equal(m.kvc.pages.cpu().numpy(), data), f"pos {pos}: pages"
    assert np.array_equal(m.kvc.scales.cpu().numpy().view(np.uint16), param.view(np.uint16)), f"pos {pos}: parameters"
    ref, (spa, qa) = PR.paged_prefill_f64(tr["q"].double().cpu().numpy(), qo, data, param, *tabs, 0)
    err = np.abs(tr["out"].double().cpu().numpy() - ref)
    bound = PR.prefill_bound(ref, spa, qa, U_BF16, np.full((BSZ * n_new, 1, 1), float(pos + n_new)))
    print(f"pos {pos}, {n_new} tokens: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"pos {pos}: max err / bound = {(err / bound).max()}"


@pytest.mark.parametrize("quant_type", ["MXFP4", "NVFP4"])
def test_a_prompt_in_two_calls(quant_type):
    e2e, cfg = _toy()
    T = FIRST + SECOND
    gen = torch.Generator(device=DEV).manual_seed(5)
    tok = torch.randint(0, cfg.vocab_size, (BSZ, T), device=DEV, generator=gen)
    nxt = torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV, generator=gen)
    with torch.no_grad():
        split = e2e.DecoderModel(cfg, BSZ, T + 1, DEV, fused=True, attention="cache", quant_type=quant_type, kv_cache="int4", kv_paged_prefill=True)
        whole = e2e.DecoderModel(cfg, BSZ, T + 1, DEV, fused=True, attention="cache", quant_type=quant_type, kv_cache="int4", kv_paged_prefill=True)
        split.kv_trace, whole.kv_trace = [], []
        data = np.zeros(tuple(split.kvc.pages.shape), dtype=np.uint8)
        param = np.zeros(tuple(split.kvc.scales.shape), dtype=np.float16)
        l1 = split.forward(tok[:, :FIRST].contiguous(), 0)
        _check_call(split, split.kv_trace[-1], 0, FIRST, data, param)
        l2 = split.forward(tok[:, FIRST:].contiguous(), FIRST)                # pos != 0: no longer raises
        assert len(split.kv_trace) == 2
        _check_call(split, split.kv_trace[-1], FIRST, SECOND, data, param)
        assert torch.isfinite(l1.float()).all() and torch.isfinite(l2.float()).all()

        wdata, wparam = np.zeros_like(data), np.zeros_like(param)
        lw = whole.forward(tok, 0)
        _check_call(whole, whole.kv_trace[-1], 0, T, wdata, wparam)
        assert torch.isfinite(lw.float()).all()
        if quant_type == "MXFP4":       # the split prompt leaves the pages of the whole one, byte for byte
            assert torch.equal(split.kvc.pages, whole.kvc.pages)
            assert torch.equal(split.kvc.scales.view(torch.int16), whole.kvc.scales.view(torch.int16))

        # a decode step follows: append + batch_decode_i4 over the ten positions
        logits = split.forward(nxt, T)
        assert torch.isfinite(logits.float()).all() and len(split.kv_trace) == 3
        tr = split.kv_trace[-1]
        (kq, kp), (vq, vp) = R.quantize_i4(_rows(tr["k"])), R.quantize_i4(_rows(tr["v"]))
        tabs = _np_tables(split.kvc.tables(T + 1))
        R.write_rows(data, param, *tabs, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None, 0)
        assert np.array_equal(split.kvc.pages.cpu().numpy(), data)
        ref, (spa, qa) = R.paged_attention_f64(tr["q"].double().cpu().numpy(), data, param, *tabs, 0)
        assert (np.abs(tr["out"].double().cpu().numpy() - ref) <= R.decode_bound(ref, spa, qa, U_BF16)).all()


def test_without_the_flag_a_later_multi_token_call_still_raises():
    e2e, cfg = _toy()
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, FIRST + SECOND, DEV, fused=True, attention="cache", kv_cache="int4")
        assert m.kv_paged_prefill is False
        tok = torch.randint(0, cfg.vocab_size, (BSZ, FIRST + SECOND), device=DEV)
        m.forward(tok[:, :FIRST].contiguous(), 0)
        with pytest.raises(ValueError, match="position 0"):
            m.forward(tok[:, FIRST:].contiguous(), FIRST)
    with pytest.raises(ValueError, match="kv_paged_prefill"):
        e2e.DecoderModel(cfg, BSZ, 8, DEV, fused=True, attention="cache", kv_paged_prefill=True)
