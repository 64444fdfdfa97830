"""The harness's opt-in int4 KV cache (``DecoderModel(kv_cache="int4")``, ``-m gpu``): a toy decoder with one layer and bs = 3 writes its
prefill through init_kv_quantize_i4 and runs decode steps through append_kv_quantize_i4 + batch_decode_i4.  The pages must equal the
reference quantisation (tests/kv_reference.py) of the K / V the model produced, each step's attention output must lie within the fp32
bound of tests/test_kvcache_gpu.py of an fp64 attention over the model's own pages, and the default dense cache must be untouched.

The toy has 16 heads, not 4: the harness's linears need hidden_size >= 2048 (the RMSNorm quantiser's range) and the int4 cache needs a
head dimension of 128, so 2048 / 128 = 16 heads is the smallest model both accept."""
import numpy as np
import pytest
import torch

from tests import kv_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BSZ, PREFILL, STEPS = 3, 20, 3


def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toykv", num_layers=1, num_heads=16, hidden_size=2048, intermediate_size=4096, vocab_size=512,
                                attention_bias=True, mlp_bias=True)


def _np_tables(t):
    return t["kv_indptr"].cpu().numpy(), t["kv_indices"].cpu().numpy(), t["last_page_offset"].cpu().numpy()


def _rows(x):
    """bf16 device tensor [..., nh, 128] -> CPU tensor [tokens, nh, 128]."""
    return x.detach().cpu().reshape(-1, x.shape[-2], 128)


def test_int4_cache_model_against_the_reference_format():
    e2e, cfg = _toy()
    nh = cfg.num_heads
    gen = torch.Generator(device=DEV).manual_seed(3)
    tok = torch.randint(0, cfg.vocab_size, (BSZ, PREFILL), device=DEV, generator=gen)
    nxt = [torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV, generator=gen) for _ in range(STEPS)]
    with torch.no_grad():
        dense = e2e.DecoderModel(cfg, BSZ, PREFILL + STEPS, DEV, fused=True, attention="cache")
        named = e2e.DecoderModel(cfg, BSZ, PREFILL + STEPS, DEV, fused=True, attention="cache", kv_cache="bf16")
        i4 = e2e.DecoderModel(cfg, BSZ, PREFILL + STEPS, DEV, fused=True, attention="cache", kv_cache="int4")
        i4.kv_trace = []
        # the default is the dense cache, and naming it changes nothing
        lp = dense.forward(tok, 0)
        assert torch.equal(lp, named.forward(tok, 0))
        assert torch.equal(dense.forward(nxt[0], PREFILL), named.forward(nxt[0], PREFILL))
        assert i4.layers[0]["kv"].numel() == 0 and dense.kvc is None

        # prefill: the pages hold the reference quantisation of the K / V the dense-cache model holds at the same positions (exact:
        # layer 0's inputs are the same in both models)
        li = i4.forward(tok, 0)
        assert torch.isfinite(li.float()).all() and li.shape == lp.shape
        data = np.zeros(tuple(i4.kvc.pages.shape), dtype=np.uint8)
        param = np.zeros(tuple(i4.kvc.scales.shape), dtype=np.float16)
        kc, vc = dense.layers[0]["kc"][:, :, :PREFILL], dense.layers[0]["vc"][:, :, :PREFILL]              # [B, nh, T, 128]
        (kq, kp), (vq, vp) = R.quantize_i4(_rows(kc.transpose(1, 2))), R.quantize_i4(_rows(vc.transpose(1, 2)))
        tabs = _np_tables(i4.kvc.tables(PREFILL))
        R.write_rows(data, param, *tabs, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), np.arange(BSZ + 1) * PREFILL, 0)
        assert np.array_equal(i4.kvc.pages.cpu().numpy(), data)
        assert np.array_equal(i4.kvc.scales.cpu().numpy().view(np.uint16), param.view(np.uint16))

        # decode steps: pages against the model's own k / v, attention against fp64 over the model's own pages
        for step in range(STEPS):
            pos = PREFILL + step
            logits = i4.forward(nxt[step], pos)
            assert torch.isfinite(logits.float()).all()
            tr = i4.kv_trace[-1]
            assert tr["layer"] == 0 and tr["pos"] == pos and len(i4.kv_trace) == step + 1
            (kq, kp), (vq, vp) = R.quantize_i4(_rows(tr["k"])), R.quantize_i4(_rows(tr["v"]))
            tabs = _np_tables(i4.kvc.tables(pos + 1))
            R.write_rows(data, param, *tabs, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None, 0)
            assert np.array_equal(i4.kvc.pages.cpu().numpy(), data), f"step {step}: pages"
            assert np.array_equal(i4.kvc.scales.cpu().numpy().view(np.uint16), param.view(np.uint16)), f"step {step}: parameters"
            ref, (spa, qa) = R.paged_attention_f64(tr["q"].double().cpu().numpy(), data, param, *tabs, 0)
            err = np.abs(tr["out"].double().cpu().numpy() - ref)
            bound = R.decode_bound(ref, spa, qa, 2.0 ** -8)
            print(f"step {step}: max err / bound = {(err / bound).max():.3f}")
            assert (err <= bound).all(), f"step {step}: max err / bound = {(err / bound).max()}"


def test_int4_cache_decode_replays_from_a_graph():
    """The page tables of every length exist before the capture: a captured decode step replays to the eager logits."""
    e2e, cfg = _toy()
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, PREFILL + 2, DEV, fused=True, attention="cache", kv_cache="int4")
        tok = torch.randint(0, cfg.vocab_size, (BSZ, PREFILL), device=DEV)
        nxt = torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV)
        m.forward(tok, 0)
        want = m.forward(nxt, PREFILL).clone()
        torch.cuda.synchronize()
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            m.forward(nxt, PREFILL)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                out = m.forward(nxt, PREFILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.parametrize("fused,quant_type", [(False, "NVFP4"), (True, "MXFP4"), (False, "MXFP4")])
def test_int4_cache_in_the_other_call_structures(fused, quant_type):
    """The reference's call structure (separate q, k, v GEMMs) and the MXFP4 models reach the same cache code: a prefill and one decode
    step, pages equal to the reference quantisation of the step's own k / v, attention within the bound."""
    e2e, cfg = _toy()
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, PREFILL + 1, DEV, fused=fused, attention="cache", quant_type=quant_type, kv_cache="int4")
        m.kv_trace = []
        gen = torch.Generator(device=DEV).manual_seed(4)
        m.forward(torch.randint(0, cfg.vocab_size, (BSZ, PREFILL), device=DEV, generator=gen), 0)
        before = m.kvc.pages.cpu().numpy().copy(), m.kvc.scales.cpu().numpy().copy()
        logits = m.forward(torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV, generator=gen), PREFILL)
    assert torch.isfinite(logits.float()).all() and len(m.kv_trace) == 1
    tr, (data, param) = m.kv_trace[0], before
    (kq, kp), (vq, vp) = R.quantize_i4(_rows(tr["k"])), R.quantize_i4(_rows(tr["v"]))
    tabs = _np_tables(m.kvc.tables(PREFILL + 1))
    R.write_rows(data, param, *tabs, kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None, 0)
    assert np.array_equal(m.kvc.pages.cpu().numpy(), data) and np.array_equal(m.kvc.scales.cpu().numpy().view(np.uint16), param.view(np.uint16))
    ref, (spa, qa) = R.paged_attention_f64(tr["q"].double().cpu().numpy(), data, param, *tabs, 0)
    err = np.abs(tr["out"].double().cpu().numpy() - ref)
    assert (err <= R.decode_bound(ref, spa, qa, 2.0 ** -8)).all()


def test_int4_cache_arguments():
    e2e, cfg = _toy()
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 1, 8, DEV, fused=True, attention="current", kv_cache="int4")
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 1, 8, DEV, fused=True, attention="cache", kv_cache="fp8")
