"""The harness's opt-in one-launch decode step (``DecoderModel(kv_cache="int4", kv_fused_step=True)``, ``-m gpu``) on the toy decoder of
tests/test_e2e_kv_gpu.py: against the same model with the three-launch chain, the logits, the pages and the parameters are equal bit for
bit at every step, in the fused call structure (views of q|k|v) and in the reference's (separate q, k, v); a captured step replays three
times to the eager logits -- an arrival counter that is not handed back zeroed shows in the second replay."""
import pytest
import torch

from tests.test_e2e_kv_gpu import BSZ, DEV, PREFILL, _toy

pytestmark = pytest.mark.gpu

STEPS = 3


@pytest.mark.parametrize("fused,quant_type", [(True, "NVFP4"), (False, "NVFP4")])
def test_fused_step_model_equals_the_chain_model(fused, quant_type):
    e2e, cfg = _toy()
    gen = torch.Generator(device=DEV).manual_seed(7)
    tok = torch.randint(0, cfg.vocab_size, (BSZ, PREFILL), device=DEV, generator=gen)
    nxt = [torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV, generator=gen) for _ in range(STEPS)]
    with torch.no_grad():
        models = []
        for step in (False, True):
            models.append(e2e.DecoderModel(cfg, BSZ, PREFILL + STEPS, DEV, fused=fused, attention="cache", quant_type=quant_type, kv_cache="int4",
                                           kv_fused_step=step))
        chain, one = models
        assert one.kv_step_state is not None and chain.kv_step_state is None
        one.kv_trace = []
        assert torch.equal(chain.forward(tok, 0), one.forward(tok, 0))
        for s in range(STEPS):
            a, b = chain.forward(nxt[s], PREFILL + s), one.forward(nxt[s], PREFILL + s)
            assert torch.isfinite(b.float()).all()
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"step {s}: logits"
            assert torch.equal(chain.kvc.pages, one.kvc.pages), f"step {s}: pages"
            assert torch.equal(chain.kvc.scales.view(torch.int16), one.kvc.scales.view(torch.int16)), f"step {s}: parameters"
            assert not one.kv_step_state.counters.any()
            assert len(one.kv_trace) == s + 1 and one.kv_trace[-1]["pos"] == PREFILL + s and one.kv_trace[-1]["out"].shape == (BSZ, cfg.num_heads, 128)


def test_fused_step_replays_from_a_graph_three_times():
    e2e, cfg = _toy()
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, PREFILL + 2, DEV, fused=True, attention="cache", kv_cache="int4", kv_fused_step=True)
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
        for replay in range(3):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want), f"replay {replay}"
            assert not m.kv_step_state.counters.any()


def test_fused_step_arguments():
    e2e, cfg = _toy()
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 1, 8, DEV, fused=True, attention="cache", kv_fused_step=True)
    with pytest.raises(ValueError):
        e2e.DecoderModel(cfg, 1, 8, DEV, fused=True, attention="cache", kv_cache="bf16", kv_fused_step=True)
