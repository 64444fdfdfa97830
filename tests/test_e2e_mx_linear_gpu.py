"""DecoderModel(quant_type="MXFP4", fused=True, mx_fused_linears=...) on the MI355X (``-m gpu``): a two-layer model on a small config whose
decode step at bs = 4 runs q|k|v, o and gate|up through the fused linears (mx.linear_rmsnorm_repacked, mx.linear_quantize_repacked,
mx.linear_rmsnorm_silu_repacked) gives the logits of the flag-off model bit for bit, eagerly and replayed from a HIP graph, under
mx_repacked_decode and under mx_repacked_only; calls of more than 16 tokens take the unfused path and agree too."""
import pytest
import torch

from arcquant_amd import mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = "qkv,o,gateup"


def _toy():
    from arcquant_amd import e2e
    return e2e, e2e.ModelConfig("toy", num_layers=2, num_heads=4, hidden_size=2048, intermediate_size=4096, vocab_size=512)


class _Count:
    """Counts the fused launches of a model call (the wrappers are looked up on the module at every call)."""
    NAMES = ("linear_rmsnorm_repacked", "linear_quantize_repacked", "linear_rmsnorm_silu_repacked")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(mx, name, self._wrap(name, getattr(mx, name)))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return counted

    def take(self):
        out, self.n = tuple(self.n[k] for k in self.NAMES), dict.fromkeys(self.NAMES, 0)
        return out


@pytest.mark.parametrize("flag", ["mx_repacked_decode", "mx_repacked_only"])
def test_fused_linears_give_equal_logits(flag, monkeypatch):
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(2)
    tok = torch.randint(0, cfg.vocab_size, (4, 5), generator=g).to(dev)          # 20 tokens: beyond the fused linears
    nxt = torch.randint(0, cfg.vocab_size, (4, 1), generator=g).to(dev)
    count = _Count(monkeypatch)
    with torch.no_grad():
        off = e2e.DecoderModel(cfg, 4, 8, dev, fused=True, quant_type="MXFP4", **{flag: True})
        on = e2e.DecoderModel(cfg, 4, 8, dev, fused=True, quant_type="MXFP4", mx_fused_linears=ALL, **{flag: True})
        assert on.mx_fuse == {"qkv", "o", "gateup"} and not off.mx_fuse
        assert torch.equal(on.forward(tok, 0), off.forward(tok, 0))
        assert count.take() == (0, 0, 0), "a 20-token call took a fused linear"
        want = off.forward(nxt, 5)
        assert count.take() == (0, 0, 0), "the flag-off model took a fused linear"
        assert torch.equal(on.forward(nxt, 5), want)
        assert count.take() == (2, 2, 2), "the decode step did not fuse q|k|v, o and gate|up of both layers"
        torch.cuda.synchronize()
        graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(st):
            with torch.cuda.graph(graph, stream=st):
                logits = on.forward(nxt, 5)
        torch.cuda.synchronize()
        for _ in range(2):
            logits.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(logits, want)
        # each linear fused alone: the same logits, and only that linear's launches
        for one, n in (("qkv", (2, 0, 0)), ("o", (0, 2, 0)), ("gateup", (0, 0, 2))):
            on.mx_fuse = frozenset((one,))
            count.take()
            assert torch.equal(on.forward(nxt, 5), want), one
            assert count.take() == n, one


def test_a_17_token_call_takes_the_unfused_path(monkeypatch):
    e2e, cfg = _toy()
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(3)
    tok17 = torch.randint(0, cfg.vocab_size, (1, 17), generator=g).to(dev)
    tok16 = tok17[:, :16].contiguous()
    count = _Count(monkeypatch)
    with torch.no_grad():
        off = e2e.DecoderModel(cfg, 1, 24, dev, fused=True, quant_type="MXFP4", mx_repacked_only=True)
        on = e2e.DecoderModel(cfg, 1, 24, dev, fused=True, quant_type="MXFP4", mx_repacked_only=True, mx_fused_linears=ALL)
        assert torch.equal(on.forward(tok17, 0), off.forward(tok17, 0))
        assert count.take() == (0, 0, 0), "a 17-token call took a fused linear"
        assert torch.equal(on.forward(tok16, 0), off.forward(tok16, 0))          # 16 tokens: the last fused size
        assert count.take() == (2, 2, 2)


def test_bench_decode_reports_the_flag():
    e2e, cfg = _toy()
    e2e.MODEL_CFGS["toy"] = cfg
    try:
        out = e2e.bench_decode("toy", batch=2, prefill=16, steps=2, repeats=1, fused=True, quant_type="MXFP4", mx_repacked_only=True,
                               mx_fused_linears="o,qkv")
    finally:
        del e2e.MODEL_CFGS["toy"]
    assert out["mx_fused_linears"] == "o,qkv" and out["mx_repacked_only"] is True and out["decode_tok_per_s"] > 0
