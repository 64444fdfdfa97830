"""The harness's opt-in RoPE (``DecoderModel(rope=True)``, ``-m gpu``) on the toy of tests/test_e2e_kv_gpu.py: a prefill and three decode
steps.

Positions are right: layer 0's inputs do not depend on attention, so the K rows a ``rope=True`` model holds at position t are
``apply_rope`` at position t of the rows the ``rope=False`` model holds there -- byte for byte, in the dense cache and (after the
reference quantisation) in the int4 pages, with and without ``kv_paged_prefill``.  The int4 chain and the one-launch step agree bit for
bit, tables of (ones, zeros) change nothing, real tables change the logits, and a captured step replays to the eager logits."""
import functools

import numpy as np
import pytest
import torch

from tests import kv_reference as R
from tests import rope_reference as RR
from tests.test_e2e_kv_gpu import BSZ, PREFILL, _np_tables, _toy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEPS = 3
T = PREFILL + STEPS
THETA = 1e6                      # DecoderModel's default rope_theta


def _tokens(cfg):
    gen = torch.Generator(device=DEV).manual_seed(11)
    tok = torch.randint(0, cfg.vocab_size, (BSZ, PREFILL), device=DEV, generator=gen)
    return tok, [torch.randint(0, cfg.vocab_size, (BSZ, 1), device=DEV, generator=gen) for _ in range(STEPS)]


@functools.lru_cache(maxsize=None)
def _run(rope=False, identity=False, **kw):
    """A prefill and STEPS decode steps of one model -> logits of every call, the int4 pages / parameters after every call (or the dense
    K / V at the end), all on the CPU.  Built once per configuration and shared; nothing may modify it."""
    e2e, cfg = _toy()
    tok, nxt = _tokens(cfg)
    tables = (torch.ones((T, 128), dtype=torch.bfloat16), torch.zeros((T, 128), dtype=torch.bfloat16)) if identity else None
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, T, DEV, attention="cache", rope=rope or identity, rope_tables=tables, **kw)
        out = dict(logits=[], pages=[], scales=[])
        for i in range(STEPS + 1):
            out["logits"].append((m.forward(tok, 0) if i == 0 else m.forward(nxt[i - 1], PREFILL + i - 1)).cpu())
            if m.kvc is not None:
                out["pages"].append(m.kvc.pages.cpu().numpy())
                out["scales"].append(m.kvc.scales.cpu().numpy().view(np.uint16))
        if m.kvc is None:
            out["kc"], out["vc"] = m.layers[0]["kc"].cpu(), m.layers[0]["vc"].cpu()
        else:
            out["tables"] = _np_tables(m.kvc.tables(T))
        assert all(torch.isfinite(x.float()).all() for x in out["logits"])
    return out


def _rows(x):
    """dense cache [B, nh, T, 128] -> [B * T, nh, 128], token b * T + t."""
    return x.transpose(1, 2).reshape(BSZ * T, -1, 128).contiguous()


@functools.lru_cache(maxsize=None)
def _rotated_rows():
    """The rows of the rope=False dense model, its K rotated to position t by the reference -> (k_rot, v), [B * T, nh, 128] on the CPU."""
    plain = _run(fused=True)
    cos, sin = RR.rope_tables(T, THETA, torch.bfloat16)
    pos = np.tile(np.arange(T), BSZ)
    return RR.apply_rope(_rows(plain["kc"]), pos, cos, sin), _rows(plain["vc"])


def test_dense_cache_holds_the_rows_rotated_to_their_positions():
    k_rot, v = _rotated_rows()
    got = _run(rope=True, fused=True)
    assert torch.equal(_rows(got["kc"]).view(torch.int16), k_rot.view(torch.int16)), "prefill (torch) or decode (harness kernel) positions"
    assert torch.equal(_rows(got["vc"]).view(torch.int16), v.view(torch.int16))
    assert not torch.equal(_rows(_run(fused=True)["kc"])[1:], k_rot[1:])


@pytest.mark.parametrize("paged", [False, True], ids=["sdpa-prefill", "paged-prefill"])
def test_int4_pages_hold_the_reference_quantisation_of_the_rotated_rows(paged):
    k_rot, v = _rotated_rows()
    got = _run(rope=True, fused=True, kv_cache="int4", kv_paged_prefill=paged)
    data, param = np.zeros_like(got["pages"][-1]), np.zeros(got["scales"][-1].shape, dtype=np.float16)
    (kq, kp), (vq, vp) = R.quantize_i4(k_rot), R.quantize_i4(v)
    R.write_rows(data, param, *got["tables"], kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), np.arange(BSZ + 1) * T, 0)
    assert np.array_equal(got["pages"][-1], data)
    assert np.array_equal(got["scales"][-1], param.view(np.uint16))


@pytest.mark.parametrize("fused,quant_type", [(True, "NVFP4"), (False, "NVFP4"), (True, "MXFP4")])
def test_int4_chain_and_one_launch_step_agree(fused, quant_type):
    chain = _run(rope=True, fused=fused, quant_type=quant_type, kv_cache="int4")
    step = _run(rope=True, fused=fused, quant_type=quant_type, kv_cache="int4", kv_fused_step=True)
    for i in range(STEPS + 1):
        assert torch.equal(chain["logits"][i], step["logits"][i]), f"call {i}: logits"
        assert np.array_equal(chain["pages"][i], step["pages"][i]), f"call {i}: pages"
        assert np.array_equal(chain["scales"][i], step["scales"][i]), f"call {i}: parameters"


def test_identity_tables_change_nothing():
    """(ones, zeros): x * 1 + rot(x) * 0.  Logits and pages are compared, not q bytes: -0 * 1 + 0 is +0."""
    for kw in (dict(fused=True), dict(fused=True, kv_cache="int4"), dict(fused=True, kv_cache="int4", kv_paged_prefill=True),
               dict(fused=True, kv_cache="int4", kv_fused_step=True)):
        plain, ident = _run(**kw), _run(identity=True, **kw)
        for i in range(STEPS + 1):
            assert torch.equal(plain["logits"][i], ident["logits"][i]), (kw, i)
        if "pages" in plain and plain["pages"]:
            assert np.array_equal(plain["pages"][-1], ident["pages"][-1]) and np.array_equal(plain["scales"][-1], ident["scales"][-1]), kw
        else:
            assert torch.equal(plain["kc"], ident["kc"]) and torch.equal(plain["vc"], ident["vc"])


def test_rotation_changes_the_result():
    for kw in (dict(fused=True), dict(fused=True, kv_cache="int4")):
        plain, rot = _run(**kw), _run(rope=True, **kw)
        assert all(not torch.equal(a, b) for a, b in zip(plain["logits"], rot["logits"])), kw


def test_trace_records_what_attention_consumed():
    """With rope=True the trace holds the rotated q and k: the step's pages are the reference quantisation of the traced rows."""
    e2e, cfg = _toy()
    tok, nxt = _tokens(cfg)
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, T, DEV, fused=True, attention="cache", kv_cache="int4", rope=True)
        m.forward(tok, 0)
        data, param = m.kvc.pages.cpu().numpy().copy(), m.kvc.scales.cpu().numpy().copy()
        m.kv_trace = []
        m.forward(nxt[0], PREFILL)
    tr = m.kv_trace[0]
    k_rot, _ = _rotated_rows()
    want_k = k_rot.view(BSZ, T, -1, 128)[:, PREFILL]
    assert torch.equal(tr["k"].cpu().view(torch.int16), want_k.contiguous().view(torch.int16))
    (kq, kp), (vq, vp) = R.quantize_i4(tr["k"].cpu()), R.quantize_i4(tr["v"].cpu())
    R.write_rows(data, param, *_np_tables(m.kvc.tables(PREFILL + 1)), kq.numpy(), vq.numpy(), kp.numpy(), vp.numpy(), None, 0)
    assert np.array_equal(m.kvc.pages.cpu().numpy(), data) and np.array_equal(m.kvc.scales.cpu().numpy().view(np.uint16), param.view(np.uint16))


def test_rope_int4_decode_step_replays_from_a_graph():
    e2e, cfg = _toy()
    tok, nxt = _tokens(cfg)
    with torch.no_grad():
        m = e2e.DecoderModel(cfg, BSZ, T, DEV, fused=True, attention="cache", kv_cache="int4", rope=True)
        m.forward(tok, 0)
        want = m.forward(nxt[0], PREFILL).clone()
        torch.cuda.synchronize()
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            m.forward(nxt[0], PREFILL)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                out = m.forward(nxt[0], PREFILL)
        torch.cuda.synchronize()
        for _ in range(3):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
