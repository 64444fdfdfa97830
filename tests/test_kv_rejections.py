"""Replays the two recorded tables of the paged KV cache's boundary (written by tests/golden/make_kv_rejections.py on the commit before
the argument checks were collapsed): which fault a bad call reports, and in which words, must be equal case by case.  No case of either
table can launch: the C cases expect a rejection or ARCQ_OK on an empty batch and pass stand-in addresses that are never dereferenced;
the Python cases are CPU tensors, and where tensors live is checked last."""
import importlib
import json
import os

import pytest
import torch

from arcquant_amd import _lib, kvstep

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY_POINTS = ("arcq_rope_qk", "arcq_kv_rope_append_quantize", "arcq_kv_rope_init_quantize", "arcq_kv_init", "arcq_kv_append", "arcq_kv_append_quantize",
                "arcq_kv_init_quantize", "arcq_kv_batch_decode", "arcq_kv_batch_prefill", "arcq_kv_decode_step")
SIZE_FNS = ("arcq_kv_decode_workspace_bytes", "arcq_kv_decode_step_state_bytes")


def test_c_rejections_are_those_of_the_recorded_table():
    """tests/golden/cabi_kv_rejections.json: status and arcq_last_error() text of the ten validating entry points of include/arcq_kv.h,
    and values of the two size functions (pure integer arithmetic)."""
    L = _lib.lib()
    table = json.load(open(os.path.join(GOLDEN, "cabi_kv_rejections.json")))
    calls = [c for c in table if c["fn"] not in SIZE_FNS]
    assert len(table) >= 300 and {c["fn"] for c in calls} == set(ENTRY_POINTS) and {c["fn"] for c in table} - set(ENTRY_POINTS) == set(SIZE_FNS)
    for fn in ENTRY_POINTS:
        assert sum(c["fn"] == fn for c in calls) >= 20, fn
    for c in calls:           # before any call: every expectation is a rejection or an empty return
        assert c["status"] in (-1, -2, -4, -5) or (c["status"] == 0 and (c["B"] == 0 or c["ntok"] == 0)), c
    for c in table:
        st = getattr(L, c["fn"])(*c["args"])
        assert st == c["status"], (c, st, L.arcq_last_error())
        if st and c["fn"] not in SIZE_FNS:
            assert L.arcq_last_error().decode() == c["error"], c


def _value(v):
    """A recorded argument: tensors are {"t": dtype, "shape": ..., "stride": ... (where not contiguous)}; their contents are never read."""
    if not isinstance(v, dict):
        return v
    if "dtype" in v:
        return getattr(torch, v["dtype"])
    if "state" in v:
        return kvstep.DecodeStepState(*v["state"], "cpu")
    if "t" not in v:
        return {k: _value(x) for k, x in v.items()}
    dtype, shape = getattr(torch, v["t"]), v["shape"]
    if "stride" not in v:
        return torch.zeros(shape, dtype=dtype)
    return torch.zeros(1 + sum((n - 1) * s for n, s in zip(shape, v["stride"])), dtype=dtype).as_strided(shape, v["stride"])


def test_python_rejections_are_those_of_the_recorded_table():
    """tests/golden/kv_python_rejections.json: the str() of the RuntimeError of every public function of kvcache, kvstep, kvprefill and
    kvrope for CPU arguments with one thing broken, and for the unbroken set ("... must live on the GPU")."""
    table = json.load(open(os.path.join(GOLDEN, "kv_python_rejections.json")))
    assert len(table) == 19 and sum(len(r["cases"]) for r in table) >= 800
    for r in table:           # before any call: every expectation is an error text, the device check only for an unbroken set
        assert r["cases"] and all(c["error"] and ("must live on the GPU" in c["error"]) == ("valid" in c["what"]) for c in r["cases"]), r["fn"]
        assert not r["base"] or r["cases"][-1]["what"] == "valid" and not r["cases"][-1]["over"], r["fn"]
    for r in table:
        mod, _, attr = r["fn"].partition(".")
        target = importlib.import_module("arcquant_amd." + mod)
        for c in r["cases"]:
            kwargs = {k: _value(v) for k, v in dict(r["base"], **c["over"]).items()}
            with pytest.raises(RuntimeError) as e:
                if "ctor" in kwargs:
                    cls, method = attr.split(".")
                    getattr(getattr(target, cls)(**kwargs.pop("ctor")), method)(**kwargs)
                else:
                    getattr(target, attr)(**kwargs)
            assert str(e.value) == c["error"], (r["fn"], c["what"])
