#!/usr/bin/env python3
"""Generate tests/golden/fake_mxfp4.npz: inputs and outputs of the REFERENCE's fake MXFP4 path, executed here on CPU.

Run ONLY where the reference checkout exists (it is imported, never copied):

    python tests/golden/make_golden_mx.py

* ``t_<dt>`` / ``q_<dt>``: model/quantize.py::quantize_mxfp4_tensor on one tensor (blocks of 32: an all-zero block, a block at an
  exact power-of-two boundary, e2m1 ties, an outlier), dt in {fp32, bf16};
* ``x_*`` / ``w_*`` / ``perm_*`` / ``qx_*`` / ``qw_*``: fake_reorder_quantize_{x,w}(dtype='MXFP4') in the form of the commented-out
  model/qLinearLayer.py:58 (channels reordered by ``perm`` first, then the identity index and select_num = KE), KE in {0, 64}.

model/quantize.py does ``import agemm`` at import time; an empty stand-in module is registered for that name, as make_golden.py
does.  Only data (bit patterns) is written."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ARCQ_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests.golden.make_golden import bits, outlier_activations  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    assert os.path.isdir(REF), "the reference checkout is required"
    sys.modules.setdefault("agemm", types.ModuleType("agemm"))
    quant = _load("ref_quantize", os.path.join(REF, "model/quantize.py"))
    out = {}
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        g = torch.Generator().manual_seed(4551)
        t = (torch.randn(40, 256, generator=g) * 2.5).to(dt)
        t[0, :32] = 0                                                     # all-zero block
        t[1, :32] = torch.linspace(-3, 3, 32).to(dt)                      # amax / 6 = 2^-1 exactly
        t[1, 5] = 6.0
        t[2, :16] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * 2).to(dt)   # e2m1 ties at scale 1
        t[2, 8:16] = -t[2, :8]
        t[3, 40] = 300.0
        t[4, 64:96] = (torch.rand(32, generator=g) * 1e-3).to(dt)
        out[f"t_{name}"] = bits(t)
        out[f"q_{name}"] = bits(quant.quantize_mxfp4_tensor(t.clone()))
        for KE in (0, 64):
            M, N, K = 24, 40, 256
            x = outlier_activations(M, K, 7 + KE).to(dt)
            w = (torch.randn(N, K, generator=g) * 0.5).to(dt)
            perm = torch.randperm(K, generator=g)
            qx, _, _ = quant.fake_reorder_quantize_x(torch.index_select(x, 1, perm), torch.arange(K), KE, dtype="MXFP4")
            qw, _, _ = quant.fake_reorder_quantize_w(torch.index_select(w, 1, perm), torch.arange(K), KE, dtype="MXFP4")
            key = f"{name}_KE{KE}"
            out[f"x_{key}"], out[f"w_{key}"] = bits(x), bits(w)
            out[f"perm_{key}"] = perm.numpy().astype(np.int64)
            out[f"qx_{key}"], out[f"qw_{key}"] = bits(qx), bits(qw)
    np.savez_compressed(os.path.join(HERE, "fake_mxfp4.npz"), **out)


if __name__ == "__main__":
    main()
