"""Every Python-level rejection of the boundary, in the ctypes mirror (arcquant_amd/agemm.py) and in the extension module (csrc/agemm_ext.cpp),
from CPU tensors.  Per function: a VALID argument set is built out of CPU tensors, one thing at a time is broken (each tensor's dtype, rank
and contiguity, each size relation the function checks) and the RuntimeError must name the broken argument; then the unbroken set is passed
and must be refused for living on the CPU.  Both modules check where tensors live LAST, so that final case shows that no call of this file
can reach a launch.  Also: the two modules keep one surface (names and keyword names)."""
import inspect
import os
import re

import pytest
import torch

from arcquant_amd import _build_ext, _lib, agemm

M, N, KQ, KE = 4, 64, 2048, 64
BF16, U8, I16, I32 = torch.bfloat16, torch.uint8, torch.int16, torch.int32


@pytest.fixture(scope="module")
def ext():
    if not os.path.exists(_build_ext.OUT):
        _build_ext.build_agemm_extension()
    return _build_ext.import_agemm_extension()


def z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def sf(rows, K):
    return z(U8, _lib.lib().arcq_sf_used_bytes(rows, K))


def gemm(M=M, N=N, K=KQ + KE):
    return dict(A=z(U8, M, K // 2), B=z(U8, N, K // 2), SFA=sf(M, K), SFB=sf(N, K), scale=1.0,
                bias=z(BF16, N), residual=z(BF16, M, N), out_dtype=BF16, out=z(BF16, M, N), scale_host=1.0)


def gemm_rw(M=M, N=N, K=KQ + KE, rows=None):
    """(RW, RSF) of ``rows`` weight rows (default N: they belong to the call)."""
    L, rows = _lib.lib(), N if rows is None else rows
    kw = gemm(M, N, K)
    del kw["B"], kw["SFB"]
    return dict(kw, RW=z(U8, L.arcq_repacked_w_bytes(rows, K)), RSF=z(U8, L.arcq_repacked_sf_bytes(rows, K)), N=N)


def fused(M=M, N=N, KQ=KQ, KE=KE):
    kw = gemm_rw(M, N, KQ + KE)
    del kw["A"], kw["SFA"]
    return dict(kw, X=z(BF16, M, KQ), W=z(BF16, KQ), eps=1e-6, reorder_index=torch.arange(KQ, dtype=I16), KE=KE, variant=None,
                act_scatter_index=torch.arange(N // 2, dtype=I16), absmax_slots=z(I32, 4), scale_w=1.0, layout=0)


def quant(KQ=KQ, KE=KE):
    return dict(X=z(BF16, M, KQ), W=z(BF16, M, KQ), GU=z(BF16, M, 2 * KQ), reorder_index=torch.arange(KQ, dtype=I16), KE=KE, variant=None,
                absmax_slots=z(I32, 4), layout=0)


def mx(M=M, N=32, K=128):
    return dict(gemm(M, N, K), SFA=z(U8, M, K // 32), SFB=z(U8, N, K // 32))


def but(kw, **over):
    return dict(kw, **over)


# name -> (valid keyword arguments, tensors without a rank rule, [(what is broken, broken arguments, pattern the message must match)])
CASES = {
    "matmul": (gemm(), {"SFA", "SFB"}, [
        ("K of B", but(gemm(), B=z(U8, N, 64)), "K"), ("short SFA", but(gemm(), SFA=sf(M, 64)), "SFA"), ("short SFB", but(gemm(), SFB=sf(N, 64)), "SFB"),
        ("out_dtype", but(gemm(), out_dtype=torch.float16, out=None), "out_dtype")]),
    "matmul_silu_mul": (gemm(), {"SFA", "SFB"}, [
        ("K of B", but(gemm(), B=z(U8, N, 64)), "K"), ("N % 8", gemm(N=68), "N % 8"), ("short SFA", but(gemm(), SFA=sf(M, 64)), "SFA"),
        ("short SFB", but(gemm(), SFB=sf(N, 64)), "SFB")]),
    "matmul_rw": (gemm_rw(), {"SFA"}, [
        ("foreign RW / RSF", gemm_rw(rows=N + 16), "RW"), ("short SFA", but(gemm_rw(), SFA=sf(M, 64)), "SFA"),
        ("out_dtype", but(gemm_rw(), out_dtype=torch.float16, out=None), "out_dtype")]),
    "matmul_repacked": (gemm_rw(), {"SFA"}, [
        ("foreign RW / RSF", gemm_rw(rows=N + 16), "RW"), ("short SFA", but(gemm_rw(), SFA=sf(M, 64)), "SFA"),
        ("outside repacked_supported", gemm_rw(M=129), "repacked_supported"), ("out_dtype", but(gemm_rw(), out_dtype=torch.float16, out=None), "out_dtype")]),
    "matmul_rw_silu_mul": (gemm_rw(), {"SFA"}, [
        ("foreign RW / RSF", gemm_rw(rows=N + 16), "RW"), ("N % 8", gemm_rw(N=68), "N % 8"), ("short SFA", but(gemm_rw(), SFA=sf(M, 64)), "SFA")]),
    "matmul_repacked_silu_absmax": (gemm_rw(), {"SFA"}, [
        ("foreign RW / RSF", gemm_rw(rows=N + 16), "RW"), ("N % 4", gemm_rw(N=66), "N % 4"), ("short SFA", but(gemm_rw(), SFA=sf(M, 64)), "SFA"),
        ("outside repacked_supported", gemm_rw(M=129), "repacked_supported")]),
    "rmsnorm_matmul_repacked": (fused(), set(), [
        ("KE", fused(KE=32), "KE"), ("reorder_index length", but(fused(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
        ("foreign RW / RSF", but(fused(), **{k: gemm_rw(rows=N + 16)[k] for k in ("RW", "RSF")}), "RW"), ("W length", but(fused(), W=z(BF16, 64)), "W"),
        ("outside fused_supported", fused(M=17), "fused_supported"), ("out_dtype", but(fused(), out_dtype=torch.float16, out=None), "out_dtype")]),
    "rmsnorm_matmul_repacked_silu": (fused(), set(), [
        ("KE", fused(KE=32), "KE"), ("reorder_index length", but(fused(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
        ("foreign RW / RSF", but(fused(), **{k: gemm_rw(rows=N + 16)[k] for k in ("RW", "RSF")}), "RW"), ("W length", but(fused(), W=z(BF16, 64)), "W"),
        ("N % 4", fused(N=66), "N % 4"), ("outside fused_supported", fused(M=17), "fused_supported")]),
    "dynamic_matmul_repacked": (fused(), set(), [
        ("KE", fused(KE=32), "KE"), ("reorder_index length", but(fused(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
        ("foreign RW / RSF", but(fused(), **{k: gemm_rw(rows=N + 16)[k] for k in ("RW", "RSF")}), "RW"),
        ("empty absmax_slots", but(fused(), absmax_slots=z(I32, 0)), "absmax_slots"), ("outside fused_supported", fused(M=17), "fused_supported"),
        ("out_dtype", but(fused(), out_dtype=torch.float16, out=None), "out_dtype")]),
    "reorder_quantize_x": (quant(), set(), [("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index")]),
    "reorder_quantize_w": (quant(), set(), [("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index")]),
    "rmsnorm_quantize_x": (but(quant(), W=z(BF16, KQ), eps=1e-6), set(), [
        ("KE", but(quant(KE=32), W=z(BF16, KQ), eps=1e-6), "K"), ("KQ outside 2048 .. 8192", but(quant(KQ=1024), W=z(BF16, 1024), eps=1e-6), "K"),
        ("W length", but(quant(), W=z(BF16, 64), eps=1e-6), "weight|K value"),
        ("reorder_index length", but(quant(), W=z(BF16, KQ), eps=1e-6, reorder_index=torch.arange(64, dtype=I16)), "reorder_index|K value")]),
    "reorder_quantize_x_dynamic": (quant(), set(), [
        ("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
        ("empty absmax_slots", but(quant(), absmax_slots=z(I32, 0)), "absmax_slots")]),
    "silu_mul_quantize_x_dynamic": (quant(), set(), [
        ("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
        ("odd GU width", but(quant(), GU=z(BF16, M, 2 * KQ + 1)), "GU"), ("layout", but(quant(), layout=2), "layout"),
        ("empty absmax_slots", but(quant(), absmax_slots=z(I32, 0)), "absmax_slots"), ("no reorder_index", but(quant(), reorder_index=None), "reorder_index")]),
    "absmax_scale": (dict(X=z(BF16, M, KQ)), {"X"}, []),
    "mx_reorder_quantize_x": (quant(), set(), [("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index"),
                                               ("KQ > 32767", quant(KQ=32768), "KQ")]),
    "mx_reorder_quantize_w": (quant(), set(), [("KE", quant(KE=32), "KE"), ("reorder_index length", but(quant(), reorder_index=torch.arange(64, dtype=I16)), "reorder_index")]),
    "mx_matmul": (mx(), set(), [
        ("K of B", but(mx(), B=z(U8, 32, 128)), "K"), ("K % 128", mx(K=192), "128"), ("N % 16", mx(N=24), "16"), ("SFA shape", but(mx(), SFA=z(U8, M, 2)), "SFA"),
        ("SFB shape", but(mx(), SFB=z(U8, 32, 2)), "SFB"), ("out_dtype", but(mx(), out_dtype=torch.float16, out=None), "out_dtype")]),
}
# pure data movement, on whatever device the tensors live: every rejection as above, and the unbroken call WORKS on CPU tensors
_rw = gemm_rw()
CPU_CASES = {
    "repack_w": (dict(QW=z(U8, N, (KQ + KE) // 2), SFW=sf(N, KQ + KE)), [
        ("K % 64", dict(QW=z(U8, N, 40), SFW=sf(N, KQ + KE)), "K % 64"), ("short SFW", dict(QW=z(U8, N, (KQ + KE) // 2), SFW=sf(N, 64)), "scale buffer")]),
    "unrepack_w": (dict(RW=_rw["RW"], RSF=_rw["RSF"], N=N, K=KQ + KE), [
        ("foreign RW / RSF", dict(RW=_rw["RW"], RSF=_rw["RSF"], N=N + 16, K=KQ + KE), "RW"), ("N = 0", dict(RW=_rw["RW"], RSF=_rw["RSF"], N=0, K=KQ + KE), "RW"),
        ("K % 64", dict(RW=_rw["RW"], RSF=_rw["RSF"], N=N, K=KQ + KE + 32), "RW")]),
}
OPTIONAL = ("bias", "residual", "out", "act_scatter_index")        # tensors with one exact shape: a shorter one is named


def keywords(fn):
    """Keyword names of a Python function, or of a pybind11 function (from the signature in its __doc__)."""
    if not inspect.isbuiltin(fn):
        return list(inspect.signature(fn).parameters)
    sig = fn.__doc__.splitlines()[0]
    return re.findall(r"(\w+): ", sig[sig.index("(") : sig.rindex(") ->")])


def broken(kw, no_rank):
    """One fault per tensor argument and kind -> (what, arguments, pattern)."""
    for name, t in kw.items():
        if not isinstance(t, torch.Tensor):
            continue
        yield f"dtype of {name}", but(kw, **{name: t.to(torch.float64)}), name
        yield f"contiguity of {name}", but(kw, **{name: torch.stack([t, t], dim=-1)[..., 0]}), name
        if name not in no_rank:
            yield f"rank of {name}", but(kw, **{name: t.unsqueeze(0)}), name
        if name in OPTIONAL:
            yield f"shape of {name}", but(kw, **{name: t[..., :-1].contiguous()}), name


def modules(ext):
    return (("mirror", agemm), ("extension", ext))


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_rejection_is_reachable_with_cpu_tensors_and_the_device_is_checked_last(ext, name):
    valid, no_rank, specific = CASES[name]
    for label, mod in modules(ext):
        fn = getattr(mod, name, None)
        if fn is None:
            assert label == "extension", name
            continue
        take = set(keywords(fn))
        need = [k for k, p in inspect.signature(fn).parameters.items() if p.default is inspect.Parameter.empty] if label == "mirror" else []
        assert set(need) <= set(valid), (name, need)

        def call(kw):
            return fn(**{k: v for k, v in kw.items() if k in take})

        for what, kw, pattern in list(broken({k: v for k, v in valid.items() if k in take}, no_rank)) + specific:
            if pattern in valid and pattern not in take:
                continue                                                   # (a keyword this module's function does not have)
            with pytest.raises(RuntimeError, match=pattern):
                call(kw)
                pytest.fail(f"{label}.{name} accepted a broken {what}")
        with pytest.raises(RuntimeError, match="GPU"):
            call(valid)


def test_scatter_index_must_be_a_permutation():
    with pytest.raises(RuntimeError, match="permutation"):
        agemm.rmsnorm_matmul_repacked_silu(**{k: v for k, v in but(fused(), act_scatter_index=z(I16, N // 2)).items()
                                              if k in keywords(agemm.rmsnorm_matmul_repacked_silu)})


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_data_movement_functions_reject_the_same_way_and_run_on_cpu_tensors(ext, name):
    valid, specific = CPU_CASES[name]
    for label, mod in modules(ext):
        fn = getattr(mod, name, None)
        if fn is None:
            continue
        for what, kw, pattern in list(broken(valid, set())) + specific:
            with pytest.raises(RuntimeError, match=pattern):
                fn(**kw)
                pytest.fail(f"{label}.{name} accepted a broken {what}")
        a, b = fn(**valid)
        assert not a.is_cuda and not b.is_cuda


def test_every_public_function_is_covered(ext):
    covered = set(CASES) | set(CPU_CASES)
    helpers = {"variant_for_kq", "sf_buffer_bytes", "mx_k_padded", "rw_route", "repacked_supported", "fused_supported"}      # integers in, integer out
    kv = {"batch_decode_i4", "init_kv_i4", "append_kv_i4", "batch_decode_f16", "init_kv_f16", "append_kv_f16"}
    public = {n for n, f in vars(agemm).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == agemm.__name__}
    assert public - helpers - kv == covered
    bound = {n for n in dir(ext) if callable(getattr(ext, n)) and not n.startswith("_")}
    assert bound - helpers - kv <= covered
    for n in kv:
        for mod in (agemm, ext):
            with pytest.raises(NotImplementedError):
                getattr(mod, n)(1, 2, 3)


def test_the_two_modules_keep_one_surface(ext):
    """Every function the extension binds exists in the mirror under that name, and its keyword names are, in order, keyword names of the
    mirror's function."""
    for n in dir(ext):
        f = getattr(ext, n)
        if n.startswith("_") or not callable(f):
            continue
        g = getattr(agemm, n, None)
        assert callable(g), n
        if "*args" in f.__doc__:                                           # the KV stubs take anything, in both modules
            continue
        theirs, ours = keywords(f), keywords(g)
        if all(re.fullmatch(r"arg\d+", k) for k in theirs):                 # bound without names (the integer helpers): same arity
            assert len(theirs) == len(ours), n
            continue
        it = iter(ours)
        assert all(k in it for k in theirs), (n, theirs, ours)
