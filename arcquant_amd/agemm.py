"""Drop-in mirror of the reference's pybind11 module ``agemm`` (kernels/src/bindings.cpp:551-575).

Same function names, argument names, argument meaning, return shapes/dtypes and error behaviour
(``RuntimeError`` on an unsupported shape) as the reference, but every call goes through the C-ABI of
``libarcq_hip.so`` (hand-written gfx950 kernels).  ``torch`` is used only for device memory and the
current HIP stream.

Differences a caller can observe, all deliberate (DESIGN.md "deviations"):
  * launches go to torch's CURRENT stream (the reference uses the legacy default stream), so the ops are
    capturable in HIP graphs and ordered with surrounding torch work without device-wide syncs;
  * KQ is not limited to the reference's closed template list (bindings.cpp:141-160);
  * ``matmul(..., scale)`` also accepts a 0-dim device tensor WITHOUT a device->host sync;
  * ``rmsnorm_quantize_x`` uses the same augmented-K layout as the weights for KQ=3584 (the reference
    mixes the two layouts there); ``variant=VARIANT_G16`` reproduces the reference's layout.  This op is
    "parity unpinned" against the CUDA binary (CUDA ``rsqrtf`` is a 2-ulp approximation; kernel and oracle use
    the correctly rounded value): it is byte-exact to the restated kernel text, not provably to the reference.
"""
from __future__ import annotations

import functools

import torch

from . import _lib
from ._lib import VARIANT_G16, VARIANT_G32, OUT_BF16, OUT_F32, ArcqError  # noqa: F401  (re-exported)

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    # the current HIP stream of the tensor's device as an integer handle.  The private accessor (what torch's own extensions use)
    # saves ~1.5 us per call over building a torch.cuda.Stream object; an eager decode step makes ~170 of these calls and is
    # host-paced (tools/host_overhead.py)
    if _raw_stream is not None:
        return _raw_stream(t.get_device())             # (a GPU tensor always knows its index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _on:
    """``with _on(device):`` -- torch.cuda.device(device), but free when the device is already current (the usual case)."""
    __slots__ = ("ctx",)

    def __init__(self, device):
        idx = device.index
        self.ctx = None if idx is None or idx == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


# Every function validates in one order: dtype / rank / contiguity of its tensors (_need), the shape and size relations between them, out_dtype,
# the optional tensors (_out, _opt, _slots: dtype, rank, contiguity and shape at once), and LAST where everything lives (_same_device).  So
# every rejection but the last is reachable with CPU tensors, and a call built from CPU tensors cannot get as far as a launch.  Shape rules
# of the kernels themselves (K % 64, alignment, size limits) are the C-ABI's.

def _need(t: torch.Tensor, dtype, name: str, ndim=None):
    # the reference's data_ptr<T>() throws c10::Error on a dtype mismatch; we raise RuntimeError
    if getattr(t, "dtype", None) is not dtype:            # (dtypes are singletons; whatever is not a tensor has none of them)
        raise RuntimeError(f"agemm: {name} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError(f"agemm: {name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"agemm: {name} must be contiguous")


def _opt(t, dtype, name, shape):
    if t is None:
        return None
    _need(t, dtype, name, len(shape))
    if t.shape != shape:
        raise RuntimeError(f"agemm: {name} must have shape {shape}")
    return t.data_ptr()


def _slots(t, who):
    # abs-max words left by a producing kernel -> (pointer, count)
    if t is None:
        return None, 0
    _need(t, torch.int32, "absmax_slots", 1)
    if t.numel() == 0:
        raise RuntimeError(f"agemm.{who}: absmax_slots must not be empty")
    return t.data_ptr(), t.numel()


def _alpha(scale, scale_host):
    # the reference's ``scale`` -> (host factor, device tensor or None, its address): a 1-element fp32 device tensor is read on the device,
    # anything else is a host float
    if isinstance(scale, torch.Tensor) and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1:
        return float(scale_host), scale, scale.data_ptr()
    return float(scale_host) * float(scale), None, None   # CPU tensor or other dtype: same as the reference's __float__


def _alpha_as_f32(scale, scale_host):
    # the SiLU-epilogue GEMMs read ANY device ``scale`` tensor on the device, as fp32
    if isinstance(scale, torch.Tensor) and scale.is_cuda:
        scale = scale.reshape(-1)[:1].to(torch.float32)
        return float(scale_host), scale, scale.data_ptr()
    return float(scale_host) * float(scale), None, None


_OUT_CODES = {torch.bfloat16: OUT_BF16, torch.float32: OUT_F32}


def _out(out, M, N, out_dtype, like, who):
    # -> (the caller's ``out`` if it is [M, N] of out_dtype, else a new tensor next to ``like``; the C-ABI's code of out_dtype)
    code = _OUT_CODES.get(out_dtype)
    if code is None:
        raise RuntimeError(f"agemm.{who}: out_dtype must be bfloat16 or float32")
    if out is None:
        return torch.empty((M, N), dtype=out_dtype, device=like.device), code
    _need(out, out_dtype, "out", 2)
    if out.shape != (M, N):
        raise RuntimeError(f"agemm.{who}: out has the wrong shape, expected ({M}, {N})")
    return out, code


def _same_device(who: str, A: torch.Tensor, *ts):
    # the device guard and the stream of a call are those of its first operand: a tensor elsewhere would hand the kernel a pointer it cannot read
    # (get_device(): the GPU's index, -1 on the CPU; it costs half of comparing torch.device objects, and a decode step makes ~170 calls)
    idx = A.get_device()
    if idx < 0:
        raise RuntimeError(f"agemm.{who}: the operands must live on the GPU (there is no CPU path)")
    for t in ts:
        if t is not None and t.get_device() != idx:
            raise RuntimeError(f"agemm.{who}: every operand must live on the GPU of the first one ({A.device}), got {t.device}")


def _debug_set_tile_overlap_tail(mode: int) -> None:
    """DEBUG / tests: which launches of the LDS-tiled GEMM take the kernel whose output stores leave under its last K step
    (arcq_debug_set_tile_overlap_tail): 0 never, 1 the 256 x 256 tile's launches of whole tiles except SiLU * up (the default), 2 whenever
    legal: SiLU * up too, and every shape made of whole 256 x 256 tiles takes that tile, whatever the routes and heuristics would choose.
    Process-wide; read at every launch."""
    fn = _lib.lib().arcq_debug_set_tile_overlap_tail
    fn.restype, fn.argtypes = None, [_lib._i32]
    fn(int(mode))
    rw_route.cache_clear()                          # (the route of a shape depends on the mode)


def _debug_set_tile_pair_loads(on: int) -> None:
    """DEBUG / tests: whether a launch that takes the overlapped-tail kernel with the plain epilogue takes its paired-load sibling, which
    requests a row's two following K atoms back to back (arcq_debug_set_tile_pair_loads): 1 yes (the default), 0 no.  Process-wide; read
    at every launch.  Which launches are eligible stays _debug_set_tile_overlap_tail's rule."""
    fn = _lib.lib().arcq_debug_set_tile_pair_loads
    fn.restype, fn.argtypes = None, [_lib._i32]
    fn(int(on))


def _debug_set_tile_quad_loads(on: int) -> None:
    """DEBUG / tests: whether a launch that takes the paired-load sibling over the reference B layout takes the quad-load sibling instead,
    which requests a row's four following K atoms back to back (arcq_debug_set_tile_quad_loads): 1 yes (the default), 0 no.  Process-wide;
    read at every launch.  Inert while _debug_set_tile_pair_loads is 0."""
    fn = _lib.lib().arcq_debug_set_tile_quad_loads
    fn.restype, fn.argtypes = None, [_lib._i32]
    fn(int(on))


@functools.lru_cache(maxsize=None)
def variant_for_kq(KQ: int) -> int:
    """Layout variant the reference's dispatch picks for this in_features (bindings.cpp:141-160)."""
    return int(_lib.lib().arcq_variant_for_kq(int(KQ)))


@functools.lru_cache(maxsize=None)
def sf_buffer_bytes(rows: int, K: int) -> int:
    """get_sf{a,b}_buffer_size_in_bytes (bindings.cpp:83-95)."""
    return int(_lib.lib().arcq_sf_alloc_bytes(int(rows), int(K)))


@functools.lru_cache(maxsize=None)
def _sf_used(rows: int, K: int) -> int:
    return int(_lib.lib().arcq_sf_used_bytes(int(rows), int(K)))


@functools.lru_cache(maxsize=None)
def _repacked_bytes(N: int, K: int):
    L = _lib.lib()
    return int(L.arcq_repacked_w_bytes(N, K)), int(L.arcq_repacked_sf_bytes(N, K))


def _need_repacked(RW, RSF, SFA, M, N, K, who, n_mult=1):
    # (RW, RSF) is the repacked weight of N rows over this K (n_mult > 1: whose rows interleave gate and up), SFA the scales of A [M, K] or None
    _need(RW, torch.uint8, "RW", 1)
    _need(RSF, torch.uint8, "RSF", 1)
    if K % 64 or N % n_mult or (RW.numel(), RSF.numel()) != _repacked_bytes(N, K):
        raise RuntimeError(f"Value error in {who}: RW / RSF do not belong to a [{N}, {K}] weight" + (f", or N % {n_mult} != 0" if n_mult > 1 else ""))
    if SFA is not None and SFA.numel() < _sf_used(M, K):
        raise RuntimeError(f"Value error in {who}: SFA smaller than the swizzled layout of A")


def _quantize(fn_name: str, X: torch.Tensor, reorder_index: torch.Tensor, KE: int, variant):
    _need(X, torch.bfloat16, "X" if fn_name.endswith("_x") else "W", 2)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    rows, KQ = X.shape
    KE = int(KE)
    if reorder_index.numel() != KQ:
        raise RuntimeError(f"agemm: reorder_index has {reorder_index.numel()} entries, expected {KQ}")
    K = KQ + KE
    if variant is None:
        variant = variant_for_kq(KQ)
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ:
        raise RuntimeError(f"Value error in {fn_name}: KQ={KQ}, KE={KE} is not valid")
    _same_device(fn_name, X, reorder_index)
    Q = torch.empty((rows, K // 2), dtype=torch.uint8, device=X.device)
    SF = torch.empty((sf_buffer_bytes(rows, K),), dtype=torch.uint8, device=X.device)
    L = _lib.lib()
    fn = L.arcq_quantize_x if fn_name.endswith("_x") else L.arcq_quantize_w
    with _on(X.device):
        st = fn(X.data_ptr(), reorder_index.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, int(variant), _stream(X))
    _lib.check(st, fn_name)
    return Q, SF


def reorder_quantize_x(X: torch.Tensor, reorder_index: torch.Tensor, KE: int, variant=None):
    """agemm.reorder_quantize_x(X, reorder_index, KE) -> (QX u8 [M,(KQ+KE)/2], SFX u8 [(M/128+1)*128*(KQ+KE)/16])
    (bindings.cpp:122-163)."""
    return _quantize("reorder_quantize_x", X, reorder_index, KE, variant)


def reorder_quantize_w(W: torch.Tensor, reorder_index: torch.Tensor, KE: int, variant=None):
    """agemm.reorder_quantize_w(W, reorder_index, KE) -> (QW, SFW) (bindings.cpp:170-210)."""
    return _quantize("reorder_quantize_w", W, reorder_index, KE, variant)


def rmsnorm_quantize_x(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int, variant=None):
    """agemm.rmsnorm_quantize_x(X, W, eps, reorder_index, KE) -> (QX, SFX) (bindings.cpp:216-254)."""
    _need(X, torch.bfloat16, "X", 2)
    _need(W, torch.bfloat16, "W", 1)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    M, KQ = X.shape
    KE = int(KE)
    K = KQ + KE
    if W.numel() != KQ or reorder_index.numel() != KQ:
        raise RuntimeError("agemm: rmsnorm weight / reorder_index length must equal X.shape[1]")
    if variant is None:
        variant = variant_for_kq(KQ)
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or not (2048 <= KQ <= 8192):
        raise RuntimeError(f"Value error in run_rmsnorm_x_bf16_nvfp4: K value is not valid: {KQ}")
    _same_device("rmsnorm_quantize_x", X, W, reorder_index)
    QX = torch.empty((M, K // 2), dtype=torch.uint8, device=X.device)
    SFX = torch.empty((sf_buffer_bytes(M, K),), dtype=torch.uint8, device=X.device)
    with _on(X.device):
        st = _lib.lib().arcq_rmsnorm_quantize_x(X.data_ptr(), W.data_ptr(), float(eps), reorder_index.data_ptr(), QX.data_ptr(),
                                                SFX.data_ptr(), M, KQ, KE, int(variant), _stream(X))
    _lib.check(st, "rmsnorm_quantize_x")
    return QX, SFX


def matmul(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale, *, bias=None, residual=None,
           out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """agemm.matmul(A, B, SFA, SFB, scale) -> bf16 [M, N]  (bindings.cpp:99-120).

    ``scale`` may be a Python float (the reference's ``const float``) or a 0-dim / 1-element fp32 device
    tensor; the latter is consumed on the device (the reference converts it with an implicit ``.item()``
    sync).  Extensions used by the host mirror / e2e harness: ``bias`` (bf16 [N]), ``residual`` (bf16 [M,N], added
    after the bf16 rounding, like ``x + linear(...)``), ``out_dtype=torch.float32``, ``out``, and ``scale_host`` (a host
    float multiplied into a device ``scale``: weight scale x activation scale without a tiny multiply kernel).
    """
    _need(A, torch.uint8, "A", 2)
    _need(B, torch.uint8, "B", 2)
    _need(SFA, torch.uint8, "SFA")
    _need(SFB, torch.uint8, "SFB")
    M, N, K = A.shape[0], B.shape[0], A.shape[1] * 2       # bindings.cpp:107-109
    if B.shape[1] * 2 != K:
        raise RuntimeError(f"agemm.matmul: A has K={K}, B has K={B.shape[1] * 2}")
    if SFA.numel() < _sf_used(M, K) or SFB.numel() < _sf_used(N, K):
        raise RuntimeError("agemm.matmul: SFA / SFB smaller than the swizzled layout of its operand")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "matmul")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("matmul", A, B, SFA, SFB, alpha_dev, out, bias, residual)
    L = _lib.lib()
    ws_bytes = int(L.arcq_gemm_workspace_bytes(M, N, K))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=A.device) if ws_bytes else None
    with _on(A.device):
        st = L.arcq_gemm_nvfp4(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), out.data_ptr(), M, N, K,
                               alpha_host, alpha_p, bias_p, residual_p, oc, ws.data_ptr() if ws_bytes else None, ws_bytes, _stream(A))
    _lib.check(st, "matmul")
    return out


# ---- MXFP4 (quant_type='MXFP4'; include/arcq.h "MXFP4", DESIGN.md "MXFP4") ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def mx_k_padded(K: int) -> int:
    """round_up(K, 128): the stored K of an MXFP4 operand (codes [rows, Kp/2], scales [rows, Kp/32])."""
    return int(_lib.lib().arcq_mx_k_padded(int(K)))


def _mx_quantize(fn_name: str, X: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    xname = "X" if fn_name.endswith("_x") else "W"
    _need(X, torch.bfloat16, xname, 2)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    rows, KQ = X.shape
    KE = int(KE)
    if reorder_index.numel() != KQ:
        raise RuntimeError(f"agemm: reorder_index has {reorder_index.numel()} entries, expected {KQ}")
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or KQ > 32767:
        raise RuntimeError(f"Value error in {fn_name}: KQ={KQ}, KE={KE} is not valid")
    _same_device(fn_name, X, reorder_index)
    Kp = mx_k_padded(KQ + KE)
    Q = torch.empty((rows, Kp // 2), dtype=torch.uint8, device=X.device)
    SF = torch.empty((rows, Kp // 32), dtype=torch.uint8, device=X.device)
    L = _lib.lib()
    fn = L.arcq_mx_quantize_x if fn_name.endswith("_x") else L.arcq_mx_quantize_w
    with _on(X.device):
        st = fn(X.data_ptr(), reorder_index.data_ptr(), Q.data_ptr(), SF.data_ptr(), rows, KQ, KE, _stream(X))
    _lib.check(st, fn_name)
    return Q, SF


def mx_reorder_quantize_x(X: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    """MXFP4-ARC activation quantiser -> (QX u8 [M, Kp/2], SFX u8 E8M0 [M, Kp/32]); K = KQ + KE, Kp = round_up(K, 128).
    Positions [KQ, K) hold the quantised residual of reordered channels [KQ-KE, KQ)."""
    return _mx_quantize("mx_reorder_quantize_x", X, reorder_index, KE)


def mx_reorder_quantize_w(W: torch.Tensor, reorder_index: torch.Tensor, KE: int):
    """MXFP4-ARC weight quantiser -> (QW [N, Kp/2], SFW [N, Kp/32]); positions [KQ, K) copy reordered channels [KQ-KE, KQ)."""
    return _mx_quantize("mx_reorder_quantize_w", W, reorder_index, KE)


def mx_matmul(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale, *, bias=None, residual=None,
              out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """D = scale * deq(A) . deq(B)^T on the block-scaled fp4 MFMA -> [M, N] (bf16, or fp32 with ``out_dtype``).
    ``matmul``'s semantics for ``scale`` (float or 0-dim fp32 device tensor), ``bias``, ``residual`` (may alias ``out``),
    ``out`` and ``scale_host``.  N % 16 == 0."""
    for t, name in ((A, "A"), (B, "B"), (SFA, "SFA"), (SFB, "SFB")):
        _need(t, torch.uint8, name, 2)
    M, N, K = A.shape[0], B.shape[0], A.shape[1] * 2
    if B.shape[1] * 2 != K:
        raise RuntimeError(f"agemm.mx_matmul: A has K={K}, B has K={B.shape[1] * 2}")
    if K % 128:
        raise RuntimeError(f"agemm.mx_matmul: K={K} is not a padded MXFP4 K (a multiple of 128)")
    if N % 16:
        raise RuntimeError(f"agemm.mx_matmul: N={N} must be a multiple of 16")
    if tuple(SFA.shape) != (M, K // 32) or tuple(SFB.shape) != (N, K // 32):
        raise RuntimeError("agemm.mx_matmul: SFA / SFB must be [rows, K/32]")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "mx_matmul")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("mx_matmul", A, B, SFA, SFB, alpha_dev, out, bias, residual)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_mxfp4(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), out.data_ptr(), M, N, K,
                                        alpha_host, alpha_p, bias_p, residual_p, oc, None, 0, _stream(A))
    _lib.check(st, "mx_matmul")
    return out


def absmax_scale(X: torch.Tensor) -> torch.Tensor:
    """Extension: ``max|X| / (448*6)`` as a 0-dim fp32 device tensor, no host sync.
    Equals ``torch.max(x.abs()).float() / (448.0*6.0)`` of model/qLlamaLayer.py:74 bit for bit (0-dim, so that
    ``x / scale`` keeps x's dtype exactly as with the reference's scalar tensor)."""
    _need(X, torch.bfloat16, "X")
    _same_device("absmax_scale", X)
    out = torch.empty((1,), dtype=torch.float32, device=X.device)
    with _on(X.device):
        st = _lib.lib().arcq_absmax_scale(X.data_ptr(), X.numel(), out.data_ptr(), _stream(X))
    _lib.check(st, "absmax_scale")
    return out.reshape(())


_dyn_state = {}


def _quantize_dynamic(entry: str, who: str, X: torch.Tensor, KQ: int, reorder_index, KE: int, variant, slots=None, layout=None):
    M = X.shape[0]
    KE = int(KE)
    K = KQ + KE
    if variant is None:
        variant = variant_for_kq(KQ)
    if reorder_index is None:          # X is already in reordered channel order: NULL at the C-ABI (arcq_quantize_x_dyn_slots only)
        if entry != "arcq_quantize_x_dyn_slots":
            raise RuntimeError(f"Value error in {who}: reorder_index=None needs absmax_slots")
    else:
        _need(reorder_index, torch.int16, "reorder_index", 1)
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or (reorder_index is not None and reorder_index.numel() != KQ):
        raise RuntimeError(f"Value error in {who}: KQ={KQ}, KE={KE} or the length of reorder_index is not valid")
    slots_p, nslots = _slots(slots, who)
    _same_device(who, X, reorder_index, slots)
    dev = X.device
    QX = torch.empty((M, K // 2), dtype=torch.uint8, device=dev)
    SFX = torch.empty((sf_buffer_bytes(M, K),), dtype=torch.uint8, device=dev)
    scale = torch.empty((1,), dtype=torch.float32, device=dev)
    args = [X.data_ptr(), reorder_index.data_ptr() if reorder_index is not None else None, QX.data_ptr(), SFX.data_ptr(), scale.data_ptr()]
    if slots is not None:
        args += [slots_p, nslots]
    else:
        key = (dev, _stream(X))            # scratch of the abs-max pass: one per device and stream (include/arcq.h)
        state = _dyn_state.get(key)
        if state is None:
            state = _dyn_state[key] = torch.empty(256, dtype=torch.int32, device=dev)
        args.append(state.data_ptr())
    args += [M, KQ, KE, int(variant)]
    if layout is not None:
        args.append(int(layout))
    with _on(dev):
        st = getattr(_lib.lib(), entry)(*args, _stream(X))
    _lib.check(st, who)
    return QX, SFX, scale.reshape(())


def _sf_swizzle_offsets(N: int, K: int, dev):
    # offset in the swizzled ue4m3 layout of scale group g of row r (include/arcq.h), as an [N, K/16] index tensor
    r = torch.arange(N, device=dev).unsqueeze(1)
    g = torch.arange(K // 16, device=dev).unsqueeze(0)
    return ((r // 128) * (K // 64) + g // 4) * 512 + (r % 32) * 16 + ((r // 32) % 4) * 4 + g % 4


def repack_w(QW: torch.Tensor, SFW: torch.Tensor):
    """One-time re-layout of a quantised weight for the decode fast path (include/arcq.h, "REPACKED weight"): returns
    ``(RW, RSF)``.  Pure data movement with torch ops -- codes and scale bytes are those of ``reorder_quantize_w``:
    RW  = [row blocks of 16][tiles of 128 K][lane = 16*q + r][16 bytes], K padded to a multiple of 256, N to 16;
    RSF = [row blocks][tile pairs][lane][4 bytes: the lane's two scale bytes in each tile of the pair].
    ``unrepack_w`` is its inverse; both also run on CPU tensors."""
    _need(QW, torch.uint8, "QW", 2)            # (pure data movement: no device rule)
    _need(SFW, torch.uint8, "SFW", 1)
    N, K = QW.shape[0], QW.shape[1] * 2
    if K % 64 or SFW.numel() < _sf_used(N, K):
        raise RuntimeError("Value error in repack_w: K % 64 != 0 or the scale buffer is too small")
    dev = QW.device
    Np, Kp = (N + 15) // 16 * 16, (K + 255) // 256 * 256
    q = torch.zeros((Np, Kp // 2), dtype=torch.uint8, device=dev)
    q[:N, : K // 2] = QW
    # natural [N, K/16] scale matrix out of the swizzled buffer
    sf = torch.zeros((Np, Kp // 16), dtype=torch.uint8, device=dev)
    sf[:N, : K // 16] = SFW[_sf_swizzle_offsets(N, K, dev)]
    RB, T = Np // 16, Kp // 128
    # codes: [RB, r, T, q, 16 B] -> [RB, T, q, r, 16 B]
    RW = q.view(RB, 16, T, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    # scales: a tile has 8 groups per row, lane (r, q) owns groups 2q and 2q + 1: [RB, r, T/2, 2 tiles, q, 2] -> [RB, T/2, q, r, tile, 2]
    RSF = sf.view(RB, 16, T // 2, 2, 4, 2).permute(0, 2, 4, 1, 3, 5).contiguous().view(-1)
    assert (RW.numel(), RSF.numel()) == _repacked_bytes(N, K)
    return RW, RSF


def unrepack_w(RW: torch.Tensor, RSF: torch.Tensor, N: int, K: int):
    """The exact inverse of ``repack_w`` (pure data movement with torch ops, on RW's device): returns ``(QW, SFW)`` in the reference
    layout -- QW u8 [N, K/2], SFW u8 [sf_buffer_bytes(N, K)] with every byte outside the swizzled image of N rows zero -- so that a
    layer that keeps only the repacked weight can still export the reference's checkpoint format."""
    _need(RW, torch.uint8, "RW", 1)
    _need(RSF, torch.uint8, "RSF", 1)
    N, K = int(N), int(K)
    if N <= 0 or K <= 0 or K % 64 or (RW.numel(), RSF.numel()) != _repacked_bytes(N, K):
        raise RuntimeError(f"Value error in unrepack_w: RW / RSF do not belong to a [{N}, {K}] weight")
    dev = RW.device
    Np, Kp = (N + 15) // 16 * 16, (K + 255) // 256 * 256
    RB, T = Np // 16, Kp // 128
    # codes: [RB, T, q, r, 16 B] -> [RB, r, T, q, 16 B] = [Np, Kp/2]
    q = RW.view(RB, T, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(Np, Kp // 2)
    QW = q[:N, : K // 2].contiguous()
    # scales: [RB, T/2, q, r, tile, 2] -> [RB, r, T/2, tile, q, 2] = [Np, Kp/16], then back into the swizzled buffer
    sf = RSF.view(RB, T // 2, 4, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(Np, Kp // 16)
    SFW = torch.zeros((sf_buffer_bytes(N, K),), dtype=torch.uint8, device=dev)
    SFW[_sf_swizzle_offsets(N, K, dev)] = sf[:N, : K // 16]
    return QW, SFW


@functools.lru_cache(maxsize=None)
def rw_route(M: int, N: int, K: int) -> int:
    """Which kernels ``matmul_rw`` runs for this shape (aligned bias / residual; include/arcq.h): 1 = the repacked decode kernels
    (exactly ``matmul_repacked``), 2 = register-tiled over RW, 3 = LDS-tiled over RW (both bit-identical to ``matmul`` on the
    reference-layout weight, except the register-tiled decode shapes where ``matmul`` takes an LDS-transposing decode kernel),
    0 = unsupported."""
    return int(_lib.lib().arcq_gemm_rw_route(int(M), int(N), int(K)))


def matmul_rw(A: torch.Tensor, RW: torch.Tensor, SFA: torch.Tensor, RSF: torch.Tensor, scale, N: int, *, bias=None, residual=None,
              out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0):
    """``matmul`` for EVERY M over the weight as ``repack_w`` left it (one weight copy per layer): same arguments and result as
    ``matmul(A, B, ...)`` on the reference-layout weight, plus its row count ``N``.  Bit-identical to ``matmul_repacked`` where
    ``rw_route`` is 1 and to ``matmul`` where it is 2 or 3 -- but the decode shapes ``matmul`` serves with an LDS-transposing kernel
    (M <= 16 on very long K or very wide N), which agree up to fp32 summation order."""
    _need(A, torch.uint8, "A", 2)
    _need(SFA, torch.uint8, "SFA")
    M, K, N = A.shape[0], A.shape[1] * 2, int(N)
    _need_repacked(RW, RSF, SFA, M, N, K, "matmul_rw")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "matmul_rw")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("matmul_rw", A, RW, SFA, RSF, alpha_dev, out, bias, residual)
    L = _lib.lib()
    ws_bytes = int(L.arcq_gemm_rw_workspace_bytes(M, N, K))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=A.device) if ws_bytes else None
    with _on(A.device):
        st = L.arcq_gemm_nvfp4_rw(A.data_ptr(), RW.data_ptr(), SFA.data_ptr(), RSF.data_ptr(), out.data_ptr(), M, N, K, alpha_host,
                                  alpha_p, bias_p, residual_p, oc, ws.data_ptr() if ws_bytes else None, ws_bytes, _stream(A))
    _lib.check(st, "matmul_rw")
    return out


@functools.lru_cache(maxsize=None)
def repacked_supported(M: int, N: int, K: int) -> bool:
    """Whether ``matmul_repacked`` can run this shape: M <= 16 and the fp16 image of the activations fits LDS, or 16 < M <= 64 and
    the packed activations fit LDS (decode batches: the weight is still read once)."""
    return bool(_lib.lib().arcq_gemm_repacked_supported(int(M), int(N), int(K)))


def matmul_repacked(A: torch.Tensor, RW: torch.Tensor, SFA: torch.Tensor, RSF: torch.Tensor, scale, N: int, *, bias=None, residual=None,
                    out_dtype=torch.bfloat16, out=None, scale_host: float = 1.0, kernel: str = "auto"):
    """``matmul`` for decode shapes over a weight prepared by ``repack_w`` (same arguments otherwise, plus the row count
    ``N`` of the weight): the kernel streams the weight in MFMA operand order with no LDS transpose and no barrier in its
    K loop.  Equals ``matmul`` on the un-repacked operands up to fp32 accumulation order."""
    _need(A, torch.uint8, "A", 2)
    _need(SFA, torch.uint8, "SFA")
    M, K, N = A.shape[0], A.shape[1] * 2, int(N)
    _need_repacked(RW, RSF, SFA, M, N, K, "matmul_repacked")
    if not repacked_supported(M, N, K):
        raise RuntimeError(f"matmul_repacked: M={M}, K={K} is outside the repacked path (see repacked_supported)")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, A, "matmul_repacked")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("matmul_repacked", A, RW, SFA, RSF, alpha_dev, out, bias, residual)
    L = _lib.lib()
    # kernel="stream": the kernel body of the fused decode linears (rmsnorm_matmul_repacked, dynamic_matmul_repacked), so that
    # quantiser + this call is their bit-exact two-launch equivalent; "auto" = the fastest kernel for plain packed activations
    fn = L.arcq_gemm_nvfp4_repacked_stream if kernel == "stream" else L.arcq_gemm_nvfp4_repacked
    with _on(A.device):
        st = fn(A.data_ptr(), RW.data_ptr(), SFA.data_ptr(), RSF.data_ptr(), out.data_ptr(), M, N, K, alpha_host, alpha_p, bias_p, residual_p, oc,
                _stream(A))
    _lib.check(st, "matmul_repacked")
    return out


def matmul_silu_mul(A: torch.Tensor, B: torch.Tensor, SFA: torch.Tensor, SFB: torch.Tensor, scale, *, scale_host: float = 1.0, bias=None):
    """Extension: the gate|up GEMM with the MLP's ``act_fn(gate) * up`` (SiLU, model/qLlamaLayer.py:417) in
    its epilogue.  ``B`` is the quantised weight whose ROWS INTERLEAVE gate and up (g0, u0, g1, u1, ...).  Returns
    ``(act, absmax_slots)``: ``act`` bf16 [M, N/2] equals ``F.silu(y[:, 0::2]) * y[:, 1::2]`` of ``y = matmul(A, B, ...)``
    bit for bit; ``absmax_slots`` feeds ``reorder_quantize_x_dynamic(act, ..., absmax_slots=...)`` (one launch)."""
    _need(A, torch.uint8, "A", 2)
    _need(B, torch.uint8, "B", 2)
    _need(SFA, torch.uint8, "SFA")
    _need(SFB, torch.uint8, "SFB")
    M, N, K = A.shape[0], B.shape[0], A.shape[1] * 2
    if B.shape[1] != A.shape[1] or K % 64 or N % 8:
        raise RuntimeError(f"Value error in matmul_silu_mul: A {tuple(A.shape)} / B {tuple(B.shape)} need equal K, K % 64 == 0, N % 8 == 0")
    if SFA.numel() < _sf_used(M, K) or SFB.numel() < _sf_used(N, K):
        raise RuntimeError("Value error in matmul_silu_mul: SFA / SFB smaller than the swizzled layout of its operand")
    alpha_host, alpha_dev, alpha_p = _alpha_as_f32(scale, scale_host)
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("matmul_silu_mul", A, B, SFA, SFB, alpha_dev, bias)
    L = _lib.lib()
    act = torch.empty((M, N // 2), dtype=torch.bfloat16, device=A.device)
    slots = torch.empty((max(1, int(L.arcq_gemm_silu_mul_slots(M, N, K))),), dtype=torch.int32, device=A.device)
    with _on(A.device):
        st = L.arcq_gemm_nvfp4_silu_mul(A.data_ptr(), B.data_ptr(), SFA.data_ptr(), SFB.data_ptr(), act.data_ptr(), slots.data_ptr(), M, N, K,
                                        alpha_host, alpha_p, bias_p, _stream(A))
    _lib.check(st, "matmul_silu_mul")
    return act, slots


def matmul_rw_silu_mul(A: torch.Tensor, RW: torch.Tensor, SFA: torch.Tensor, RSF: torch.Tensor, scale, N: int, *, scale_host: float = 1.0,
                       bias=None):
    """``matmul_silu_mul`` over the weight as ``repack_w`` left it (rows interleaving gate and up), for M > 16 (prefill): returns
    ``(act, absmax_slots)`` bit-identical to ``matmul_silu_mul`` on the reference-layout weight.  Decode (M <= 16) has its own
    repacked SiLU paths (``matmul_repacked_silu_absmax``, ``rmsnorm_matmul_repacked_silu``) and raises here."""
    _need(A, torch.uint8, "A", 2)
    _need(SFA, torch.uint8, "SFA")
    M, K, N = A.shape[0], A.shape[1] * 2, int(N)
    _need_repacked(RW, RSF, SFA, M, N, K, "matmul_rw_silu_mul", n_mult=8)
    alpha_host, alpha_dev, alpha_p = _alpha_as_f32(scale, scale_host)
    bias_p = _opt(bias, torch.bfloat16, "bias", (N,))
    _same_device("matmul_rw_silu_mul", A, RW, SFA, RSF, alpha_dev, bias)
    L = _lib.lib()
    act = torch.empty((M, N // 2), dtype=torch.bfloat16, device=A.device)
    slots = torch.empty((max(1, int(L.arcq_gemm_rw_silu_mul_slots(M, N, K))),), dtype=torch.int32, device=A.device)
    with _on(A.device):
        st = L.arcq_gemm_nvfp4_rw_silu_mul(A.data_ptr(), RW.data_ptr(), SFA.data_ptr(), RSF.data_ptr(), act.data_ptr(), slots.data_ptr(), M, N, K,
                                           alpha_host, alpha_p, bias_p, _stream(A))
    _lib.check(st, "matmul_rw_silu_mul")
    return act, slots


def reorder_quantize_x_dynamic(X: torch.Tensor, reorder_index: torch.Tensor, KE: int, variant=None, absmax_slots=None):
    """Extension: ``NVFP4_reorder_quantize_x`` (model/qLlamaLayer.py:73-77) without a host sync, in ONE launch
    for decode-sized inputs (<= 256 KB) and two otherwise: returns (QX, SFX, scale) with ``scale = max|X|/2688`` a 0-dim
    fp32 device tensor and (QX, SFX) byte-identical to ``reorder_quantize_x(X / scale, reorder_index, KE)``.
    ``reorder_index=None`` (with ``absmax_slots``): X is ALREADY in reordered channel order (``rmsnorm_matmul_repacked_silu(...,
    act_scatter_index=)`` stored it so) -- same bytes as the natural-order tensor with the index, without the gather."""
    _need(X, torch.bfloat16, "X", 2)
    if absmax_slots is not None:           # max|X| already known per workgroup (matmul_silu_mul): one launch for any size
        return _quantize_dynamic("arcq_quantize_x_dyn_slots", "reorder_quantize_x_dynamic", X, X.shape[1], reorder_index, KE, variant,
                                 slots=absmax_slots)
    return _quantize_dynamic("arcq_quantize_x_dyn", "reorder_quantize_x_dynamic", X, X.shape[1], reorder_index, KE, variant)


GU_HALVES, GU_PAIRS = 0, 1


def silu_mul_quantize_x_dynamic(GU: torch.Tensor, reorder_index: torch.Tensor, KE: int, variant=None, layout: int = GU_HALVES, absmax_slots=None):
    """Extension: the MLP's ``act_fn(gate) * up`` (model/qLlamaLayer.py:417, SiLU) folded into the dynamic quantiser.
    ``GU`` is [M, 2*KQ] bf16, the output of a fused gate_up projection: ``layout=GU_HALVES`` (gate | up) or ``GU_PAIRS``
    (g0, u0, g1, u1, ...: a weight with interleaved gate/up rows, as ``matmul_silu_mul`` takes).  Returns what
    ``reorder_quantize_x_dynamic(F.silu(gate) * up, ...)`` returns, byte for byte, in two launches instead of four and
    without materialising the product."""
    _need(GU, torch.bfloat16, "GU", 2)
    if GU.shape[1] % 2:
        raise RuntimeError("Value error in silu_mul_quantize_x_dynamic: GU must hold gate and up halves of equal width")
    if layout not in (GU_HALVES, GU_PAIRS):
        raise RuntimeError("Value error in silu_mul_quantize_x_dynamic: layout must be GU_HALVES or GU_PAIRS")
    if absmax_slots is not None:           # max |silu(gate) * up| words left by matmul_repacked_silu_absmax: ONE launch
        return _quantize_dynamic("arcq_silu_mul_quantize_x_dyn_slots", "silu_mul_quantize_x_dynamic", GU, GU.shape[1] // 2, reorder_index, KE,
                                 variant, slots=absmax_slots, layout=layout)
    return _quantize_dynamic("arcq_silu_mul_quantize_x_dyn", "silu_mul_quantize_x_dynamic", GU, GU.shape[1] // 2, reorder_index, KE,
                             variant, layout=layout)


def matmul_repacked_silu_absmax(A: torch.Tensor, RW: torch.Tensor, SFA: torch.Tensor, RSF: torch.Tensor, scale, N: int, *, out=None,
                                scale_host: float = 1.0):
    """Extension for decode: ``matmul_repacked`` for a gate|up weight whose ROWS INTERLEAVE gate and up (g0, u0, g1, u1, ...).
    Returns ``(y, absmax_slots)``: ``y`` bf16 [M, N] exactly as ``matmul_repacked`` returns it, and one int32 word per block of
    16 weight rows holding max |silu(g) * u| of that block's outputs -- what ``silu_mul_quantize_x_dynamic(y, ...,
    layout=GU_PAIRS, absmax_slots=...)`` needs to quantise ``act_fn(gate) * up`` (model/qLlamaLayer.py:417) in ONE launch."""
    _need(A, torch.uint8, "A", 2)
    _need(SFA, torch.uint8, "SFA")
    M, K, N = A.shape[0], A.shape[1] * 2, int(N)
    _need_repacked(RW, RSF, SFA, M, N, K, "matmul_repacked_silu_absmax", n_mult=4)
    if not repacked_supported(M, N, K):
        raise RuntimeError(f"matmul_repacked_silu_absmax: M={M}, K={K} is outside the repacked path (see repacked_supported)")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, _ = _out(out, M, N, torch.bfloat16, A, "matmul_repacked_silu_absmax")
    _same_device("matmul_repacked_silu_absmax", A, RW, SFA, RSF, alpha_dev, out)
    slots = torch.empty(((N + 15) // 16,), dtype=torch.int32, device=A.device)
    with _on(A.device):
        st = _lib.lib().arcq_gemm_nvfp4_repacked_silu_absmax(A.data_ptr(), RW.data_ptr(), SFA.data_ptr(), RSF.data_ptr(), out.data_ptr(),
                                                    slots.data_ptr(), M, N, K, alpha_host, alpha_p, _stream(A))
    _lib.check(st, "matmul_repacked_silu_absmax")
    return out, slots


SRC_RMSNORM, SRC_DYNAMIC = 1, 2


@functools.lru_cache(maxsize=None)
def fused_supported(kind: int, M: int, N: int, KQ: int, KE: int) -> bool:
    """Whether the fused decode linear (activation quantiser as the GEMM prologue) can run this shape: M <= 16 and the LDS
    budget of one CU.  ``kind``: SRC_RMSNORM or SRC_DYNAMIC.  Callers fall back to the separate calls otherwise."""
    return bool(_lib.lib().arcq_linear_fused_supported(int(kind), int(M), int(N), int(KQ), int(KE)))


def _fused_common(who, X, reorder_index, RW, RSF, N, KE, variant):
    _need(X, torch.bfloat16, "X", 2)
    _need(reorder_index, torch.int16, "reorder_index", 1)
    M, KQ = X.shape
    KE, N = int(KE), int(N)
    if KQ % 64 or KE % 64 or KE < 0 or KE > KQ or reorder_index.numel() != KQ:
        raise RuntimeError(f"Value error in {who}: KQ={KQ}, KE={KE} or the length of reorder_index is not valid")
    _need_repacked(RW, RSF, None, M, N, KQ + KE, who)
    if variant is None:
        variant = variant_for_kq(KQ)
    return M, KQ, KE, N, int(variant)


def rmsnorm_matmul_repacked(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int, RW: torch.Tensor,
                            RSF: torch.Tensor, scale, N: int, *, bias=None, residual=None, out_dtype=torch.bfloat16, out=None,
                            scale_host: float = 1.0, variant=None):
    """Extension for decode: ``matmul_repacked(*rmsnorm_quantize_x(X, W, eps, reorder_index, KE), ...)`` in ONE launch -- the
    RMSNorm + quantiser (benchmarks/modeling_arc.py:211-228) runs as the GEMM's prologue, once per CU.  Bit-identical to the
    two calls.  ``W`` is the norm weight, ``scale`` the per-tensor weight scale (float or 0-dim device tensor)."""
    M, KQ, KE, N, variant = _fused_common("rmsnorm_matmul_repacked", X, reorder_index, RW, RSF, N, KE, variant)
    W_p = _opt(W, torch.bfloat16, "W", (KQ,))
    if not fused_supported(SRC_RMSNORM, M, N, KQ, KE):
        raise RuntimeError(f"rmsnorm_matmul_repacked: M={M}, KQ={KQ} outside the fused path (see fused_supported)")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    out, oc = _out(out, M, N, out_dtype, X, "rmsnorm_matmul_repacked")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("rmsnorm_matmul_repacked", X, W, reorder_index, RW, RSF, alpha_dev, out, bias, residual)
    with _on(X.device):
        st = _lib.lib().arcq_linear_rmsnorm_repacked(X.data_ptr(), W_p, float(eps), reorder_index.data_ptr(), RW.data_ptr(), RSF.data_ptr(),
                                                     out.data_ptr(), M, N, KQ, KE, variant, alpha_host, alpha_p, bias_p, residual_p, oc,
                                                     _stream(X))
    _lib.check(st, "rmsnorm_matmul_repacked")
    return out


_scatter_ok = {}


def _check_scatter_index(idx: torch.Tensor, n: int):
    """``act_scatter_index`` values are store columns of the kernel's epilogue: anything but a permutation of 0 .. n-1 writes out of
    bounds or leaves columns unwritten.  Checked ONCE per index tensor (one device sync, at registration time in effect), cached by
    storage address and version counter."""
    key = (idx.data_ptr(), idx.numel(), idx._version, idx.device.index)
    if _scatter_ok.get(key):
        return
    ok = idx.numel() == n and bool(torch.equal(torch.sort(idx.long()).values, torch.arange(n, device=idx.device)))
    if not ok:
        raise RuntimeError(f"agemm: act_scatter_index must be a permutation of 0 .. {n - 1}")
    if len(_scatter_ok) > 4096:
        _scatter_ok.clear()
    _scatter_ok[key] = True


def rmsnorm_matmul_repacked_silu(X: torch.Tensor, W: torch.Tensor, eps: float, reorder_index: torch.Tensor, KE: int, RW: torch.Tensor,
                                 RSF: torch.Tensor, scale, N: int, *, scale_host: float = 1.0, variant=None, bias=None,
                                 act_scatter_index=None):
    """Extension for decode, the MLP's first half in ONE launch: RMSNorm + quantise (prologue), gate|up GEMM over a repacked weight
    whose ROWS INTERLEAVE gate and up, ``act_fn(gate) * up`` (SiLU, model/qLlamaLayer.py:417) in the epilogue.  Returns
    ``(act bf16 [M, N/2], absmax_slots int32 [ceil(N/16)])``; ``act`` equals ``F.silu(y[:, 0::2]) * y[:, 1::2]`` of
    ``y = rmsnorm_matmul_repacked(...)`` bit for bit and the slots let ``dynamic_matmul_repacked`` skip its abs-max pass.
    ``act_scatter_index`` (int16 [N/2], a permutation): activation j goes to column ``act_scatter_index[j]``; with the inverse of
    the down projection's reorder_index the result is ``act[:, reorder_index]`` and the consumer quantises it with
    ``reorder_quantize_x_dynamic(act, None, KE, absmax_slots=slots)``."""
    M, KQ, KE, N, variant = _fused_common("rmsnorm_matmul_repacked_silu", X, reorder_index, RW, RSF, N, KE, variant)
    W_p = _opt(W, torch.bfloat16, "W", (KQ,))
    if N % 4 or not fused_supported(SRC_RMSNORM, M, N, KQ, KE):
        raise RuntimeError(f"rmsnorm_matmul_repacked_silu: M={M}, N={N}, KQ={KQ} outside the fused path (see fused_supported; N % 4 == 0)")
    alpha_host, alpha_dev, alpha_p = _alpha(scale, scale_host)
    bias_p, scatter_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(act_scatter_index, torch.int16, "act_scatter_index", (N // 2,))
    if act_scatter_index is not None:
        _check_scatter_index(act_scatter_index, N // 2)
    _same_device("rmsnorm_matmul_repacked_silu", X, W, reorder_index, RW, RSF, alpha_dev, bias, act_scatter_index)
    act = torch.empty((M, N // 2), dtype=torch.bfloat16, device=X.device)
    slots = torch.empty(((N + 15) // 16,), dtype=torch.int32, device=X.device)
    with _on(X.device):
        st = _lib.lib().arcq_linear_rmsnorm_silu_repacked(X.data_ptr(), W_p, float(eps), reorder_index.data_ptr(), RW.data_ptr(),
                                                          RSF.data_ptr(), act.data_ptr(), slots.data_ptr(), M, N, KQ, KE, variant, alpha_host,
                                                          alpha_p, bias_p, scatter_p, _stream(X))
    _lib.check(st, "rmsnorm_matmul_repacked_silu")
    return act, slots


def dynamic_matmul_repacked(X: torch.Tensor, reorder_index: torch.Tensor, KE: int, RW: torch.Tensor, RSF: torch.Tensor, scale_w: float, N: int, *,
                            absmax_slots=None, bias=None, residual=None, out_dtype=torch.bfloat16, out=None, variant=None):
    """Extension for decode: ``NVFP4_reorder_quantize_x`` (model/qLlamaLayer.py:73-77) + ``QLinearLayer.forward``
    (qLinearLayer.py:62-78) in ONE launch: scale = max|X|/2688 (from ``absmax_slots`` when the producing kernel left them, else
    computed from X by every workgroup), X/scale quantised in the GEMM's prologue, alpha = scale * scale_w (a host float: the
    weight's per-tensor scale).  Returns ``(y, scale)``; bit-identical to ``reorder_quantize_x_dynamic`` + ``matmul_repacked``."""
    M, KQ, KE, N, variant = _fused_common("dynamic_matmul_repacked", X, reorder_index, RW, RSF, N, KE, variant)
    if not fused_supported(SRC_DYNAMIC, M, N, KQ, KE):
        raise RuntimeError(f"dynamic_matmul_repacked: M={M}, KQ={KQ} outside the fused path (see fused_supported)")
    slots_p, nslots = _slots(absmax_slots, "dynamic_matmul_repacked")
    out, oc = _out(out, M, N, out_dtype, X, "dynamic_matmul_repacked")
    bias_p, residual_p = _opt(bias, torch.bfloat16, "bias", (N,)), _opt(residual, torch.bfloat16, "residual", (M, N))
    _same_device("dynamic_matmul_repacked", X, reorder_index, RW, RSF, absmax_slots, out, bias, residual)
    scale = torch.empty((1,), dtype=torch.float32, device=X.device)
    with _on(X.device):
        st = _lib.lib().arcq_linear_dynamic_repacked(X.data_ptr(), reorder_index.data_ptr(), RW.data_ptr(), RSF.data_ptr(), out.data_ptr(),
                                                     scale.data_ptr(), slots_p, nslots, M, N, KQ, KE, variant, float(scale_w), bias_p, residual_p, oc,
                                                     _stream(X))
    _lib.check(st, "dynamic_matmul_repacked")
    return out, scale.reshape(())


# ---- MXFP4 repacked weight (include/arcq.h "MXFP4 repacked weight"): the layout functions and the decode GEMM over it live in
# arcquant_amd/mx.py with the other MXFP4 operators that only the ctypes mirror has; they are reachable under this module's name too.
# (Resolved on first use: mx imports this module's validators.)
_FROM_MX = ("MX_REPACKED_MAX_M", "mx_repack_w", "mx_unrepack_w", "mx_repacked_supported", "mx_linear_fused_supported", "mx_matmul_repacked", "mx_matmul_rw",
            "matmul_silu_mul_rw", "matmul_silu_mul_quantize_rw", "mx_rw_route")


def __getattr__(name):
    if name in _FROM_MX:
        from . import mx
        value = globals()[name] = getattr(mx, name)
        return value
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# --- KV-cache functions of the reference module (bindings.cpp:576-581): OUT OF SCOPE.
# Present so that `from model.kv_cache import *` still imports against this module.
def _kv_stub(name):
    def f(*args, **kwargs):
        raise NotImplementedError(f"agemm.{name}: the int4 paged-KV attention is outside the ARC-NVFP4 GEMM hot path")
    f.__name__ = name
    return f


batch_decode_i4 = _kv_stub("batch_decode_i4")
init_kv_i4 = _kv_stub("init_kv_i4")
append_kv_i4 = _kv_stub("append_kv_i4")
batch_decode_f16 = _kv_stub("batch_decode_f16")
init_kv_f16 = _kv_stub("init_kv_f16")
append_kv_f16 = _kv_stub("append_kv_f16")
