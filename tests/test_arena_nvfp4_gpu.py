"""Arena tests of the NVFP4 C-ABI (``-m gpu``): every entry point of include/arcq.h once per kernel configuration, each operand inside
a poisoned arena (tests/arena.py).  Every comparison is bit-exact against the same call on tight allocations; no value needs a
reference.  Operands are random e2m1 codes with finite ue4m3 scale bytes (as test_gemm_fuzz_random_shapes_against_fp64_matmul) or
random bf16 activations; the scale bytes no row < M owns are poison.

The dispatch map (which shape reaches which kernel configuration) starts from the one stated next to GEMM_CASES,
test_repacked_weight_gemm_equals_the_reference_layout_gemm and FUSED_CASES in tests/test_gpu_parity.py and in tests/test_gemm_rw_gpu.py,
checked against the heuristics themselves (gemm_regtile_cfg, tile_choice / tile_split, choose_split / decode_split,
rowblock_choose_slices, mid_kind): several comments there predate the register-tiled kernel, which now takes most small M > 16 shapes
the tile GEMM used to see.  Where the library has a predicate for a route (arcq_gemm_rw_route, arcq_gemm_repacked_supported,
arcq_linear_fused_supported, arcq_gemm_workspace_bytes > 0 for split-K) the case asserts it, so a heuristic change cannot silently
empty the coverage.
"""
import pytest
import torch

from tests.arena import In, Out, dont_care_mask_sf, run_in_arenas

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32, U8, I32, I16 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int16


def _L():
    from arcquant_amd import _lib
    return _lib.lib()


def _ag():
    from arcquant_amd import agemm
    return agemm


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _packed(rows, K, g):
    """Random codes and finite scale bytes (ue4m3 subnormals up to 15) in a buffer of the reference's size; -> In(codes), In(scales)."""
    q = torch.randint(0, 256, (rows, K // 2), generator=g, device=DEV, dtype=U8)
    nbytes = int(_L().arcq_sf_alloc_bytes(rows, K))
    sf = torch.randint(1, 0x58, (nbytes,), generator=g, device=DEV, dtype=U8)
    return In(q, 16), In(sf, 4, dont_care=dont_care_mask_sf(rows, K, nbytes))


def _bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(BF16)


def _epilogue_inputs(M, N, g, residual=True, align=8):
    """bias, residual and the device half of alpha, the scalar in an arena of its own.  align = 8: the views the repacked decode kernels
    require (arcq.h: anything less skips route 1); align = 2: a bf16 view with no alignment beyond its element size, which is all arcq.h
    promises arcq_gemm_nvfp4 and routes 2 / 3 of arcq_gemm_nvfp4_rw."""
    def view(shape):
        # the tight run must take the route the arena run takes, so for align = 2 its tensor is a view one element into its storage too
        n = 1
        for d in shape:
            n *= d
        t = _bf16((n + 1,), g)[1:].view(shape) if align == 2 else _bf16(shape, g)
        assert t.is_contiguous() and (align != 2 or t.data_ptr() % 4 == 2)
        return In(t, align)
    ins = {"bias": view((N,)), "alpha_dev": In(torch.tensor([0.5], dtype=F32, device=DEV), 4)}
    if residual:
        ins["residual"] = view((M, N))
    return ins


# ------------------------------------------------------------------------------------------------ arcq_gemm_nvfp4 and its repacked twins
def _run_gemm(entry, M, N, K, out_dtype=BF16, epi=False, alias=False, seed=0, epi_align=8):
    """entry: "nvfp4" (arcq_gemm_nvfp4), "rw" (arcq_gemm_nvfp4_rw), "repacked" / "stream" (arcq_gemm_nvfp4_repacked[_stream])."""
    L, g = _L(), _gen(seed + M + N + K)
    a, sfa = _packed(M, K, g)
    b, sfb = _packed(N, K, g)
    ins = {"A": a, "SFA": sfa}
    if entry == "nvfp4":
        ins["B"], ins["SFB"] = b, sfb
        ws_bytes = int(L.arcq_gemm_workspace_bytes(M, N, K))
    else:
        RW, RSF = _ag().repack_w(b.tensor, sfb.tensor)              # exactly arcq_repacked_{w,sf}_bytes, every byte meaningful
        assert (RW.numel(), RSF.numel()) == (int(L.arcq_repacked_w_bytes(N, K)), int(L.arcq_repacked_sf_bytes(N, K)))
        ins["B"], ins["SFB"] = In(RW, 16), In(RSF, 4)
        ws_bytes = int(L.arcq_gemm_rw_workspace_bytes(M, N, K)) if entry == "rw" else 0
    if epi or alias:
        ins.update(_epilogue_inputs(M, N, g, residual=not alias, align=epi_align))
    init = _bf16((M, N), g) if alias else None                        # the residual aliases D: the arena holds it, D is the same view
    outs = {"D": Out((M, N), out_dtype, 16, init=init)}
    scratch = {"ws": Out((ws_bytes,), U8, 16)} if ws_bytes else {}
    oc = 0 if out_dtype is BF16 else 1
    fn = {"nvfp4": L.arcq_gemm_nvfp4, "rw": L.arcq_gemm_nvfp4_rw, "repacked": L.arcq_gemm_nvfp4_repacked,
          "stream": L.arcq_gemm_nvfp4_repacked_stream}[entry]

    def call(o):
        res = o["D"] if alias else o.get("residual")
        args = [_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["D"]), M, N, K, 0.01, _p(o.get("alpha_dev")), _p(o.get("bias")), _p(res), oc]
        if entry in ("nvfp4", "rw"):
            args += [_p(o.get("ws")), ws_bytes]
        return fn(*args, _stream())

    run_in_arenas(call, ins, outs, scratch, device=DEV)
    return ws_bytes


GEMM_REGTILE = [
    # M, N, K, split-K workspace expected -- launcher and configuration.  gemm_regtile.hip serves M <= 16 (16 x 16 decode tiles) and every
    # 16 < M whose smallest one-round tile gives 96 .. 256 workgroups (gemm_regtile_cfg; the shapes are those named next to GEMM_CASES):
    (3, 100, 320, False),          # gemm_regtile.hip 16 x 16 decode tiles; N % 16 != 0, 1 tail atom
    (16, 50, 192, False),          # ... N % 4 != 0 (scalar stores), 3 tail atoms
    (4, 1024, 2112, False),        # ... 8 quad-steps over the 8 waves + 1 tail atom
    (24, 3104, 320, False),        # gemm_regtile.hip 32 x 16 tiles, 1 quad-step + 1 tail atom, 24 live rows
    (300, 264, 320, False),        # ... ragged M and N over 10 x 17 tiles (the tile GEMM no longer sees this shape)
    (64, 2112, 2176, False),       # gemm_regtile.hip 32 x 32 tiles, 2 tail atoms
    (32, 8200, 320, False),        # gemm_regtile.hip 32 x 64 tiles
    (100, 2110, 384, False),       # gemm_regtile.hip 64 x 32 tiles, ragged M and N, N % 4 != 0 (scalar stores), 2 tail atoms
    (200, 2500, 448, False),       # gemm_regtile.hip 64 x 64 tiles (droppable requests), 3 tail atoms, N % 16 = 4
    (300, 4100, 640, False),       # gemm_regtile.hip 128 x 64 tiles, 2 tail atoms
    (192, 10000, 320, False),      # gemm_regtile.hip 64 x 128 tiles
    (256, 10752, 320, False),      # gemm_regtile.hip 128 x 128 tiles
    (20, 16448, 320, False),       # gemm_regtile.hip 32 x 64 tiles over two rounds
]
GEMM_OTHER = [
    # the LDS-transposing decode kernels: M <= 8 with K > 8448 or N > 16384
    (4, 384, 8576, False),         # gemm_skinny.hip (16-row tiles), k_last clamp of the partial tail slab
    (4, 384, 32704, True),         # gemm_skinny.hip split-K x2 (needs 16 slabs of 2048: only reachable at this K), partial tail slab
    (2, 5120, 8512, False),        # gemm_decode.hip (32-row tiles), long K, partial tail slab
    (8, 16400, 320, False),        # gemm_decode.hip, N > 16384, ragged N (N % 16 != 0): scale bytes of rows >= N masked
    (5, 16402, 192, False),        # gemm_decode.hip, N % 4 != 0, a single partial slab
    (4, 5120, 15424, True),        # gemm_decode.hip split-K x2 (160 <= tiles < 192 and 16 slabs: only reachable here), partial tail slab
    # gemm_tile.hip (tile_choice): 32 x 256 for M <= 32, 64 x 256 for M <= 64, then 128 x 256, 128 x 128 or 256 x 256 by tile count
    (17, 136, 320, False),         # 32-row tile, first M on the tile kernel, one pass over K
    (24, 260, 2048, True),         # 32-row tile, split-K x4, ragged 256-row weight tiles
    (33, 516, 2112, True),         # 64-row tile (33 live rows), split-K x4
    (40, 130, 2048, False),        # 64-row tile, N % 4 != 0: the split is refused, one pass over K, scalar stores
    (130, 200, 256, False),        # 128 x 256 tile, ragged M and N, no K tail
    (300, 130, 320, False),        # 128 x 256 tile, N % 4 != 0: scalar stores
    (130, 264, 2112, True),        # 128 x 256 tile, split-K x4, ragged M and N
    (1100, 2056, 8192, True),      # 128 x 128 tile (reachable only past the register-tiled kernel's M N K limit), split-K x2, ragged M and N
    (300, 24600, 320, False),      # 256 x 256 tile (needs >= 192 tiles): interior tiles with 16-byte vector stores, both ragged edges
    (300, 24602, 320, False),      # 256 x 256 tile, N % 4 != 0: scalar stores
]

GEMM_NVFP4 = GEMM_REGTILE + GEMM_OTHER
_REGTILE_ROWS = set(c[:3] for c in GEMM_REGTILE)


@pytest.mark.parametrize("M,N,K,split", GEMM_NVFP4)
def test_gemm_nvfp4(M, N, K, split):
    """arcq_gemm_nvfp4, bf16 and fp32, once plain and once with bias + residual + alpha_dev; the split-K workspace is exactly
    arcq_gemm_workspace_bytes, poisoned, and asked for where the case expects the split (every split ends in gemm_splitk_finish,
    gemm_skinny.hip's splitk_finish_kernel, which reads the partial planes back)."""
    L = _L()
    if M > 16 and L.arcq_gemm_rw_route(M, N, K) != 1:
        # arcq_gemm_nvfp4 has no route predicate of its own, but arcq.h defines routes 2 / 3 of arcq_gemm_nvfp4_rw as the register-tiled /
        # LDS-tiled kernel "in the configuration arcq_gemm_nvfp4 would use" (route 1, the repacked decode kernels, hides it for M <= 128
        # on small weights): where it shows, it must be the kernel this table names
        assert L.arcq_gemm_rw_route(M, N, K) == (2 if (M, N, K) in _REGTILE_ROWS else 3), (M, N, K)
    for out_dtype, epi in ((BF16, False), (F32, True), (BF16, True)):
        ws = _run_gemm("nvfp4", M, N, K, out_dtype=out_dtype, epi=epi)
        assert (ws > 0) == split, (M, N, K, ws)


@pytest.mark.parametrize("entry,M,N,K", [
    ("nvfp4", 3, 100, 320),        # gemm_regtile.hip 16 x 16 decode tiles
    ("nvfp4", 200, 2500, 448),     # gemm_regtile.hip 64 x 64 tiles
    ("nvfp4", 130, 264, 2112),     # gemm_tile.hip 128 x 256 tile with split-K: the residual is added by splitk_finish_kernel
    ("nvfp4", 300, 24600, 320),    # gemm_tile.hip 256 x 256 tile, interior tiles and ragged edges
    ("nvfp4", 2, 5120, 8512),      # gemm_decode.hip
    ("rw", 129, 1000, 576),        # route 2
    ("rw", 300, 130, 704),         # route 3
    ("rw", 4, 100, 576),           # a route-1 shape: the misaligned views send it to route 2 (arcq.h)
])
def test_gemm_bias_and_residual_views_with_two_byte_alignment(entry, M, N, K):
    """arcq.h promises arcq_gemm_nvfp4 no alignment of bias / residual beyond bf16's own, and arcq_gemm_nvfp4_rw that such views take
    route 2 or 3: the epilogues meet views at an address that is 2 modulo 4 (element loads instead of 8-byte ones)."""
    for out_dtype in (BF16, F32):
        _run_gemm(entry, M, N, K, out_dtype=out_dtype, epi=True, epi_align=2)


REPACKED = [
    # M, N, K -- gemm_rowblock.hip (M <= 16), the kernel over the fp16 activation image in LDS.  Waves per row block
    # (rowblock_choose_slices over ceil(K / 256) tile pairs) and image units per thread (ceil(M * pairs * 8 / 512) -> 1, 2, 4, 8):
    (3, 1000, 64),                 # 1 wave, a single half-filled tile pair (K % 256 = 64)
    (1, 512, 320),                 # 2 waves, 1 unit per thread
    (4, 100, 320),                 # ... ragged N (N % 16 = 4)
    (5, 5120, 448),                # 2 waves, K % 256 = 192
    (8, 778, 640),                 # 2 waves owning 2 + 1 pairs, K % 256 = 128, N % 4 != 0
    (16, 272, 1088),               # 4 waves owning 2 + 1 + 1 + 1 pairs, 2 units per thread
    (4, 1000, 2112),               # 8 waves, 9 pairs
    (16, 100, 2240),               # 8 waves, 4 units per thread
    (16, 256, 4160),               # 8 waves, 8 units per thread, a 139 KB image
    # gemm_rowblock.hip's no-image kernel (8 Mi <= N * K <= 24 Mi elements, only reachable there)
    (4, 3584, 3648),               # 8 waves
    (2, 52000, 320),               # 1 wave per row block: too many row blocks to split
    # gemm_rowmid.hip (16 < M <= 128), no activations in LDS (N * K <= 32 Mi): 2, 3, 4, 6 and 8 token tiles
    (17, 128, 320), (33, 516, 2048), (50, 778, 576), (81, 1000, 64), (96, 520, 1152), (120, 264, 1088),
    # gemm_rowmid.hip with the packed activations resident in LDS: only reachable for N * K > 32 Mi elements
    (33, 16008, 2112),
]


@pytest.mark.parametrize("M,N,K", REPACKED)
def test_gemm_repacked(M, N, K):
    """arcq_gemm_nvfp4_repacked (gemm_rowblock.hip / gemm_rowmid.hip) and, for M <= 16, arcq_gemm_nvfp4_repacked_stream
    (gemm_stream.hip) over RW / RSF of exactly arcq_repacked_{w,sf}_bytes."""
    assert _L().arcq_gemm_repacked_supported(M, N, K)
    _run_gemm("repacked", M, N, K, out_dtype=BF16, epi=True)
    _run_gemm("repacked", M, N, K, out_dtype=F32)
    if M <= 16:
        _run_gemm("stream", M, N, K, out_dtype=BF16, epi=True)
        _run_gemm("stream", M, N, K, out_dtype=F32)


@pytest.mark.parametrize("M,N,K,route,split", [
    (4, 100, 576, 1, False),       # route 1: gemm_rowblock.hip through arcq_gemm_nvfp4_rw
    (40, 300, 576, 1, False),      # route 1: gemm_rowmid.hip
    (129, 1000, 576, 2, False),    # route 2: gemm_regtile.hip over RW (32 x 32 tiles), K % 256 = 64, ragged N
    (300, 264, 320, 2, False),     # route 2: 32 x 16 tiles, ragged M and N
    (8, 264, 10304, 2, False),     # route 2, a G' shape (arcq_gemm_nvfp4 takes gemm_skinny.hip): the 16 x 16 configuration over RW
    (300, 130, 704, 3, False),     # route 3: gemm_tile_rw.hip 128 x 256 tiles, N % 4 != 0, K % 256 = 192
    (130, 264, 2112, 3, True),     # route 3 with split-K x4, the workspace poisoned
    (300, 24600, 320, 3, False),   # route 3: 256 x 256 tiles, interior tiles plus both ragged edges
])
def test_gemm_rw(M, N, K, route, split):
    """arcq_gemm_nvfp4_rw on routes 1, 2 and 3 (asserted through arcq_gemm_rw_route), route 3 also with split-K."""
    L = _L()
    assert L.arcq_gemm_rw_route(M, N, K) == route
    ws = _run_gemm("rw", M, N, K, out_dtype=BF16, epi=True)
    _run_gemm("rw", M, N, K, out_dtype=F32)
    if route == 3:
        assert ws == L.arcq_gemm_workspace_bytes(M, N, K) and (ws > 0) == split


@pytest.mark.parametrize("entry,M,N,K", [("nvfp4", 4, 100, 320), ("nvfp4", 300, 264, 320), ("nvfp4", 33, 516, 2112), ("nvfp4", 300, 130, 320),
                                         ("nvfp4", 2, 5120, 8512), ("rw", 129, 1000, 576), ("rw", 130, 264, 2112), ("repacked", 4, 100, 320),
                                         ("repacked", 40, 516, 576)])
def test_gemm_residual_aliasing_d(entry, M, N, K):
    """`x + linear(x')` written in place: the arena holds the residual, D is the same view (gemm_regtile.hip decode and 32 x 16 tiles,
    gemm_tile.hip with and without split-K, gemm_decode.hip, both tiled kernels over RW, gemm_rowblock.hip, gemm_rowmid.hip)."""
    _run_gemm(entry, M, N, K, alias=True)


# ------------------------------------------------------------------------------------------------ SiLU-epilogue GEMMs
def _run_silu(entry, M, N, K, bias=False, seed=3):
    """entry: "nvfp4" (arcq_gemm_nvfp4_silu_mul), "rw" (arcq_gemm_nvfp4_rw_silu_mul), "repacked" (arcq_gemm_nvfp4_repacked_silu_absmax)."""
    L, g = _L(), _gen(seed + M + N + K)
    a, sfa = _packed(M, K, g)
    b, sfb = _packed(N, K, g)
    ins = {"A": a, "SFA": sfa, "alpha_dev": In(torch.tensor([0.5], dtype=F32, device=DEV), 4)}
    if entry == "nvfp4":
        ins["B"], ins["SFB"] = b, sfb
        nslots, fn, width = int(L.arcq_gemm_silu_mul_slots(M, N, K)), L.arcq_gemm_nvfp4_silu_mul, N // 2
    else:
        RW, RSF = _ag().repack_w(b.tensor, sfb.tensor)
        ins["B"], ins["SFB"] = In(RW, 16), In(RSF, 4)
        if entry == "rw":
            nslots, fn, width = int(L.arcq_gemm_rw_silu_mul_slots(M, N, K)), L.arcq_gemm_nvfp4_rw_silu_mul, N // 2
        else:
            nslots, fn, width = (N + 15) // 16, L.arcq_gemm_nvfp4_repacked_silu_absmax, N
    assert nslots > 0
    if bias:
        ins["bias"] = In(_bf16((N,), g), 8)
    outs = {"ACT": Out((M, width), BF16, 16), "slots": Out((nslots,), I32, 4)}

    def call(o):
        args = [_p(o["A"]), _p(o["B"]), _p(o["SFA"]), _p(o["SFB"]), _p(o["ACT"]), _p(o["slots"]), M, N, K, 0.004, _p(o["alpha_dev"])]
        if entry != "repacked":
            args.append(_p(o.get("bias")))
        return fn(*args, _stream())

    run_in_arenas(call, ins, outs, device=DEV)


@pytest.mark.parametrize("entry,M,N,K,bias", [
    ("nvfp4", 3, 272, 320, False),         # gemm_decode.hip with the SiLU epilogue (every M <= 16), ragged N % 256
    ("nvfp4", 4, 5128, 576, False),        # ... several weight tiles, partial tail slab
    ("nvfp4", 24, 264, 320, True),         # gemm_tile.hip 32 x 256 tile (the SiLU epilogue never takes gemm_regtile.hip)
    ("nvfp4", 40, 520, 576, True),         # gemm_tile.hip 64 x 256 tile
    ("nvfp4", 100, 392, 320, True),        # gemm_tile.hip 128 x 256 tile
    ("nvfp4", 300, 5640, 320, True),       # gemm_tile.hip 128 x 128 tile (more than 64 tiles of 128 x 256)
    ("nvfp4", 300, 24600, 320, False),     # gemm_tile.hip 256 x 256 tile, interior tiles plus ragged edges
    ("rw", 17, 264, 576, True),            # gemm_tile_rw.hip with the SiLU epilogue, first prefill M, 32 x 256 tile
    ("rw", 100, 392, 320, False),          # ... 128 x 256 tile
    ("rw", 300, 5640, 320, True),          # ... 128 x 128 tile
    ("repacked", 1, 36, 320, False),       # gemm_rowblock.hip SiLU abs-max, N % 16 = 4
    ("repacked", 3, 272, 320, False),
    ("repacked", 16, 2000, 1088, False),
    ("repacked", 4, 5120, 576, False),
    ("repacked", 4, 5120, 2112, False),    # gemm_rowblock.hip's no-image kernel with the SiLU abs-max
])
def test_gemm_silu_epilogues(entry, M, N, K, bias):
    """arcq_gemm_nvfp4_silu_mul, arcq_gemm_nvfp4_rw_silu_mul, arcq_gemm_nvfp4_repacked_silu_absmax: ACT and absmax_slots as outputs of
    exactly the words the slot helpers promise."""
    if entry == "repacked":
        assert _L().arcq_gemm_repacked_supported(M, N, K)
    _run_silu(entry, M, N, K, bias=bias)


# ------------------------------------------------------------------------------------------------ fused decode linears
def _magnitude_slots(x, chunk=997):
    """abs-max words as a producing kernel leaves them: bf16 magnitude bits, any split of the tensor works."""
    mag = x.reshape(-1).view(I16).to(I32) & 0x7FFF
    return torch.stack([c.max() for c in mag.split(chunk)]).to(I32).contiguous()


def _fused_weight(N, K, g):
    b, sfb = _packed(N, K, g)
    RW, RSF = _ag().repack_w(b.tensor, sfb.tensor)
    return In(RW, 16), In(RSF, 4)


@pytest.mark.parametrize("M,N,KQ,KE", [(1, 272, 2048, 64), (3, 1000, 3584, 64), (16, 100, 2048, 0), (3, 48, 3584, 0)])
def test_fused_rmsnorm_linears(M, N, KQ, KE):
    """arcq_linear_rmsnorm_repacked (bf16 plain, fp32 and bf16 with bias + residual + alpha_dev) and arcq_linear_rmsnorm_silu_repacked
    (with and without act_scatter_index): gemm_stream.hip with the RMSNorm quantiser as its prologue."""
    L, g, K = _L(), _gen(M + N + KQ), KQ + KE
    assert L.arcq_linear_fused_supported(1, M, N, KQ, KE)
    variant = int(L.arcq_variant_for_kq(KQ))
    rw, rsf = _fused_weight(N, K, g)
    base = {"X": In(_bf16((M, KQ), g, 3.0), 16), "Wn": In(_bf16((KQ,), g) * 0.1 + 1, 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16),
            "RW": rw, "RSF": rsf}
    for out_dtype, epi in ((BF16, False), (F32, True), (BF16, True)):
        ins = dict(base)
        if epi:
            ins.update(_epilogue_inputs(M, N, g))
        oc = 0 if out_dtype is BF16 else 1

        def call(o):
            return L.arcq_linear_rmsnorm_repacked(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["RW"]), _p(o["RSF"]), _p(o["D"]), M, N, KQ, KE, variant,
                                                  0.01, _p(o.get("alpha_dev")), _p(o.get("bias")), _p(o.get("residual")), oc, _stream())
        run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16)}, device=DEV)
    for scatter in (False, True):
        ins = dict(base)
        ins["bias"] = In(_bf16((N,), g), 8)
        if scatter:
            ins["scatter"] = In(torch.randperm(N // 2, generator=g, device=DEV).to(I16), 16)

        def call(o):
            return L.arcq_linear_rmsnorm_silu_repacked(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["RW"]), _p(o["RSF"]), _p(o["ACT"]), _p(o["slots"]),
                                                       M, N, KQ, KE, variant, 0.004, None, _p(o["bias"]), _p(o.get("scatter")), _stream())
        run_in_arenas(call, ins, {"ACT": Out((M, N // 2), BF16, 16), "slots": Out(((N + 15) // 16,), I32, 4)}, device=DEV)


@pytest.mark.parametrize("M,N,KQ,KE", [(1, 272, 2048, 64), (3, 1000, 3584, 64), (16, 100, 2048, 0), (3, 50, 3584, 0), (4, 48, 18944, 64)])
def test_fused_dynamic_linear(M, N, KQ, KE):
    """arcq_linear_dynamic_repacked (gemm_stream.hip with the dynamic quantiser as its prologue) with and without absmax_slots, scale_out a
    4-byte output in an arena of its own; the last case gathers its 18944-wide rows from global memory (the 152 KB image leaves no LDS
    to stage them)."""
    L, g, K = _L(), _gen(7 + M + N + KQ), KQ + KE
    assert L.arcq_linear_fused_supported(2, M, N, KQ, KE)
    variant = int(L.arcq_variant_for_kq(KQ))
    rw, rsf = _fused_weight(N, K, g)
    x = _bf16((M, KQ), g, 3.0)
    base = {"X": In(x, 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16), "RW": rw, "RSF": rsf}
    for out_dtype, epi, slots in ((BF16, False, False), (F32, True, True), (BF16, True, False)):
        ins = dict(base)
        if epi:
            ins["bias"], ins["residual"] = In(_bf16((N,), g), 8 if N % 4 == 0 else 2), In(_bf16((M, N), g), 8 if N % 4 == 0 else 2)
        if slots:
            ins["slots"] = In(_magnitude_slots(x), 4)
        nslots = ins["slots"].tensor.numel() if slots else 0
        oc = 0 if out_dtype is BF16 else 1

        def call(o):
            return L.arcq_linear_dynamic_repacked(_p(o["X"]), _p(o["idx"]), _p(o["RW"]), _p(o["RSF"]), _p(o["D"]), _p(o["scale_out"]), _p(o.get("slots")), nslots,
                                                  M, N, KQ, KE, variant, 0.01, _p(o.get("bias")), _p(o.get("residual")), oc, _stream())
        run_in_arenas(call, ins, {"D": Out((M, N), out_dtype, 16), "scale_out": Out((1,), F32, 4)}, device=DEV)


# ------------------------------------------------------------------------------------------------ quantisers
def _sfx(rows, K):
    nbytes = int(_L().arcq_sf_alloc_bytes(rows, K))
    return Out((nbytes,), U8, 4, dont_care=dont_care_mask_sf(rows, K, nbytes))       # only the offsets of rows < M may be written


@pytest.mark.parametrize("rows,KQ,KE,variant", [(1, 256, 64, 0), (3, 320, 64, 1), (130, 256, 0, 0), (33, 2048, 2048, 0), (5, 3584, 64, 1), (129, 1088, 128, 1),
                                                 (2, 28672, 64, 1)])
def test_static_quantisers(rows, KQ, KE, variant):
    """arcq_quantize_x and arcq_quantize_w (quantize.hip), G16 and G32, one and several 128-row scale tiles, the 56 KB "down" row."""
    L, g, K = _L(), _gen(rows + KQ), KQ + KE
    ins = {"X": In(_bf16((rows, KQ), g, 300.0), 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}
    for fn in (L.arcq_quantize_x, L.arcq_quantize_w):
        def call(o):
            return fn(_p(o["X"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), rows, KQ, KE, variant, _stream())
        run_in_arenas(call, ins, {"Q": Out((rows, K // 2), U8, 8), "SF": _sfx(rows, K)}, device=DEV)


@pytest.mark.parametrize("rows,KQ,KE,variant", [(1, 2048, 64, 0), (3, 3584, 64, 1), (130, 2048, 0, 0), (5, 8192, 128, 0), (3, 3584, 64, 0)])
def test_rmsnorm_quantiser(rows, KQ, KE, variant):
    """arcq_rmsnorm_quantize_x, G16 and G32."""
    L, g, K = _L(), _gen(rows + KQ + 1), KQ + KE
    ins = {"X": In(_bf16((rows, KQ), g, 3.0), 16), "Wn": In(_bf16((KQ,), g) * 0.1 + 1, 16), "idx": In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)}

    def call(o):
        return L.arcq_rmsnorm_quantize_x(_p(o["X"]), _p(o["Wn"]), 1e-6, _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), rows, KQ, KE, variant, _stream())
    run_in_arenas(call, ins, {"Q": Out((rows, K // 2), U8, 8), "SF": _sfx(rows, K)}, device=DEV)


@pytest.mark.parametrize("n", [8, 1000, 4096 * 33 + 5])
def test_absmax_scale(n):
    """arcq_absmax_scale: one block, a ragged tail, many blocks."""
    L = _L()
    x = _bf16((n,), _gen(n), 37.0)

    def call(o):
        return L.arcq_absmax_scale(_p(o["X"]), n, _p(o["scale_out"]), _stream())
    run_in_arenas(call, {"X": In(x, 16)}, {"scale_out": Out((1,), F32, 4)}, device=DEV)


DYN_SHAPES = [
    # M, KQ, KE, variant
    (4, 2048, 64, 0),          # 16 KB: the single-launch path, `state` untouched
    (3, 3584, 64, 1),
    (80, 2048, 64, 0),         # 320 KB > 256 KB: the abs-max pass leaves its words in `state`
    (130, 1088, 128, 1),       # ... two 128-row scale tiles
]


@pytest.mark.parametrize("M,KQ,KE,variant", DYN_SHAPES)
def test_dynamic_quantisers(M, KQ, KE, variant):
    """arcq_quantize_x_dyn and arcq_silu_mul_quantize_x_dyn (both layouts): `state` is ARCQ_DYN_STATE_BYTES of poisoned scratch."""
    L, g, K = _L(), _gen(M + KQ + 2), KQ + KE
    idx = In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)
    outs = lambda: {"Q": Out((M, K // 2), U8, 8), "SF": _sfx(M, K), "scale_out": Out((1,), F32, 4)}      # noqa: E731
    scratch = lambda: {"state": Out((1024,), U8, 16)}                                                          # noqa: E731

    def call(o):
        return L.arcq_quantize_x_dyn(_p(o["X"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), _p(o["scale_out"]), _p(o["state"]), M, KQ, KE, variant, _stream())
    run_in_arenas(call, {"X": In(_bf16((M, KQ), g, 3.0), 16), "idx": idx}, outs(), scratch(), device=DEV)
    gu = In(_bf16((M, 2 * KQ), g, 3.0), 16)
    for layout in (0, 1):
        def call(o):
            return L.arcq_silu_mul_quantize_x_dyn(_p(o["GU"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), _p(o["scale_out"]), _p(o["state"]), M, KQ, KE, variant,
                                                  layout, _stream())
        run_in_arenas(call, {"GU": gu, "idx": idx}, outs(), scratch(), device=DEV)


@pytest.mark.parametrize("M,KQ,KE,variant", DYN_SHAPES)
def test_slot_fed_quantisers(M, KQ, KE, variant):
    """arcq_quantize_x_dyn_slots (with reorder_index and with NULL: X already in reordered order) and
    arcq_silu_mul_quantize_x_dyn_slots (both layouts), the abs-max words an input of exactly nslots words."""
    import torch.nn.functional as F
    L, g, K = _L(), _gen(M + KQ + 3), KQ + KE
    idx = In(torch.randperm(KQ, generator=g, device=DEV).to(I16), 16)
    outs = lambda: {"Q": Out((M, K // 2), U8, 8), "SF": _sfx(M, K), "scale_out": Out((1,), F32, 4)}      # noqa: E731
    x = _bf16((M, KQ), g, 3.0)
    slots = _magnitude_slots(x)
    for with_idx in (True, False):
        def call(o):
            return L.arcq_quantize_x_dyn_slots(_p(o["X"]), _p(o.get("idx")), _p(o["Q"]), _p(o["SF"]), _p(o["scale_out"]), _p(o["slots"]), slots.numel(),
                                               M, KQ, KE, variant, _stream())
        ins = {"X": In(x, 16), "slots": In(slots, 4)}
        if with_idx:
            ins["idx"] = idx
        run_in_arenas(call, ins, outs(), device=DEV)
    gu = _bf16((M, 2 * KQ), g, 3.0)
    for layout in (0, 1):
        gate, up = (gu[:, :KQ], gu[:, KQ:]) if layout == 0 else (gu[:, 0::2], gu[:, 1::2])
        gslots = _magnitude_slots((F.silu(gate) * up).contiguous())

        def call(o):
            return L.arcq_silu_mul_quantize_x_dyn_slots(_p(o["GU"]), _p(o["idx"]), _p(o["Q"]), _p(o["SF"]), _p(o["scale_out"]), _p(o["slots"]), gslots.numel(),
                                                        M, KQ, KE, variant, layout, _stream())
        run_in_arenas(call, {"GU": In(gu, 16), "idx": idx, "slots": In(gslots, 4)}, outs(), device=DEV)


# ------------------------------------------------------------------------------------------------ include/arcq_harness.h
@pytest.mark.parametrize("variant", ["default", "sliced"])
@pytest.mark.parametrize("pos,first", [(0, 0), (17, 0), (17, 9), (599, 0), (599, 300), (599, 590)])
def test_harness_attn_decode_window(pos, first, variant):
    """arcq_harness_attn_decode_window (harness_attn.hip: attn_decode_fused, one launch, no scratch) and
    arcq_harness_attn_decode_window_sliced (attn_decode_partial + attn_decode_combine: one, two and three live slices of the three that
    Tmax = 600 lays out, the partial records going through the poisoned workspace).  The reference is the tight run over the finite
    random cache.  In the arenas every cache position outside [first, pos) holds the poison -- so does `pos`, which the call writes from
    qkv and must not read -- and the output and the live and the written cache rows must equal the reference's while every other cache
    byte keeps the poison: only row `pos` of each (b, h) changes."""
    L, g = _L(), _gen(pos)
    B, H, Tmax, D = 2, 3, 600, 128
    qkv = _bf16((B, 3 * H * D), g)
    kc, vc = _bf16((B, H, Tmax, D), g), _bf16((B, H, Tmax, D), g)
    ws_bytes = int(L.arcq_harness_attn_workspace_bytes(B, H, Tmax))
    poison = torch.ones((B, H, Tmax, D * 2), dtype=torch.bool, device=DEV)            # per byte of the bf16 caches
    poison[:, :, first:pos] = False
    untouched = poison.clone()
    untouched[:, :, pos] = False                                                      # row `pos` is poisoned going in and compared coming out
    poison, untouched = poison.reshape(-1), untouched.reshape(-1)
    fn = L.arcq_harness_attn_decode_window if variant == "default" else L.arcq_harness_attn_decode_window_sliced

    def call(o):
        return fn(_p(o["qkv"]), _p(o["kcache"]), _p(o["vcache"]), _p(o["out"]), _p(o["ws"]), B, H, Tmax, pos, first, _stream())

    outs = {"out": Out((B, H * D), BF16, 16), "kcache": Out(kc.shape, BF16, 16, dont_care=untouched, init=kc, poison=poison),
            "vcache": Out(vc.shape, BF16, 16, dont_care=untouched, init=vc, poison=poison)}
    want = run_in_arenas(call, {"qkv": In(qkv, 16)}, outs, {"ws": Out((ws_bytes,), U8, 16)}, device=DEV)
    hidden = H * D
    for name, t, part in (("kcache", kc, 1), ("vcache", vc, 2)):                      # the reference itself: row `pos` appended, nothing else
        after = want[name].view(BF16).reshape(B, H, Tmax, D)
        expect = t.clone()
        expect[:, :, pos] = qkv[:, part * hidden:(part + 1) * hidden].reshape(B, H, D)
        assert torch.equal(after.view(I16), expect.view(I16)), name


def test_harness_rmsnorm_with_a_strided_input():
    """arcq_harness_rmsnorm over rows of H values with row stride ldx > H: the gaps between the rows are poison."""
    L, g = _L(), _gen(11)
    rows, H, ldx = 5, 264, 512
    x = _bf16((rows, ldx), g)
    gaps = torch.zeros((rows, ldx * 2), dtype=torch.bool, device=DEV)
    gaps[:, H * 2:] = True

    def call(o):
        return L.arcq_harness_rmsnorm(_p(o["X"]), ldx, _p(o["W"]), _p(o["out"]), rows, H, 1e-6, _stream())
    run_in_arenas(call, {"X": In(x, 16, dont_care=gaps.reshape(-1)), "W": In(_bf16((H,), g) * 0.1 + 1, 16)}, {"out": Out((rows, H), BF16, 16)}, device=DEV)
