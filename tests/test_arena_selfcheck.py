"""The arena helper (tests/arena.py) must be shown to bite without a GPU: ``Arena("cpu")`` is driven with pure-torch stand-in
"kernels" that are wrong on purpose, each in one of the ways the GPU arena tests exist to catch.  Host tensors and the library's
pure-integer host helpers only."""
import pytest
import torch

from tests import arena as AR
from tests.arena import In, Out, run_in_arenas

N = 61          # an odd operand size: the tail guard must start at byte 61, not at a rounded-up address


def _reach(t, before=0, after=0):
    """1-D view of ``t`` extended by up to ``before`` / ``after`` elements, as far as its storage has room -- what a kernel's stray
    address reaches.  A tight allocation has no room: there the stray access of a stand-in finds nothing, like a stray read that
    happens to meet zeros.  Returns (view, elements gained in front, elements gained behind)."""
    off = t.storage_offset()
    room = t.untyped_storage().nbytes() // t.element_size() - off - t.numel()
    b, a = min(before, off), min(after, room)
    return t.as_strided((t.numel() + b + a,), (1,), off - b), b, a


def _correct(ops):
    """out = x + sf[0] through the scratch, which it writes before it reads; sf[1] is a don't-care byte."""
    ops["ws"].copy_(ops["x"])
    ops["out"].copy_(ops["ws"] + ops["sf"][0])
    return 0


def _writes_past_output(ops):
    _correct(ops)
    ext, _, a = _reach(ops["out"], after=1)
    if a:
        ext[-1] = 1
    return 0


def _writes_before_output(ops):
    _correct(ops)
    ext, b, _ = _reach(ops["out"], before=1)
    if b:
        ext[0] = 1
    return 0


def _reads_past_input(ops):
    _correct(ops)
    ext, _, a = _reach(ops["x"], after=1)
    if a:
        ops["out"][-1] += ext[-1]
    return 0


def _reads_dont_care_scale(ops):
    _correct(ops)
    ops["out"][3] += ops["sf"][1]
    return 0


def _reads_uninitialised_scratch(ops):
    ops["out"].copy_(ops["x"] + ops["ws"] + ops["sf"][0])
    return 0


def _modifies_input(ops):
    _correct(ops)
    ops["x"][5] += 1
    return 0


def _fails(ops):
    return -1


def _drive(kernel):
    x = torch.arange(N, dtype=torch.uint8)
    sf = torch.tensor([3, 0, 0, 0], dtype=torch.uint8)
    dont_care = torch.tensor([False, True, True, True])
    run_in_arenas(kernel, {"x": In(x, align=16), "sf": In(sf, align=4, dont_care=dont_care)}, {"out": Out((N,), torch.uint8, align=16)},
                  {"ws": Out((N,), torch.uint8, align=16)}, device="cpu")


def test_a_correct_stand_in_passes():
    _drive(_correct)


@pytest.mark.parametrize("kernel,message", [
    (_writes_past_output, rf"out: 1 guard byte\(s\) on the tail side changed .*offsets {N} \.\. {N} relative"),
    (_writes_before_output, r"out: 1 guard byte\(s\) on the head side changed .*offsets -1 \.\. -1 relative"),
    (_reads_past_input, rf"out: output depends on bytes outside .*fill 0xFF 1 byte\(s\) differ.*offsets {N - 1} \.\. {N - 1} of {N}"),
    (_reads_dont_care_scale, r"out: output depends on bytes outside .*fill 0xFF 1 byte\(s\) differ.*offsets 3 \.\. 3"),
    (_reads_uninitialised_scratch, rf"out: output depends on bytes outside .*fill 0xFF {N} byte\(s\) differ.*offsets 0 \.\. {N - 1}"),
    (_modifies_input, r"x: input modified.*1 byte\(s\), offsets 5 \.\. 5"),
    (_fails, r"status -1"),
])
def test_each_wrong_stand_in_is_reported_with_operand_side_and_offset(kernel, message):
    with pytest.raises(AssertionError, match=message):
        _drive(kernel)


def test_the_arena_itself_reports_a_modified_input_and_both_guards():
    for touch, message in ((lambda v: v.__setitem__(2, 9), r"x: input modified.*offsets 2 \.\. 2 of 7"),
                           (lambda v: _reach(v, after=3)[0].__setitem__(slice(7, 10), 1), r"x: 3 guard byte\(s\) on the tail side.*offsets 7 \.\. 9"),
                           (lambda v: _reach(v, before=2)[0].__setitem__(0, 1), r"x: 1 guard byte\(s\) on the head side.*offsets -2 \.\. -2")):
        a = AR.Arena("cpu", 0x7F)
        v = a.place(torch.zeros(7, dtype=torch.uint8), align=8, name="x")
        a.check_untouched()
        touch(v)
        with pytest.raises(AssertionError, match=message):
            a.check_untouched()


def test_an_output_that_writes_its_dont_care_bytes_is_reported():
    def kernel(ops):
        ops["sfx"].fill_(1)
        return 0
    with pytest.raises(AssertionError, match=r"sfx: 2 don't-care byte\(s\) of the output written .*offsets 1 \.\. 3"):
        run_in_arenas(kernel, {}, {"sfx": Out((4,), torch.uint8, align=4, dont_care=torch.tensor([False, True, False, True]))}, device="cpu")


def test_a_nondeterministic_stand_in_fails_the_precondition_and_can_drop_only_the_value_check():
    calls = []

    def kernel(ops):
        calls.append(1)
        ops["out"].fill_(len(calls))
        return 0
    with pytest.raises(AssertionError, match="precondition: two tight runs differ in output out"):
        run_in_arenas(kernel, {}, {"out": Out((4,), torch.uint8)}, device="cpu")
    run_in_arenas(kernel, {}, {"out": Out((4,), torch.uint8)}, device="cpu", deterministic=False)
    with pytest.raises(AssertionError, match="tail side"):                # ... but the guards still hold
        run_in_arenas(_writes_past_output, {"x": In(torch.zeros(N, dtype=torch.uint8)), "sf": In(torch.zeros(4, dtype=torch.uint8), 4)},
                      {"out": Out((N,), torch.uint8)}, {"ws": Out((N,), torch.uint8)}, device="cpu", deterministic=False)


@pytest.mark.parametrize("align", [2, 4, 8, 16])
@pytest.mark.parametrize("fill", AR.FILLS)
def test_place_alignment_and_adjacency(align, fill):
    a = AR.Arena("cpu", fill)
    t = torch.arange(3 * 7, dtype=torch.int16).reshape(3, 7)                  # 42 bytes: no multiple of any alignment above 2
    v = a.place(t, align=align, name="t")
    o = a.place_out((5,), torch.bfloat16, align=align, name="o")
    assert torch.equal(v, t) and v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous()
    assert o.shape == (5,) and o.dtype == torch.bfloat16 and bool((o.view(torch.uint8) == fill).all())
    for p, view in zip(a.placements, (v, o)):
        assert view.data_ptr() % align == 0 and view.data_ptr() % (2 * align) == align      # what arcq.h promises, and no more
        assert p.buf.data_ptr() + p.head == view.data_ptr()
        assert p.head >= AR.GUARD and p.buf.numel() - p.head - p.nbytes >= AR.GUARD
        assert p.nbytes == view.numel() * view.element_size()
        # the tail guard starts at the operand's last byte + 1: the byte there is poison, and changing it is seen
        assert int(p.buf[p.head + p.nbytes]) == fill and int(p.buf[p.head - 1]) == fill
    a.check_untouched()
    a.placements[0].buf[a.placements[0].head + 42] ^= 0x55
    with pytest.raises(AssertionError, match=r"t: 1 guard byte\(s\) on the tail side.*offsets 42 \.\. 42"):
        a.check_untouched()


def test_guard_exceeds_the_largest_tile_of_the_arena_shapes():
    assert AR.GUARD > 256 * 4288 and AR.FILLS == (0x00, 0xFF, 0x7F)


@pytest.mark.parametrize("rows,K", [(1, 64), (3, 320), (130, 256), (128, 128), (300, 1088), (16, 576), (33, 2112), (257, 192), (129, 704), (520, 448),
                                    (4, 8576), (100, 384), (385, 64)])
def test_dont_care_mask_equals_the_host_helper_and_the_parity_tests_mask(rows, K):
    from arcquant_amd import _lib
    from tests.test_gpu_parity import _used_sf_mask
    L = _lib.lib()
    nbytes = int(L.arcq_sf_alloc_bytes(rows, K))
    direct = torch.zeros(nbytes, dtype=torch.bool)
    for r in range(rows):
        for p in range(K // 16):
            direct[L.arcq_sf_offset(r, p, K)] = True
    mask = AR.dont_care_mask_sf(rows, K, nbytes)
    assert mask.dtype == torch.bool and mask.shape == (nbytes,)
    assert torch.equal(~mask, direct)
    assert torch.equal(~mask, _used_sf_mask(rows, K, nbytes))
    assert int((~mask).sum()) == rows * K // 16
