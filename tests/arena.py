"""Guarded arenas for C-ABI calls: a kernel's result must not depend on bytes outside its operands, and it must not write any.

Every operand of a call is copied into the middle of a larger ``uint8`` allocation whose other bytes -- and every byte of the
operand the contract calls "don't care" -- hold one loud poison byte.  ``run_in_arenas`` runs the call on plain tight allocations
first, then once per poison in arenas, and demands that

  (a) every declared output byte equals the tight run's (compared as integers, so NaN payloads count),
  (b) no guard byte and no input byte changed (``Arena.check_untouched``),
  (c) the call returned status 0.

No numeric tolerance is involved and no reference is needed: the comparison is with the same kernel on other surroundings.

The two constants of this module:

``GUARD``  bytes of poison in front of and behind every operand.  It is a condition, not a measurement: a load or store whose
           address is wrong by up to one tile of the operand must still land in memory the test owns (and so show up as a changed
           result or a changed guard instead of a fault).  The largest single-tile footprint of the shapes the arena tests use is
           256 rows x 4288 bytes (a 256-row tile of a packed operand with K = 8576), about 1.05 MiB, hence 2 MiB.

``FILLS``  the poison bytes.  0xFF is NaN as bf16, fp32, ue4m3 and E8M0, the e2m1 code pair (-6, -6) and the index -1; 0x7F is
           E8M0 1.0, ue4m3 NaN, bf16 3.4e38 and the codes (6, -6); 0x00 is the value ``torch.empty`` neighbours usually have,
           i.e. the surroundings under which a stray read goes unnoticed -- it anchors the other two.  Between them a read that
           reaches arithmetic is loud in every operand type.

Nothing else is a tuned number.  An allocation is ``GUARD + 2 * align + nbytes + GUARD`` bytes: the ``2 * align`` of slack is derived
from the operand's own alignment, not chosen -- it is what lets the operand start at an address that is a multiple of ``align`` and of
nothing larger (at most ``2 * align - 1`` bytes after the head guard's first ``GUARD`` bytes), so a kernel that assumes more than arcq.h
promises meets exactly what it promises.  Both guards therefore hold at least ``GUARD`` bytes, and the tail guard still starts at the
operand's last byte + 1.
"""
from __future__ import annotations

import torch

GUARD = 2 << 20
FILLS = (0x00, 0xFF, 0x7F)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    """Flat uint8 view of a contiguous tensor (shares its memory)."""
    return t.reshape(-1).view(torch.uint8)


def _span(diff: torch.Tensor):
    """(count, first, last) of the True entries of a 1-D bool tensor."""
    idx = diff.nonzero().reshape(-1)
    return int(idx.numel()), int(idx[0]), int(idx[-1])


class In:
    """An input operand: a contiguous tensor, the alignment arcq.h requires of it and (optionally) a bool mask over its bytes that
    marks the ones the contract calls don't care (they are replaced by the poison in the arena copy)."""

    def __init__(self, tensor: torch.Tensor, align: int = 16, dont_care: torch.Tensor | None = None):
        assert tensor.is_contiguous()
        self.tensor, self.align, self.dont_care = tensor, align, dont_care


class Out:
    """An output (or scratch) operand: shape, dtype, alignment; ``dont_care`` marks declared bytes the call must leave alone (they
    must still hold the poison afterwards and are not compared); ``init`` is the content of an in-place operand (a residual that
    aliases D, a cache that is appended to) -- without it the declared bytes start as poison.  ``poison`` marks bytes of ``init`` whose
    value the call must not use: the arena copy holds the poison there (the tight run keeps ``init``'s own values); it defaults to
    ``dont_care`` and is larger where the call overwrites a byte it must not read."""

    def __init__(self, shape, dtype, align: int = 16, dont_care: torch.Tensor | None = None, init: torch.Tensor | None = None,
                 poison: torch.Tensor | None = None):
        self.shape, self.dtype, self.align, self.dont_care, self.init = tuple(shape), dtype, align, dont_care, init
        self.poison = poison if poison is not None else (dont_care if init is not None else None)


class _Placement:
    __slots__ = ("name", "kind", "buf", "head", "nbytes", "view", "want")


class Arena:
    """Places operands between two guards of ``GUARD`` poisoned bytes each."""

    def __init__(self, device, fill: int = 0xFF):
        self.device, self.fill = torch.device(device), int(fill)
        self.placements: list[_Placement] = []
        self._ref = torch.empty((0,), dtype=torch.uint8, device=self.device)

    def _filled(self, n: int) -> torch.Tensor:
        """``n`` poison bytes on the device, to compare a guard with."""
        if self._ref.numel() < n:
            self._ref = torch.full((n,), self.fill, dtype=torch.uint8, device=self.device)
        return self._ref[:n]

    def _alloc(self, nbytes: int, align: int, name, kind) -> _Placement:
        assert align >= 1 and (align & (align - 1)) == 0
        # the operand starts GUARD (+ at most 2 * align - 1) bytes into the allocation, at an address that is a multiple of `align` and
        # of nothing larger: a kernel that assumes more than arcq.h promises meets an operand that has exactly what it promises
        buf = torch.full((GUARD + 2 * align + nbytes + GUARD,), self.fill, dtype=torch.uint8, device=self.device)
        head = GUARD + (align - (buf.data_ptr() + GUARD) % (2 * align)) % (2 * align)
        p = _Placement()
        p.name, p.kind, p.buf, p.head, p.nbytes, p.want = name or f"operand{len(self.placements)}", kind, buf, head, nbytes, None
        self.placements.append(p)
        return p

    def _view(self, p: _Placement, shape, dtype) -> torch.Tensor:
        v = p.buf[p.head:p.head + p.nbytes].view(dtype).view(shape)
        assert v.is_contiguous() and v.data_ptr() == p.buf.data_ptr() + p.head
        p.view = v
        return v

    def place(self, t: torch.Tensor, align: int = 16, name=None, dont_care=None, kind: str = "in") -> torch.Tensor:
        """Copy the contiguous tensor ``t`` into a fresh arena; returns a contiguous view of the same shape and dtype whose
        ``data_ptr()`` is ``align``-aligned and whose last byte is followed at once by the tail guard."""
        assert t.is_contiguous()
        p = self._alloc(t.numel() * t.element_size(), align, name, kind)
        v = self._view(p, t.shape, t.dtype)
        v.copy_(t)
        if dont_care is not None:
            _bytes(v)[dont_care.to(self.device)] = self.fill
        if kind == "in":
            p.want = _bytes(v).clone()
        return v

    def place_out(self, shape, dtype, align: int = 16, name=None, kind: str = "out") -> torch.Tensor:
        """The same for an output: the declared region holds the poison too."""
        n = 1
        for s in shape:
            n *= int(s)
        p = self._alloc(n * torch.empty((), dtype=dtype).element_size(), align, name, kind)
        return self._view(p, tuple(shape), dtype)

    def check_untouched(self):
        """Every guard byte still equals the poison and every input's payload equals what was placed (compared on the device)."""
        for p in self.placements:
            tail0 = p.head + p.nbytes
            for side, region, base in (("head", p.buf[:p.head], -p.head), ("tail", p.buf[tail0:], p.nbytes)):
                if not torch.equal(region, self._filled(region.numel())):
                    n, first, last = _span(region != self.fill)
                    raise AssertionError(f"{p.name}: {n} guard byte(s) on the {side} side changed (fill 0x{self.fill:02X}): offsets "
                                         f"{base + first} .. {base + last} relative to the operand of {p.nbytes} bytes")
            if p.want is not None and not torch.equal(_bytes(p.view), p.want):
                n, first, last = _span(_bytes(p.view) != p.want)
                raise AssertionError(f"{p.name}: input modified (fill 0x{self.fill:02X}): {n} byte(s), offsets {first} .. {last} "
                                     f"of {p.nbytes}")


def sf_used_mask(rows: int, K: int, nbytes: int, sf_offset) -> torch.Tensor:
    """Bool mask over an NVFP4 scale buffer of ``nbytes``: True at ``sf_offset(r, p, K)`` for r < rows, p < K/16.  ``sf_offset`` is the
    library's host helper arcq_sf_offset.  The layout of include/arcq.h is a sum of a row term and a position term, so the helper is
    asked for every row (at p = 0) and for every position (at r = 0): rows + K/16 calls instead of rows * K/16.  That the sum holds
    is not taken on trust: the last position of every row and the last row of every position are asked for as well and must agree.
    tests/test_arena_selfcheck.py checks the result against a call per (r, p)."""
    P = K // 16
    base = sf_offset(0, 0, K)
    row = torch.tensor([sf_offset(r, 0, K) for r in range(rows)], dtype=torch.int64)
    pos = torch.tensor([sf_offset(0, p, K) for p in range(P)], dtype=torch.int64)
    off = row.unsqueeze(1) + pos.unsqueeze(0) - base
    last_p = torch.tensor([sf_offset(r, P - 1, K) for r in range(rows)], dtype=torch.int64)
    last_r = torch.tensor([sf_offset(rows - 1, p, K) for p in range(P)], dtype=torch.int64)
    assert torch.equal(off[:, P - 1], last_p) and torch.equal(off[rows - 1], last_r), "arcq_sf_offset is not row term + position term"
    used = torch.zeros(nbytes, dtype=torch.bool)
    used[off.reshape(-1)] = True
    return used


def dont_care_mask_sf(rows: int, K: int, nbytes: int, sf_offset=None) -> torch.Tensor:
    """Bool mask of the NVFP4 scale bytes that are NOT ``arcq_sf_offset(r, p, K)`` for any r < rows, p < K/16: arcq.h calls only the
    offsets of rows < M written or meaningful."""
    if sf_offset is not None:
        return ~sf_used_mask(rows, K, nbytes, sf_offset)
    key = (rows, K, nbytes)
    if key not in _MASKS:               # (a case asks for the same mask once per run; callers do not modify it)
        from arcquant_amd import _lib
        _MASKS[key] = ~sf_used_mask(rows, K, nbytes, _lib.lib().arcq_sf_offset)
    return _MASKS[key]


_MASKS: dict = {}


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def _status_text(st):
    try:
        from arcquant_amd import _lib
        return f"status {st}: {_lib.lib().arcq_last_error().decode('utf-8', 'replace')}"
    except Exception:      # (a stand-in kernel on a machine without the library)
        return f"status {st}"


def _tight_run(call, inputs, outputs, scratch, device):
    ops = {k: s.tensor for k, s in inputs.items()}
    for name, s in list(outputs.items()) + list(scratch.items()):
        ops[name] = s.init.clone() if s.init is not None else torch.zeros(s.shape, dtype=s.dtype, device=device)
    before = {k: _bytes(s.tensor).clone() for k, s in inputs.items()}
    st = call(ops)
    _sync(device)
    assert st == 0, f"tight call: {_status_text(st)}"
    for k, s in inputs.items():
        if not torch.equal(_bytes(s.tensor), before[k]):
            n, first, last = _span(_bytes(s.tensor) != before[k])
            raise AssertionError(f"{k}: input modified by the tight call: {n} byte(s), offsets {first} .. {last} of {before[k].numel()}")
    return {k: _bytes(ops[k]).clone() for k in outputs}


def run_in_arenas(call, inputs: dict, outputs: dict, scratch: dict | None = None, device="cuda:0", deterministic: bool = True,
                  fills=FILLS):
    """``call(ops) -> status`` receives a dict name -> tensor holding every key of ``inputs`` (``In``), ``outputs`` and ``scratch``
    (``Out``).  Runs it twice on tight allocations (the two runs must agree byte for byte: the precondition of comparing at all),
    then once per poison with every operand in an arena, and asserts (a), (b), (c) of the module docstring.  Scratch is placed and
    poisoned like an output but its contents are not compared.  ``deterministic=False`` (an entry point whose two tight runs differ:
    a finding, say so where it is used) drops (a) only.  Returns the tight run's output bytes."""
    scratch = scratch or {}
    assert not (set(inputs) & set(outputs)) and not (set(scratch) & (set(inputs) | set(outputs)))
    want = _tight_run(call, inputs, outputs, scratch, device)
    again = _tight_run(call, inputs, outputs, scratch, device)
    if deterministic:
        for k in outputs:
            assert torch.equal(want[k], again[k]), f"precondition: two tight runs differ in output {k}"
    for fill in fills:
        arena = Arena(device, fill)
        ops = {k: arena.place(s.tensor, s.align, name=k, dont_care=s.dont_care) for k, s in inputs.items()}
        for kind, group in (("out", outputs), ("scratch", scratch)):
            for k, s in group.items():
                if s.init is not None:
                    ops[k] = arena.place(s.init, s.align, name=k, dont_care=s.poison, kind=kind)
                else:
                    ops[k] = arena.place_out(s.shape, s.dtype, s.align, name=k, kind=kind)
        st = call(ops)
        _sync(device)
        assert st == 0, f"arena call (fill 0x{fill:02X}): {_status_text(st)}"
        arena.check_untouched()
        for k, s in outputs.items():
            got = _bytes(ops[k])
            if s.dont_care is not None:
                dc = s.dont_care.to(got.device)
                if not bool((got[dc] == fill).all()):
                    n, first, last = _span(dc & (got != fill))
                    raise AssertionError(f"{k}: {n} don't-care byte(s) of the output written (fill 0x{fill:02X}): offsets {first} .. {last}")
                diff = (got != want[k]) & ~dc
            else:
                diff = got != want[k]
            if deterministic and bool(diff.any()):
                n, first, last = _span(diff)
                raise AssertionError(f"{k}: output depends on bytes outside the operands' contract: with fill 0x{fill:02X} {n} byte(s) differ "
                                     f"from the tight call, offsets {first} .. {last} of {got.numel()}")
    return want
