"""Guarded device buffers for the memory-contract tests: a body of exactly the size a call is promised, inside ONE
allocation, between two guard regions filled with a canary.  A write that misses the body by less than the guard lands
in memory the test owns (harmless) and changes a canary byte (detected).  Plain module, imported like knn_ref.py.

    whole, body = guarded(nbytes, guard)        # uint8; body = whole[guard : guard + nbytes], 256-byte aligned base
    fill(body, "ones")                          # one of FILLS
    ... the call under test, then a device synchronise ...
    assert guards_intact(whole, guard)

Row-shaped helpers for the operator tests: guarded_rows() (an output inside canary guard rows), inside_nan() (an input as
a slice out of the middle of a NaN-filled allocation), canary_left() (was every element of the body written?).
"""
import torch

CANARY = 0xA5  # as bf16 0xA5A5 and as fp32 0xA5A5A5A5: about -2.9e-16, a value no test's arithmetic produces

# The fill patterns of a workspace body, as the byte sequence that is repeated, and what each one is under the element
# types the library keeps in a workspace (bf16, fp32, e4m3 payload, e8m0 block scales).
FILLS = {
    "zeros": bytes([0x00]),
    "ones": bytes([0xFF]),           # every bit set
    "bf16_1000": bytes([0x7A, 0x44]),  # bf16 1000.0 (0x447A), little endian
}
FILL_MEANS = {
    "zeros": {"bf16": "zero", "fp32": "zero", "e4m3": "zero", "e8m0": "tiny"},   # e8m0 0x00 = 2^-127
    "ones": {"bf16": "nan", "fp32": "nan", "e4m3": "nan", "e8m0": "nan"},
    "bf16_1000": {"bf16": "1000"},
}


def fill(body: torch.Tensor, name: str, lo: int = 0, hi: int = None) -> None:
    """Fill bytes [lo, hi) of a uint8 body with pattern `name`, phase-locked to the body's start (so a partial fill of a
    two-byte pattern continues the whole one).  lo / hi even for the two-byte pattern."""
    assert body.dtype == torch.uint8 and body.dim() == 1 and body.is_contiguous()
    pat = FILLS[name]
    hi = body.numel() if hi is None else hi
    assert 0 <= lo <= hi <= body.numel() and lo % len(pat) == 0
    n = hi - lo
    if len(pat) == 1:
        body[lo:hi] = pat[0]
        return
    p = torch.tensor(list(pat), dtype=torch.uint8, device=body.device)
    body[lo:lo + n - n % len(pat)].view(-1, len(pat)).copy_(p.expand(n // len(pat), len(pat)))
    if n % len(pat):
        body[hi - 1] = pat[0]


def guarded(nbytes: int, guard: int, device="cuda"):
    """(whole, body): one uint8 allocation of guard + nbytes + guard bytes, all canary; body is its middle, numel() ==
    nbytes exactly, base address a multiple of 256."""
    assert nbytes >= 0 and guard > 0 and guard % 256 == 0
    whole = torch.full((guard + nbytes + guard,), CANARY, dtype=torch.uint8, device=device)
    body = whole[guard:guard + nbytes]
    assert body.numel() == nbytes
    assert whole.device.type == "cpu" or body.data_ptr() % 256 == 0, "allocator base not 256-byte aligned"
    return whole, body


def guard_damage(whole: torch.Tensor, guard: int):
    """Offsets (relative to the body's start; negative = in front) of the overwritten guard bytes nearest the body, as
    (first damaged byte in front or None, first damaged byte behind or None)."""
    w = whole.view(torch.uint8).reshape(-1)
    n = w.numel() - 2 * guard
    front = torch.nonzero(w[:guard] != CANARY).reshape(-1)
    back = torch.nonzero(w[guard + n:] != CANARY).reshape(-1)
    return (int(front.max()) - guard if front.numel() else None, n + int(back.min()) if back.numel() else None)


def guards_intact(whole: torch.Tensor, guard: int) -> bool:
    """True while every byte of both guards still holds the canary."""
    return guard_damage(whole, guard) == (None, None)


def canary_value(dtype: torch.dtype) -> torch.Tensor:
    """One element of `dtype` whose bytes are all CANARY."""
    return torch.full((dtype.itemsize,), CANARY, dtype=torch.uint8).view(dtype)[0]


def guarded_rows(rows: int, cols: int, dtype: torch.dtype, guard_rows: int = 8, device="cuda"):
    """(whole, body): a canary-filled [guard_rows + rows + guard_rows, cols] tensor and its middle `rows` rows."""
    whole = torch.full(((rows + 2 * guard_rows) * cols * dtype.itemsize,), CANARY, dtype=torch.uint8, device=device)
    whole = whole.view(dtype).view(rows + 2 * guard_rows, cols)
    return whole, whole[guard_rows:guard_rows + rows]


def rows_intact(whole: torch.Tensor, guard_rows: int) -> bool:
    b = whole.view(torch.uint8)
    return bool((b[:guard_rows] == CANARY).all()) and bool((b[whole.shape[0] - guard_rows:] == CANARY).all())


def canary_left(body: torch.Tensor) -> int:
    """Number of elements of the body whose bytes are all still the canary (0: every element was written)."""
    b = body.contiguous().view(torch.uint8).reshape(-1, body.dtype.itemsize)
    return int((b == CANARY).all(dim=1).sum())


def inside_nan(t: torch.Tensor, pad: int = 8, device="cuda") -> torch.Tensor:
    """A copy of t on `device` that is a slice out of the middle of a larger NaN-filled allocation: `pad` rows on each
    side for a matrix, `pad` elements for a vector (pad * row bytes a multiple of 16 keeps the alignment of a fresh
    allocation).  The slice is contiguous."""
    assert t.dim() in (1, 2) and t.is_floating_point()
    lead = t.shape[0]
    big = torch.full((lead + 2 * pad,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype, device=device)
    view = big[pad:pad + lead]
    view.copy_(t)
    assert view.is_contiguous()
    return view
