"""Guard bands: the only out-of-bounds check a device store can get without a GPU sanitizer.

`guarded(shape, dtype, device)` returns a tensor that is a view into the middle of one larger allocation.  In front of it and behind it
lies a band of a fixed bit pattern; `check` (or the `watch` context manager around a call) asserts afterwards that both bands still hold
that pattern, and that every tensor registered as an input (`frozen`) has the bits it had before the call.  torch only, CPU and GPU
tensors alike; host arrays of a C ABI are CPU tensors whose `data_ptr()` is passed on.

The pattern is the 32-bit word PATTERN = 0x7FC5A3B1, stored little-endian over the whole allocation from its first byte:
  * read as float32 it is a quiet NaN with the payload 0x45A3B1: a kernel that reads a band by mistake poisons its result, and a
    float comparison of the band with itself fails (NaN != NaN), which is why every comparison here is made on integers (the bytes);
  * each of its four bytes (0xB1, 0xA3, 0xC5, 0x7F) is odd, so a band read as a uint8 mask is "sampled" everywhere and never 0 or 1;
  * its bytes are pairwise different, so a store of a shifted copy of the pattern is seen too.
Read as float64, two words make 0x7FC5A3B17FC5A3B1 = 1.2e307 (finite): float64 / complex128 bands are compared as bytes like the rest.

Layout of one allocation (all figures in bytes, E = the dtype's element size):

    | leading band: B | skew: 16 (pattern as well) | the view: numel * E | trailing band: B | pad to a multiple of 4 |

B = band * E rounded up to a multiple of 64, band = max(4096 elements, one H x W plane of the view) when the view is at least 2-D and 4096
elements otherwise.  The width is a condition, not a measurement: an overrun by a whole 2048-pixel chunk, a whole row block or a whole
plane lands inside the band, i.e. inside memory the test owns.  The view starts B + skew bytes into the allocation; torch allocations
are at least 64-byte aligned, so with skew = 16 the view's pointer is 16 mod 32: 16-byte aligned and no more than that (`guarded`
raises if the allocator did not deliver that).  The skew bytes belong to the leading band and are checked with it.

A failure names the tensor, the side ("leading" / "trailing" band, or "frozen input"), the first touched offset in ELEMENTS RELATIVE TO
THE VIEW (negative in the leading band, >= numel in the trailing one) and the count of touched elements."""
from __future__ import annotations

import contextlib
from typing import Dict, Mapping, Optional

import torch

PATTERN = 0x7FC5A3B1
PATTERN_BYTES = (0xB1, 0xA3, 0xC5, 0x7F)          # little-endian
MIN_BAND = 4096                                    # elements
SKEW = 16                                          # bytes

_REAL_OF = {torch.complex64: torch.float32, torch.complex128: torch.float64}


class GuardBandError(AssertionError):
    pass


class _Info:
    """Where a guarded view lies inside its allocation (bytes)."""
    __slots__ = ("raw", "start", "nbytes", "itemsize", "name")

    def __init__(self, raw, start, nbytes, itemsize, name):
        self.raw, self.start, self.nbytes, self.itemsize, self.name = raw, start, nbytes, itemsize, name


def itemsize(dtype: torch.dtype) -> int:
    return torch.empty((), dtype=dtype).element_size()


def band_elements(shape) -> int:
    """max(4096 elements, one H x W plane) for a view of at least two dimensions, 4096 elements otherwise."""
    shape = tuple(int(v) for v in shape)
    return max(MIN_BAND, shape[-2] * shape[-1]) if len(shape) >= 2 else MIN_BAND


def pattern_bytes(n: int, phase: int, device) -> torch.Tensor:
    """uint8 [n]: the bytes an untouched allocation holds from byte offset `phase` on."""
    word = torch.tensor(PATTERN_BYTES, dtype=torch.uint8, device=device)
    return word.repeat((n + phase % 4 + 3) // 4 + 1)[phase % 4: phase % 4 + n]


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    """The bits of a contiguous tensor as a flat uint8 view (complex dtypes through view_as_real)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.reshape(-1).view(torch.uint8)


def guarded(shape, dtype: torch.dtype, device, fill=None, band: Optional[int] = None, skew: int = SKEW, name: Optional[str] = None) -> torch.Tensor:
    """A contiguous tensor of `shape` / `dtype` inside one larger allocation, a band of PATTERN on either side (see the module docstring).
    fill: None leaves the view holding the pattern too; a tensor (any device) of the same number of elements is copied in; a number fills it.
    band: elements per side (default `band_elements(shape)`).  The returned tensor carries its bookkeeping as `._guard`."""
    shape = tuple(int(v) for v in shape)
    device = torch.device(device)
    size = itemsize(dtype)
    numel = 1
    for v in shape:
        numel *= v
    band = band_elements(shape) if band is None else int(band)
    bbytes = (band * size + 63) // 64 * 64
    start, nbytes = bbytes + skew, numel * size
    total = (start + nbytes + bbytes + 3) // 4 * 4
    raw = torch.full((total // 4,), PATTERN, dtype=torch.int32, device=device).view(torch.uint8)
    flat = raw[start:start + nbytes]
    real = _REAL_OF.get(dtype)
    if real is not None:                                   # complex: a view of the real buffer
        view = torch.view_as_complex(flat.view(real).view(numel, 2)).view(shape)
    else:
        view = flat.view(dtype).view(shape)
    if view.data_ptr() != raw.data_ptr() + start or view.data_ptr() % 32 != skew % 32:
        raise RuntimeError(f"guarded: the allocator gave {raw.data_ptr():#x}; the view at +{start} is not {skew} mod 32")
    if fill is not None:
        if torch.is_tensor(fill):
            view.copy_(fill.reshape(shape).to(dtype))
        else:
            view.fill_(fill)
    view._guard = _Info(raw, start, nbytes, size, name)
    return view


def _touched(got: torch.Tensor, want: torch.Tensor, first_byte: int, size: int):
    """(first touched element, touched elements) of a byte range that starts `first_byte` bytes from the view's first byte, or None."""
    if torch.equal(got, want):
        return None
    idx = torch.nonzero(got != want).reshape(-1) + first_byte
    elems = torch.unique(torch.div(idx, size, rounding_mode="floor"))
    return int(elems.min()), int(elems.numel())


def band_report(t: torch.Tensor, name: Optional[str] = None):
    """Failure lines for the two bands of one guarded tensor (empty when both hold the pattern)."""
    g = t._guard
    name = name or g.name or "tensor"
    end = g.start + g.nbytes
    out = []
    for side, lo, hi in (("leading", 0, g.start), ("trailing", end, g.raw.numel())):
        hit = _touched(g.raw[lo:hi], pattern_bytes(hi - lo, lo, g.raw.device), lo - g.start, g.itemsize)
        if hit:
            out.append(f"{name}: {side} band touched: first at offset {hit[0]} (elements, relative to the view), {hit[1]} elements touched")
    return out


def snapshot(t: torch.Tensor) -> torch.Tensor:
    """The bits of a tensor, to compare with after a call (`frozen`)."""
    return as_bytes(t).clone()


def frozen_report(t: torch.Tensor, before: torch.Tensor, name: str):
    hit = _touched(as_bytes(t), before, 0, t.element_size())
    return [f"{name}: frozen input changed: first at offset {hit[0]} (elements, relative to the view), {hit[1]} elements touched"] if hit else []


def check(tensors: Mapping[str, Optional[torch.Tensor]], frozen: Optional[Mapping[str, torch.Tensor]] = None) -> None:
    """Assert that both bands of every tensor in `tensors` (name -> guarded tensor; None entries are skipped) hold the pattern and that every
    tensor named in `frozen` (name -> `snapshot` taken before the call) still has those bits.  Synchronises the GPU first."""
    if torch.cuda.is_available() and any(t is not None and t.is_cuda for t in tensors.values()):
        torch.cuda.synchronize()
    lines = []
    for name, t in tensors.items():
        if t is None:
            continue
        lines += band_report(t, name)
        if frozen and name in frozen:
            lines += frozen_report(t, frozen[name], name)
    if lines:
        raise GuardBandError("\n".join(lines))


@contextlib.contextmanager
def watch(outputs: Optional[Dict[str, Optional[torch.Tensor]]] = None, inputs: Optional[Dict[str, Optional[torch.Tensor]]] = None):
    """`with watch(outputs={...}, inputs={...}): call(...)`: on leaving the block without an exception, `check` every tensor; the
    `inputs` are frozen at their bits on entry."""
    outputs = {k: v for k, v in (outputs or {}).items() if v is not None}
    inputs = {k: v for k, v in (inputs or {}).items() if v is not None}
    before = {k: snapshot(v) for k, v in inputs.items()}
    yield
    check({**outputs, **inputs}, before)
