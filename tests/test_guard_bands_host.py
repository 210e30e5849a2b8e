"""The guard-band harness (tests/guard_bands.py) on CPU tensors: every way a store can leave its tensor is reported with the right
side, offset and count, for every dtype the GPU tests guard; an untouched view passes; a changed input is reported; the pointer is
16 mod 32; the pattern is what the harness documents and no comparison is a float comparison."""
import os
import struct
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as gb  # noqa: E402

DTYPES = [torch.float32, torch.complex64, torch.uint8, torch.float64, torch.complex128, torch.int32, torch.int64]
SHAPES = [(3, 1, 16, 16), (2, 80, 80), (65,), (3,)]        # 2-D+ (band = max(4096, plane)), 1-D; 3 uint8 = a view that ends off a word


def _ids(vals):
    return [str(v).replace("torch.", "") for v in vals]


def _poke(t, elem, byte=0, xor=0xFF):
    """Flip bits of one byte of the element `elem` (relative to the view, may lie in a band) in the allocation of a guarded tensor."""
    g = t._guard
    g.raw[g.start + elem * g.itemsize + byte] ^= xor


def _band(t):
    g = t._guard
    return (g.start - gb.SKEW) // g.itemsize, (g.raw.numel() - g.start - g.nbytes) // g.itemsize     # whole elements in front / behind


def test_pattern_is_a_nan_with_a_payload_and_odd_bytes():
    (f,) = struct.unpack("<f", struct.pack("<I", gb.PATTERN))
    assert f != f                                                               # NaN
    assert (gb.PATTERN >> 23) & 0xFF == 0xFF and gb.PATTERN & 0x3FFFFF != 0     # payload beyond the quiet bit
    assert tuple(struct.pack("<I", gb.PATTERN)) == gb.PATTERN_BYTES
    assert all(b & 1 for b in gb.PATTERN_BYTES) and len(set(gb.PATTERN_BYTES)) == 4
    t = gb.guarded((4, 4), torch.float32, "cpu")
    assert bool(torch.isnan(t).all())                                           # an unfilled view holds the pattern too
    assert bool((t.view(torch.int32) == gb.PATTERN).all())
    m = gb.guarded((16, 16), torch.uint8, "cpu")
    assert bool((m & 1).all())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_layout_band_width_and_alignment(dtype, shape):
    t = gb.guarded(shape, dtype, "cpu", fill=1)
    g = t._guard
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 32 == 16                                              # 16-byte aligned and no more
    assert t.data_ptr() == g.raw.data_ptr() + g.start
    want = max(4096, shape[-2] * shape[-1]) if len(shape) >= 2 else 4096
    assert gb.band_elements(shape) == want
    front, back = _band(t)
    assert front >= want and back >= want and front < want + 64 and back < want + 64
    assert g.start == front * g.itemsize + 16
    gb.check({"t": t})


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_stores_outside_the_view_are_reported_with_side_offset_and_count(dtype, shape):
    n = 1
    for v in shape:
        n *= v
    size = gb.itemsize(dtype)
    probe = gb.guarded(shape, dtype, "cpu", fill=0)
    g = probe._guard
    first = -(g.start // size)                              # the far edge of the leading band (the skew bytes count with it)
    last = n + (g.raw.numel() - g.start - g.nbytes) // size - 1
    assert first <= -4096 and last >= n + 4095
    for elem, side in ((-1, "leading"), (n, "trailing"), (first, "leading"), (last, "trailing")):
        t = gb.guarded(shape, dtype, "cpu", fill=0, name="buf")
        _poke(t, elem, byte=size - 1)
        with pytest.raises(gb.GuardBandError) as ei:
            gb.check({"out": t})
        msg = str(ei.value)
        assert msg == f"out: {side} band touched: first at offset {elem} (elements, relative to the view), 1 elements touched", msg
    # a run of elements on both sides: first offset and count per side, one line each
    t = gb.guarded(shape, dtype, "cpu", fill=0)
    for elem in (-5, -4, -2, n + 1, n + 2, n + 7):
        _poke(t, elem)
    with pytest.raises(gb.GuardBandError) as ei:
        gb.check({"out": t})
    lines = str(ei.value).split("\n")
    assert lines == ["out: leading band touched: first at offset -5 (elements, relative to the view), 3 elements touched",
                     f"out: trailing band touched: first at offset {n + 1} (elements, relative to the view), 3 elements touched"], lines


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_a_single_flipped_bit_is_reported(dtype):
    size = gb.itemsize(dtype)
    for elem, byte, bit in ((-1, 0, 0), (48, size - 1, 7), (-4096, size // 2, 3), (48 + 4095, 0, 6)):
        t = gb.guarded((3, 16), dtype, "cpu", fill=0)
        _poke(t, elem, byte=byte, xor=1 << bit)
        with pytest.raises(gb.GuardBandError, match=rf"first at offset {elem} \(elements, relative to the view\), 1 elements touched"):
            gb.check({"t": t})


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_an_untouched_view_passes_whatever_is_written_inside_it(dtype):
    t = gb.guarded((2, 1, 16, 32), dtype, "cpu")
    gb.check({"t": t})
    t.fill_(3)
    t[1, 0, 15, 31] = 5
    t[0, 0, 0, 0] = 7
    with gb.watch(outputs={"t": t}):
        t.mul_(2)
    assert bool((t.reshape(-1)[1:-1] == 6).all()) and t[0, 0, 0, 0] == 14 and t[1, 0, 15, 31] == 10


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_a_frozen_input_that_changed_is_reported(dtype):
    src = torch.arange(2 * 16 * 16).reshape(2, 16, 16) % 7
    t = gb.guarded((2, 16, 16), dtype, "cpu", fill=src)
    assert torch.equal(t, src.to(dtype))
    with gb.watch(inputs={"x": t}):
        pass                                                # unchanged: passes
    with pytest.raises(gb.GuardBandError) as ei:
        with gb.watch(inputs={"x": t}):
            t[1, 2, 3] += 1
            t[1, 15, 15] += 1
    assert str(ei.value) == ("x: frozen input changed: first at offset 291 (elements, relative to the view), 2 elements touched")
    # an output may change; the same tensor as an output passes
    with gb.watch(outputs={"x": t}):
        t[0, 0, 0] += 1


def test_comparisons_are_made_on_integers_not_floats():
    """A band is NaN as float32: a float comparison would call an untouched band touched (NaN != NaN), and a frozen input that holds
    NaN would be called changed.  Both pass; a NaN whose payload changed, or -0 for +0, is reported."""
    t = gb.guarded((16, 16), torch.float32, "cpu", fill=float("nan"))
    g = t._guard
    band = g.raw[:g.start].view(torch.float32)
    assert not torch.equal(band, band.clone()) or not bool((band == band).any())     # what a float comparison would say
    with gb.watch(inputs={"t": t}):
        pass
    # the pattern survives clone (as bits)
    c = g.raw.clone()
    assert torch.equal(c, g.raw) and torch.equal(c[:g.start], gb.pattern_bytes(g.start, 0, "cpu"))
    assert bool((c[:g.start - g.start % 4].view(torch.int32) == gb.PATTERN).all())
    # another NaN in the band: equal as floats to nothing, different as bits
    band[-1] = float("nan")
    with pytest.raises(gb.GuardBandError, match="leading band touched: first at offset -1 "):
        gb.check({"t": t})
    z = gb.guarded((4,), torch.float32, "cpu", fill=0.0)
    with pytest.raises(gb.GuardBandError, match="frozen input changed: first at offset 2 "):
        with gb.watch(inputs={"z": z}):
            z[2] = -0.0                                     # equal as floats


def test_fill_from_a_tensor_and_none_entries():
    src = torch.view_as_complex(torch.arange(2 * 3 * 4 * 2, dtype=torch.float32).reshape(2, 3, 4, 2))
    t = gb.guarded((2, 3, 4), torch.complex64, "cpu", fill=src)
    assert torch.equal(t, src)
    gb.check({"t": t, "absent": None})
    with gb.watch(outputs={"t": t, "absent": None}, inputs={"also_absent": None}):
        pass
    assert torch.equal(gb.as_bytes(t), gb.as_bytes(src))
