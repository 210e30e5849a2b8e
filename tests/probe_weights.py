"""Dyadic probe weights for the denoiser's conv kernels (no test in here; tests/test_probe_host.py proves what is claimed below on
the CPU, tests/test_gpu_probe.py uses it on the GPU).  tests/variant_cases.py is the table of every handle the probes and the oracle are
run on, MATRIX below included; tests/test_variant_reach_host.py checks it against the kernel variants a default handle can plan.

A probe is a full 56-key state dict, an image batch and a sigma vector made of small dyadic rationals, with at most two non-zero taps
per output channel, non-negative everywhere (LeakyReLU is the identity) and zero weights on the bilinearly upsampled half of every
`up*.conv-0` input (align_corners fractions are not dyadic; the skip half carries the signal).  Every product and every partial sum of
a conv, in ANY order, split or tile, is then exactly representable in f32 as long as `bit_budget` says <= 24 bits, so the only correct
result is the float64 one, bit for bit; in bf16 mode the rounding of an exact value is a deterministic function, so nothing can flip.

  route  one tap of weight 1 per output channel: pure indexing, every value on the grid 2^-4
  sum    route + a second tap in each stage's middle conv (both 1/2): accumulation; the grid refines by one bit per stage, so the bf16
         kernels round activations with more than 8 significant bits (nearest even, ties included)
  lo     one tap of 1545/2048 (even output channels: hi = 193/256, lo = +2^-11) or 1551/2048 (odd: hi = 194/256, lo = -2^-11) in every
         layer with Cin >= 32: a weight that needs both bf16 terms, with either sign of the second.  bf16 families only (in f32
         arithmetic the grid refines by 11 bits per layer).  Its biases are >= 2^-4 everywhere: that floor on the activations is what
         bounds the exponent range inside a sum, see `bit_budget`.

Tap 0 of output channel o reads input channel (o + seed) % cin_eff at position (o // cin_eff + o + seed) % 9 (cin_eff: the skip
channels of an upsample-concat layer; the two-channel first layer: (o // 2 + seed) % 9); at the two
lowest levels every even channel reads the centre instead, so that the 2 x 2 and 1 x 1 levels of a 16 x 16 slice still carry signal.  The second tap takes channel and position from `hash_uniform`.
"""
from __future__ import annotations

import functools
import hashlib
from fractions import Fraction
from typing import Dict, List, Optional

import numpy as np
import torch

from dt4image_restoration_amd import synthetic
from dt4image_restoration_amd.unet_spec import SRC_UPCAT, UNET_LAYERS
from oracle import pnp_oracle as O

PROBES = ("route", "sum", "lo")
STAGES = ("x1", "x2", "x3", "x4", "x5", "y1", "y2", "y3", "y4")
W_LO = (1545.0 / 2048.0, 1551.0 / 2048.0)      # 0.75 * (1 + 3 * 2^-9): lo = +2^-11;  0.75 * (1 + 5 * 2^-9): lo = -2^-11
OUTC_BIAS = 2.0 ** -5                         # route / sum
OUTC_BIAS_LO = 2.0 ** -6
LO_OUT_BOUND = 2.0 * 2.0 ** -24               # lo output = x + 2^-6 * a + b: at most two f32 roundings of values <= 1


def _cin_eff(l) -> int:
    return l.cskip if l.src == SRC_UPCAT else l.cin


def _first_tap(l, o: int, seed: int):
    ce = _cin_eff(l)
    pos = (o // ce + (o if ce >= 9 else 0) + seed) % 9      # (two input channels: o // 2 alone walks all nine for each)
    if l.level >= 3 and o % 2 == 0:
        pos = 4
    return (o + seed) % ce, pos


def _readout_shift(probe: str) -> int:
    """k of the 2^-k read-out weights: the smallest for which the budget's bound keeps x + residual + bias below 1 (x <= 15/16)."""
    return {"route": 13, "sum": 13, "lo": 6}[probe]


def probe_state_dict(probe: str, seed: int = 0, outc_bias: Optional[float] = None) -> Dict[str, np.ndarray]:
    """{key: float32 ndarray} under the 56 reference key names (unet_spec.STATE_DICT_KEYS)."""
    assert probe in PROBES, probe
    sd: Dict[str, np.ndarray] = {}
    for l in UNET_LAYERS[:27]:
        ce = _cin_eff(l)
        w = np.zeros((l.cout, l.cin, 9), np.float32)
        two = probe == "sum" and l.index % 3 == 1
        u = synthetic.hash_uniform(seed, 1000 + l.index, 2 * l.cout).astype(np.float64)
        for o in range(l.cout):
            c0, p0 = _first_tap(l, o, seed)
            if probe == "lo" and l.cin >= 32:
                w[o, c0, p0] = W_LO[o & 1]
            else:
                w[o, c0, p0] = 0.5 if two else 1.0
            if two:
                c1 = min(int((u[2 * o] + 1) * 0.5 * ce), ce - 1)
                p1 = min(int((u[2 * o + 1] + 1) * 0.5 * 9), 8)
                w[o, c1, p1] += 0.5                      # on the first tap's place: one tap of 1
        sd[l.weight_key] = w.reshape(l.cout, l.cin, 3, 3)
        # bias k * 2^-4, k = 0..2 (lo: 1..3) from the hash: o % 3 would add up to the same total along every channel chain
        kb = np.minimum(np.floor((synthetic.hash_uniform(seed, 2000 + l.index, l.cout).astype(np.float64) + 1) * 1.5), 2)
        sd[l.bias_key] = ((kb + (1 if probe == "lo" else 0)) * 2.0 ** -4).astype(np.float32)
    l = UNET_LAYERS[27]
    w = np.zeros((1, 32, 1, 1), np.float32)
    k = _readout_shift(probe)
    if probe == "lo":
        w[0, (5 + 7 * seed) % 32] = 2.0 ** -k                # one channel: a 24-bit value times a power of two, bias and image added
    else:
        w[:] = 2.0 ** -k
    sd[l.weight_key] = w
    default = OUTC_BIAS_LO if probe == "lo" else OUTC_BIAS
    sd[l.bias_key] = np.full((1,), default if outc_bias is None else outc_bias, np.float32)
    return sd


def probe_inputs(seed: int, n: int, h: int, w: int):
    """(x [n,1,h,w] with values k/16, k = 0..15, sigma [n] alternating 1/4, 1/8), float32 torch tensors."""
    u = synthetic.hash_uniform(seed, 77 + 1000 * h + w, n * h * w).astype(np.float64)
    k = np.minimum(np.floor((u + 1) * 8), 15)
    x = torch.from_numpy((k / 16).astype(np.float32).reshape(n, 1, h, w))
    sigma = torch.tensor([0.25 if i % 2 == 0 else 0.125 for i in range(n)], dtype=torch.float32)
    return x, sigma


def check_coverage(sd) -> None:
    """Over the output channels of every 3x3 layer each of the 9 tap positions is used, and each input channel of the half that is not
    zeroed; the upsampled half of an upsample-concat layer has zero weights; everything is >= 0 and at most two taps per channel."""
    for l in UNET_LAYERS[:27]:
        w = sd[l.weight_key].reshape(l.cout, l.cin, 9)
        ce = _cin_eff(l)
        assert (w >= 0).all() and (sd[l.bias_key] >= 0).all(), l.key
        assert not w[:, ce:].any(), l.key
        nz = w != 0
        assert nz.any(axis=(0, 1)).all(), f"{l.key}: tap positions {np.flatnonzero(~nz.any(axis=(0, 1)))} unused"
        assert nz[:, :ce].any(axis=(0, 2)).all(), f"{l.key}: unused input channels"
        per = nz.sum(axis=(1, 2))
        assert per.min() >= 1 and per.max() <= 2, l.key


# ---- bit budget ---------------------------------------------------------------------------------------------------------------------
def _grid(a: np.ndarray) -> int:
    """smallest g >= 0 with every element of a (float64, dyadic) a multiple of 2^-g"""
    a = np.abs(np.asarray(a, np.float64))
    a = a[a != 0]
    g = 0
    while a.size and g < 200:
        a = a[np.floor(a) != a]
        if not a.size:
            break
        a = a * 2
        g += 1
    assert g < 200, "not dyadic"
    return g


def _bits(bound: Fraction, grid: int) -> int:
    """significand bits that hold every multiple of 2^-grid up to `bound` in magnitude"""
    return max(int(bound * 2 ** grid).bit_length(), 1)


def _bf16_np(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _bf16_up(v: Fraction) -> Fraction:
    """smallest 8-bit-significand value >= v > 0"""
    e = v.numerator.bit_length() - v.denominator.bit_length()
    while Fraction(2) ** e > v:
        e -= 1
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    step = Fraction(2) ** (e - 7)
    q = v / step
    return step * (q.numerator // q.denominator + (0 if q.denominator == 1 else 1))


def _floor_log2(v: Fraction) -> int:
    e = v.numerator.bit_length() - v.denominator.bit_length()
    while Fraction(2) ** e > v:
        e -= 1
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    return e


_WINO_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


def bit_budget(sd, family: str, shape=None) -> List[int]:
    """Significand bits that the widest partial sum of each of the 28 layers can need when the state dict `sd` runs on images with
    values k/16 <= 15/16 and sigma on the grid 2^-4, in the arithmetic of `family`:

      "f32"     products and sums of f32 operands in any order (direct kernels, split-K planes, fused first / last layer)
      "wino2"   F(2x2, 3x3): input transform B^T d B (entries 0, +-1: four terms), U = G g G^T (1, 1/2, 1/4), the products summed over
                the input channels, output transform A^T M A (nine terms) - every one of them dyadic
      "bf16"    layers with Cin >= 32: the activation rounded to 8 bits, times hi = bf16(w) and times lo = bf16(w - hi), all summed in f32
      "bf16w1"  the same with hi alone

    It propagates, layer by layer and in exact arithmetic (`fractions`; float64 only on dyadic weights, where it is exact), the grid
    2^-g every activation lies on, the bound max_o(sum|w| * max|a| + |b|) and - all terms being >= 0 - a floor under the non-zero
    activations, along the network's graph (an upsample-concat layer takes the state of its skip tensor).  The floor matters in the bf16 families: an 8-bit activation a >= m lies on the grid 2^(floor(log2 m) - 7), however
    fine the grid of the unrounded tensor was.  `shape` (n, h, w) is accepted for the callers' convenience: pooling, the zero padding
    and the zero-weighted upsample change neither grid nor bound, so the budget holds at every size.  The last entry (outc) includes
    the residual addition of the image."""
    assert family in ("f32", "wino2", "bf16", "bf16w1"), family
    key = (family, hashlib.sha1(b"".join(np.ascontiguousarray(sd[k], np.float32).tobytes() for k in sorted(sd))).hexdigest())
    if key not in _BUDGETS:
        _BUDGETS[key] = _bit_budget(sd, family)
    return list(_BUDGETS[key])


_BUDGETS: Dict[tuple, List[int]] = {}


def _bit_budget(sd, family: str) -> List[int]:
    g, hi_a, lo_a = 4, Fraction(15, 16), Fraction(1, 16)     # image k/16 and sigma 1/4, 1/8
    out: List[int] = []
    after = {}
    for l in UNET_LAYERS:
        if l.src == SRC_UPCAT:                                # reads the skip tensor alone: the weights on the upsampled half are zero
            if np.asarray(sd[l.weight_key])[:, l.cskip:].any():          # bilinear fractions are not dyadic: nothing fits from here on
                return out + [999] * (28 - len(out))
            g, hi_a, lo_a = after[{15: 11, 18: 8, 21: 5, 24: 2}[l.index]]
        w = np.asarray(sd[l.weight_key], np.float64).reshape(l.cout, l.cin, -1)
        b = np.asarray(sd[l.bias_key], np.float64)
        assert (w >= 0).all() and (b >= 0).all()
        terms = [w]
        ga, hi_in, lo_in = g, hi_a, lo_a
        if family in ("bf16", "bf16w1") and l.cin >= 32 and l.ksize == 3:
            whi = _bf16_np(w)
            terms = [whi] if family == "bf16w1" else [whi, _bf16_np(w - whi)]
            assert family == "bf16w1" or (terms[0] + terms[1] == w).all()
            hi_in = _bf16_up(hi_a)
            ga = min(g, 7 - _floor_log2(lo_a))            # rounding keeps a value >= the floor when the floor is a power of two
            assert lo_a == Fraction(2) ** _floor_log2(lo_a)
        weff = sum(terms)
        assert (weff >= 0).all()
        gw = max(_grid(t) for t in terms)
        gb = _grid(b)
        gsum = max(ga + gw, gb, 4 if l.ksize == 1 else 0)
        sabs = sum(np.abs(t) for t in terms).sum(axis=(1, 2))
        bound = max(Fraction(float(s)) * hi_in + Fraction(float(bb)) for s, bb in zip(sabs, b)) + (1 if l.ksize == 1 else 0)
        bits = _bits(bound, gsum)
        if family == "wino2" and l.ksize == 3:
            U = np.einsum("ik,ockl,jl->ocij", _WINO_G, w.reshape(l.cout, l.cin, 3, 3), _WINO_G)
            assert (U.astype(np.float32).astype(np.float64) == U).all()
            gu = _grid(U)
            sm = Fraction(float(np.abs(U).sum(axis=1).max())) * 4 * hi_in
            bits = max(bits, _bits(4 * hi_in, ga), _bits(sm, ga + gu), _bits(9 * sm + Fraction(float(b.max())), max(ga + gu, gb)))
        out.append(bits)
        # what the layer hands on: exact values sum(weff * a) + b
        # (floor, all terms being >= 0: a channel with a bias never falls below it; one without, not below its smallest weight times the floor)
        wmin = np.where(weff > 0, weff, np.inf).min(axis=(1, 2))
        lo_a = Fraction(2) ** _floor_log2(min(Fraction(float(bb)) if bb > 0 else Fraction(float(wm)) * lo_in for wm, bb in zip(wmin, b)))
        hi_a = max(Fraction(float(s)) * hi_in + Fraction(float(bb)) for s, bb in zip(weff.sum(axis=(1, 2)), b))
        g = max(ga + _grid(weff), gb)
        after[l.index] = (g, hi_a, lo_a)
    return out


# ---- references ------------------------------------------------------------------------------------------------------------------------
class TruncPlan(O.Bf16Plan):
    """A WRONG arithmetic, for the sensitivity test: activations truncated to bf16 instead of rounded to nearest even."""

    def operands(self, li, x, w):
        xi = x.to(torch.float32).contiguous().view(torch.int32) & -65536
        plain = O.Bf16Plan(acts=False, weight_terms=self.weight_terms, layer_terms=self.layer_terms)
        return xi.view(torch.float32).to(x.dtype), plain.operands(li, x, w)[1]


def plan_of(arith: str):
    return {"f32": False, "bf16": O.Bf16Plan(), "bf16w1": O.Bf16Plan(weight_terms=1), "trunc": TruncPlan()}[arith]


def reference(sd_np, x: torch.Tensor, sigma: torch.Tensor, arith="f32", dtype=torch.float32):
    """(clamped output, {stage name: tensor}) of the oracle in `dtype`; arith: a key of `plan_of` or a Bf16Plan."""
    n, _, h, w = x.shape
    sd = O.torch_weights(sd_np, dtype)
    xin = torch.cat([x.to(dtype), torch.ones(n, 1, h, w, dtype=dtype) * sigma.to(dtype).reshape(n, 1, 1, 1)], 1)
    raw, stages = O.unet_forward(sd, xin, return_stages=True, bf16_operands=plan_of(arith) if isinstance(arith, str) else arith)
    return torch.clamp(raw, 0, 1), stages


@functools.lru_cache(maxsize=2)
def cached_reference(probe: str, seed: int, n: int, h: int, w: int, arith: str = "f32", outc_bias: Optional[float] = None):
    """f32 oracle on a probe (test_probe_host.py proves it equal to the float64 one), eight slices at a time; the last few cases are
    kept, so that handles which differ in a knob only share a run (the 64-slice runs are the long pole of the GPU file)."""
    x, sigma = probe_inputs(seed, n, h, w)
    sd = probe_state_dict(probe, seed, outc_bias)
    parts = [reference(sd, x[i:i + 8], sigma[i:i + 8], arith) for i in range(0, n, 8)]
    return torch.cat([p[0] for p in parts]), {k: torch.cat([p[1][k] for p in parts]) for k in STAGES}


# ---- the GPU matrix (tests/test_gpu_probe.py runs it, tests/test_probe_host.py proves budgets and caps at its shapes) ---------------
SWEEP = [(1, 16, 48), (5, 32, 16), (2, 80, 48), (3, 96, 112), (1, 144, 64), (4, 16, 16), (2, 64, 176), (1, 208, 32)]   # test_gpu_kernels._SWEEP
# row: (budget family, arithmetic of the oracle, engine in bf16 mode, environment, probes, shapes)
MATRIX = {
    "direct": ("f32", "f32", False, {"PNP_NO_WINOGRAD": "1"}, ("sum", "route"), SWEEP + [(2, 256, 256), (1, 16, 1024), (1, 1024, 16)]),
    "wino2": ("wino2", "f32", False, {"PNP_WINO_MIN_BLOCKS": "1", "PNP_NO_WINO_F4": "1"}, ("sum", "route"),
              [(1, 32, 32), (2, 48, 64), (3, 64, 16), (64, 128, 128)]),
    "bf16": ("bf16", "bf16", True, {}, ("sum", "lo"),
             SWEEP + [(2, 256, 256), (16, 256, 256), (64, 256, 256), (2, 512, 512), (1, 1008, 112)]),
    "bf16-no-ws": ("bf16", "bf16", True, {"PNP_BF16_NO_WS": "1"}, ("sum", "lo"), [(3, 48, 80), (16, 256, 256)]),
    "bf16-f32-acts": ("bf16", "bf16", True, {"PNP_BF16_F32_ACTS": "1"}, ("sum", "lo"), [(3, 48, 80), (16, 256, 256)]),
    "bf16-no-holdhi": ("bf16", "bf16", True, {"PNP_BF16_NO_HOLDHI": "1"}, ("sum", "lo"), [(3, 48, 80), (16, 256, 256)]),
    "bf16-w1": ("bf16w1", "bf16w1", True, {"PNP_BF16_W1": "1"}, ("lo",), [(2, 128, 128), (16, 256, 256)]),
    "f4": (None, "f32", False, {}, ("route",), [(2, 256, 256), (3, 128, 64), (8, 272, 272), (64, 256, 256)]),
}
SEEDS = (0, 1)


# ---- the comparison the GPU tests use ---------------------------------------------------------------------------------------------
def assert_same_bits(got: torch.Tensor, ref: torch.Tensor, name: str, tile: int = 32) -> None:
    """got == ref bit for bit (ref may be float64: compared as values, which for f32-representable numbers is the same thing).
    On failure: how many differ, and the first few with channel, coordinates and coordinates modulo the tile size - with one or two
    taps per channel the tap and channel at fault can be read off."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    bad = got.to(torch.float64) != ref.to(torch.float64)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    lines = []
    for idx in bad.nonzero()[:12].tolist():
        i, c, y, x = idx
        lines.append(f"  n={i} c={c} y={y} x={x} (y%{tile}={y % tile} x%{tile}={x % tile}): got {float(got[i, c, y, x])!r} want {float(ref[i, c, y, x])!r}")
    err = float((got.to(torch.float64) - ref.to(torch.float64)).abs().max())
    chans = sorted(set(bad.nonzero()[:, 1].tolist()))[:16]
    raise AssertionError(f"{name}: {nbad} of {bad.numel()} elements differ (max |diff| {err:.3e}; channels {chans} ...)\n" + "\n".join(lines))


def assert_probe_result(got_out, got_stages, ref_out, ref_stages, probe: str, label: str = "") -> int:
    """The acceptance rule of a probe run: every stage handed in equals the reference bit for bit; the output too, except for `lo`,
    whose output is within LO_OUT_BOUND.  got_stages: {name: tensor}, all nine or the ones a production handle can read.  Returns the number of elements
    compared bit for bit."""
    count = 0
    for name, a in (got_stages or {}).items():
        assert_same_bits(a, ref_stages[name], f"{label} stage {name}")
        count += a.numel()
    if probe == "lo":
        err = float((got_out.detach().cpu().to(torch.float64) - ref_out.to(torch.float64)).abs().max())
        assert err <= LO_OUT_BOUND, f"{label} output: max |diff| {err:.3e} > 2^-23"
    else:
        assert_same_bits(got_out, ref_out, f"{label} output")
        count += got_out.numel()
    return count


def differing_fraction(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.detach().cpu().to(torch.float64) != b.detach().cpu().to(torch.float64)).double().mean())
