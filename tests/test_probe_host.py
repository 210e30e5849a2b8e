"""CPU proof that the dyadic probes of tests/probe_weights.py are what they claim: the bit budget is within f32's 24 bits for every
family a probe is used with, the oracle in f32 equals the oracle in float64 bit for bit under each arithmetic, the probes cannot pass
vacuously (caps below, stated and not measured), the plain-C oracle agrees, and the comparison the GPU tests use rejects a reference
with a moved tap, a dropped `lo` term or truncated activations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import probe_weights as P
from dt4image_restoration_amd import weights
from dt4image_restoration_amd.unet_spec import STATE_DICT_KEYS, UNET_LAYERS
from oracle import pnp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (probe, arithmetic) pairs in use, from the matrix; the f4 row (route, f32) has a tolerance and no budget
_USES = sorted({(probe, row[0], row[1]) for row in P.MATRIX.values() for probe in row[4] if row[0]})
_SHAPES = sorted({(h, w) for row in P.MATRIX.values() for (_, h, w) in row[5]})
_SMALL = [(2, 16, 16), (1, 16, 48), (2, 96, 80), (1, 144, 64), (3, 32, 64)]


@pytest.mark.parametrize("probe", P.PROBES)
@pytest.mark.parametrize("seed", P.SEEDS)
def test_probe_state_dicts_load_and_cover_every_tap_and_channel(probe, seed):
    sd = P.probe_state_dict(probe, seed)
    assert list(sd.keys()) == STATE_DICT_KEYS and all(v.dtype == np.float32 for v in sd.values())
    chk = weights.check_state_dict(sd)
    blob = weights.flatten_state_dict(sd)
    assert blob.dtype == np.float32 and blob.size == sum(v.size for v in chk.values())
    O.torch_weights(sd)
    P.check_coverage(sd)
    assert float(sd["outc.conv.bias"][0]) == (2.0 ** -6 if probe == "lo" else 2.0 ** -5)
    if probe == "lo":                                        # both signs of the second bf16 term, and it is really needed
        w = torch.from_numpy(sd[UNET_LAYERS[5].weight_key])
        lo = (w - O._bf16(w))
        assert float(lo.min()) == -2.0 ** -11 and float(lo.max()) == 2.0 ** -11
        assert torch.equal(O._bf16(w) + O._bf16(lo), w)
    other = P.probe_state_dict(probe, 1 - seed)
    assert any(not np.array_equal(sd[k], other[k]) for k in STATE_DICT_KEYS)     # the seed moves the layout


def test_matrix_sweep_is_the_kernel_suite_sweep():
    import test_gpu_kernels
    assert P.SWEEP == test_gpu_kernels._SWEEP


@pytest.mark.parametrize("probe,family,arith", _USES)
@pytest.mark.parametrize("seed", P.SEEDS)
def test_bit_budget_fits_f32_at_every_matrix_shape(probe, family, arith, seed):
    """<= 24 significand bits in every 3x3 layer; in the read-out too for sum and route (32 terms of 2^-13 plus bias plus image).
    The `lo` read-out multiplies a 22-bit value by 2^-6 and adds image and bias: not exact, bounded by 2 * 2^-24 instead."""
    sd = P.probe_state_dict(probe, seed)
    for (h, w) in _SHAPES:                                   # (the budget does not depend on the size: see its docstring)
        bits = P.bit_budget(sd, family, (1, h, w))
        assert len(bits) == 28
        assert max(bits[:27]) <= 24, (h, w, bits)
        if probe != "lo":
            assert bits[27] <= 24, (h, w, bits)
        if (h, w) != _SHAPES[0]:
            assert bits == first
        first = bits


def test_bit_budget_refuses_what_does_not_fit():
    """`lo` in f32 arithmetic refines the grid by 11 bits per layer; dense weights are out at once."""
    assert max(P.bit_budget(P.probe_state_dict("lo", 0), "f32")[:27]) > 24
    assert max(P.bit_budget(P.probe_state_dict("lo", 0), "wino2")[:27]) > 24
    dense = {k: np.abs(v) for k, v in weights.generate_unet_weights(0, "unit_gain").items()}
    assert max(P.bit_budget(dense, "f32")[:27]) > 24


def _arithmetics(probe):
    return sorted({row[1] for row in P.MATRIX.values() if probe in row[4]})


@pytest.mark.parametrize("n,h,w", _SMALL)
@pytest.mark.parametrize("probe", P.PROBES)
@pytest.mark.parametrize("seed", P.SEEDS)
def test_f32_oracle_equals_float64_oracle_bit_for_bit(probe, seed, n, h, w):
    sd = P.probe_state_dict(probe, seed)
    x, sigma = P.probe_inputs(seed, n, h, w)
    for arith in _arithmetics(probe):
        o32, s32 = P.reference(sd, x, sigma, arith, torch.float32)
        o64, s64 = P.reference(sd, x, sigma, arith, torch.float64)
        for name in P.STAGES:
            P.assert_same_bits(s32[name], s64[name], f"{probe}/{arith} {name}")
        if probe == "lo":
            assert float((o32.double() - o64).abs().max()) <= P.LO_OUT_BOUND
        else:
            P.assert_same_bits(o32, o64, f"{probe}/{arith} output")
        assert float(o64.min()) > 0.0 and float(o64.max()) < 1.0           # the clamp does not act


@pytest.mark.parametrize("h,w", _SHAPES)
@pytest.mark.parametrize("probe", P.PROBES)
def test_probes_cannot_pass_vacuously(probe, h, w, monkeypatch):
    """Caps, at every size of the matrix (two slices: one per sigma) and for both seeds: every stage >= 50 % non-zero and >= 16 distinct
    values; `lo` under two-term and one-term weights differs on >= 10 % of every stage; `sum` under bf16 operands differs from f32
    arithmetic in at least three stages; every pre-activation is >= 0 (same bits with the LeakyReLU slope set to 1); the output stays
    inside (0, 1)."""
    for seed in P.SEEDS:
        sd = P.probe_state_dict(probe, seed)
        x, sigma = P.probe_inputs(seed, 2, h, w)
        assert set(np.unique(x.numpy() * 16)) <= set(range(16)) and len(np.unique(x.numpy())) == 16
        arith = "bf16" if probe == "lo" else "f32"
        out, st = P.reference(sd, x, sigma, arith)
        for name in P.STAGES:
            assert float((st[name] != 0).double().mean()) >= 0.5, name
            assert st[name].unique().numel() >= 16, name
        assert float(out.min()) > 0.0 and float(out.max()) < 1.0
        monkeypatch.setattr(O, "LEAKY", 1.0)
        out1, st1 = P.reference(sd, x, sigma, arith)
        monkeypatch.undo()
        assert torch.equal(out1, out) and all(torch.equal(st1[k], st[k]) for k in P.STAGES)
        if probe == "lo":
            _, one = P.reference(sd, x, sigma, "bf16w1")
            for name in P.STAGES:
                assert P.differing_fraction(st[name], one[name]) >= 0.10, name
        if probe == "sum":
            _, b = P.reference(sd, x, sigma, "bf16")
            assert sum(1 for name in P.STAGES if not torch.equal(st[name], b[name])) >= 3


def test_clamp_variants_are_exact_and_clamped():
    """`sum` with the read-out bias moved by +-1 (everything clamps) and +-1/2 (about half does): still exact."""
    x, sigma = P.probe_inputs(0, 2, 48, 64)
    for bias, lo_frac, hi_frac in ((2.0 ** -5 + 1, 1.0, 1.0), (2.0 ** -5 - 1, 1.0, 1.0), (2.0 ** -5 + 0.5, 0.3, 0.7), (2.0 ** -5 - 0.5, 0.3, 0.7)):
        sd = P.probe_state_dict("sum", 0, outc_bias=bias)
        o32, _ = P.reference(sd, x, sigma, "f32")
        o64, _ = P.reference(sd, x, sigma, "f32", torch.float64)
        P.assert_same_bits(o32, o64, f"bias {bias}")
        frac = float(((o32 == 0) | (o32 == 1)).double().mean())
        assert lo_frac <= frac <= hi_frac, (bias, frac)


def test_c_oracle_agrees_on_a_probe():
    """A second, ATen-free witness: oracle/pnp_ref.c (direct loops, double accumulation) on the f32 probes, whole denoiser, exactly."""
    so = os.path.join(ROOT, "oracle", "libpnp_ref.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
    ref = C.CDLL(so)
    n, h, w = 2, 32, 48
    for probe in ("sum", "route"):
        sd = P.probe_state_dict(probe, 1)
        x, sigma = P.probe_inputs(1, n, h, w)
        blob = weights.flatten_state_dict(sd)
        xn, sn = np.ascontiguousarray(x.numpy()), np.ascontiguousarray(sigma.numpy())
        out = np.empty_like(xn)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ref.ref_denoise(p(blob), p(xn), p(sn), p(out), n, h, w, 1) == 0
        want, _ = P.reference(sd, x, sigma, "f32", torch.float64)
        P.assert_same_bits(torch.from_numpy(out), want, f"C oracle, {probe}")


# ---- sensitivity: the comparison of the GPU tests rejects a perturbed reference ---------------------------------------------------
_ALWAYS_F32 = ("x5", "y1", "y2", "y3")


def _rejects(got, ref, probe):
    """Both forms in which the GPU tests call the comparison: with all nine stages (keep_stages handles), and with the output and the
    stages that every production handle keeps readable in f32 - the ones that feed an upsample.  The second form is needed: the weights on
    the upsampled half being zero, the OUTPUT of a probe sees level 0 alone."""
    with pytest.raises(AssertionError):
        P.assert_probe_result(got[0], got[1], ref[0], ref[1], probe)
    with pytest.raises(AssertionError):
        P.assert_probe_result(got[0], {k: got[1][k] for k in _ALWAYS_F32}, ref[0], ref[1], probe)


@pytest.mark.parametrize("probe,arith", [("route", "f32"), ("sum", "f32"), ("sum", "bf16"), ("lo", "bf16")])
@pytest.mark.parametrize("li", [1, 7, 13, 16, 24, 26])
def test_comparison_rejects_one_moved_tap(probe, arith, li):
    """One tap of one output channel of one layer moved by one position (every source mode: plain, pooled, upsample-concat)."""
    n, h, w = 2, 48, 64
    sd = P.probe_state_dict(probe, 0)
    x, sigma = P.probe_inputs(0, n, h, w)
    ref = P.reference(sd, x, sigma, arith)
    P.assert_probe_result(ref[0], ref[1], ref[0], ref[1], probe)           # ... and accepts the unperturbed one
    bad = {k: v.copy() for k, v in sd.items()}
    wt = bad[UNET_LAYERS[li].weight_key].reshape(UNET_LAYERS[li].cout, UNET_LAYERS[li].cin, 9)
    o = 5
    c, p = [int(v[0]) for v in np.nonzero(wt[o])]
    wt[o, c, (p + 1) % 9], wt[o, c, p] = wt[o, c, p], 0.0
    _rejects(P.reference(bad, x, sigma, arith), ref, probe)


@pytest.mark.parametrize("li", [1, 4, 8, 12, 15, 21, 24, 26])
def test_comparison_rejects_a_dropped_lo_term(li):
    n, h, w = 2, 48, 64
    sd = P.probe_state_dict("lo", 1)
    x, sigma = P.probe_inputs(1, n, h, w)
    ref = P.reference(sd, x, sigma, "bf16")
    _rejects(P.reference(sd, x, sigma, O.Bf16Plan(layer_terms={li: 1})), ref, "lo")


@pytest.mark.parametrize("probe", ["sum", "lo"])
def test_comparison_rejects_truncated_activations(probe):
    n, h, w = 2, 96, 80
    sd = P.probe_state_dict(probe, 0)
    x, sigma = P.probe_inputs(0, n, h, w)
    ref = P.reference(sd, x, sigma, "bf16")
    got = P.reference(sd, x, sigma, "trunc")
    _rejects(got, ref, probe)
