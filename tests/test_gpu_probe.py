"""Every conv kernel family against the float64-exact answer on the dyadic probes of tests/probe_weights.py: bit for bit where the
bit budget says a correct kernel cannot differ (tests/test_probe_host.py proves the budgets, the f32 == float64 equality of the oracle
and the caps against passing vacuously, on the CPU), and for F(4x4) - whose points +-3/4, +-3/2 are not exact - within the suite's
f32 bound AND equal after rounding to the probe's grid.

A keep_stages handle compares all nine stage tensors and the output.  A production handle - the only way to the fused first and last
layer, the pooled epilogues and the bf16 activation storage - compares the output and every stage it still holds in f32 (always x5,
y1, y2, y3: what feeds an upsample).  The stages are needed: the upsampled half carrying zero weights, a probe's OUTPUT sees level 0
alone.  Also here: reloading weights on a live handle, a non-zero last-layer bias with dense weights on every fused-last code path,
and the clamp."""
import numpy as np
import pytest
import torch

import probe_weights as P
from dt4image_restoration_amd import weights
from oracle import pnp_oracle as O

pytestmark = pytest.mark.gpu

KEEP_MAX_N = 16            # keep_stages handles up to this batch; the 64-slice cases run the production handle alone


def _cases():
    out = []
    for row, (family, arith, bf16, env, probes, shapes) in P.MATRIX.items():
        for probe in probes:
            for shape in shapes:
                for seed in P.SEEDS:
                    out.append((arith, probe, seed, shape, row))
    out.sort(key=lambda c: (c[0], c[1], c[2], c[3], c[4]))    # handles that share an oracle run (cached_reference) side by side
    return out


CASES = _cases()
CASE_IDS = [f"{row}-{probe}-s{seed}-{n}x{h}x{w}" for (_, probe, seed, (n, h, w), row) in CASES]
# one case per family also runs denoise twice and requires the same bits
REPEAT = {("direct", "sum", 0, (3, 96, 112)), ("wino2", "sum", 0, (2, 48, 64)),
          ("bf16", "lo", 0, (16, 256, 256)), ("bf16-no-ws", "lo", 0, (3, 48, 80)), ("bf16-w1", "lo", 0, (2, 128, 128)),
          ("f4", "route", 0, (2, 256, 256))}


def _engine(n, h, w, bf16, keep_stages, env, monkeypatch):
    from dt4image_restoration_amd.engine import PnPEngine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return PnPEngine(n, h, w, keep_stages=keep_stages, bf16_convs=bf16)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _check_family(e, row, n, keep_stages):
    """the handle is on the family the row is about (codes: 0 direct, 1 F(2x2), 4 F(4x4), 5 bf16 producer / consumer)"""
    algos = e.conv_algorithms()
    mid = algos[1:27]
    if row.startswith("direct"):
        assert all(v == 0 for v in mid) and e.bf16_weight_terms() == 0, algos
    elif row == "wino2":
        assert 4 not in algos and sum(1 for v in algos if v == 1) >= (20 if n == 64 else 26 if keep_stages else 20), algos
    elif row == "f4":                                       # the default plan: F(4x4) where it is planned (at 64 x 256 x 256 it is)
        assert e.bf16_weight_terms() == 0 and (n < 64 or 4 in mid), algos
        print(f"default plan {n} slices: {algos}")
    else:
        assert all(v in (0, 5) for v in mid), algos
        assert e.bf16_weight_terms() == (1 if row == "bf16-w1" else 2)
        if row == "bf16-no-ws":
            assert 5 not in mid, algos
        elif n >= 16:
            assert 5 in mid, algos                          # chip-filling: the producer / consumer kernel


def _read_stages(e, keep_stages):
    from dt4image_restoration_amd._lib import PnPError
    got = {}
    for which, name in enumerate(P.STAGES):
        try:
            got[name] = e.read_stage(which).cpu()
        except PnPError:
            assert not keep_stages                          # fused away or held as bf16: production handles only
    assert all(k in got for k in ("x5", "y1", "y2", "y3"))
    return got


def _check_f4(out, stages, ref_out, ref_stages, label):
    """F(4x4) on `route`: the suite's f32 bound (test_winograd_f4_path_matches_oracle_per_stage, unchanged), and - every true value
    being a multiple of 2^-4, a wrong tap off by >= 2^-4 - exact equality after rounding to that grid.  The output's grid is 2^-17
    (32 read-out terms of 2^-13 on the 2^-4 grid): the stage bound, 2.2e-4 per element of y4 at most, moves it by < 9e-7, a quarter step."""
    for name, a in stages.items():
        ref = ref_stages[name]
        err = float((a - ref).abs().max())
        assert err < 5e-5 * max(1.0, float(ref.abs().max())), f"{label} stage {name}: max err {err}"
        P.assert_same_bits(torch.round(a * 16) / 16, ref, f"{label} stage {name}, rounded to 2^-4")
    np.testing.assert_allclose(out.numpy(), ref_out.numpy(), rtol=0, atol=1e-5)
    P.assert_same_bits(torch.round(out.double() * 2 ** 17) / 2 ** 17, ref_out, f"{label} output, rounded to 2^-17")


@pytest.mark.parametrize("arith,probe,seed,shape,row", CASES, ids=CASE_IDS)
def test_probe_is_bit_exact(arith, probe, seed, shape, row, monkeypatch):
    n, h, w = shape
    family, _, bf16, env, _, _ = P.MATRIX[row]
    env = {k: v for k, v in env.items() if not (k == "PNP_WINO_MIN_BLOCKS" and n >= 64)}    # (64 slices pass the gate by themselves)
    sd = P.probe_state_dict(probe, seed)
    if family is not None:
        assert max(P.bit_budget(sd, family, shape)[:27 if probe == "lo" else 28]) <= 24
    x, sigma = P.probe_inputs(seed, n, h, w)
    ref_out, ref_stages = P.cached_reference(probe, seed, n, h, w, arith)
    xg, sg = x.cuda(), sigma.cuda()
    compared = 0
    for keep_stages in ((True, False) if n <= KEEP_MAX_N else (False,)):
        label = f"{row} {probe} seed {seed} {n}x{h}x{w} {'keep_stages' if keep_stages else 'production'}"
        e = _engine(n, h, w, bf16, keep_stages, env, monkeypatch)
        try:
            e.load_weights(sd)
            _check_family(e, row, n, keep_stages)
            out = e.denoise(xg, sg).cpu()
            stages = _read_stages(e, keep_stages)
            if row == "f4" and 4 in e.conv_algorithms():           # (a default plan without F(4x4) - small problems - is exact)
                _check_f4(out, stages, ref_out, ref_stages, label)
            else:
                compared += P.assert_probe_result(out, stages, ref_out, ref_stages, probe, label)
            if (row, probe, seed, shape) in REPEAT:
                assert torch.equal(e.denoise(xg, sg).cpu(), out), f"{label}: second pass differs"
            if row == "bf16-w1" and keep_stages:
                # the built-in mutant: equal to the ONE-term oracle above, and far from the two-term one - the `lo` probe sees a missing term
                _, two = P.cached_reference(probe, seed, n, h, w, "bf16")
                fr = [P.differing_fraction(stages[k], two[k]) for k in P.STAGES]
                print(f"PNP_BF16_W1 {n}x{h}x{w} seed {seed}: fraction differing from the two-term oracle per stage {[round(f, 3) for f in fr]}")
                assert min(fr) >= 0.10, fr
        finally:
            e.close()
    print(f"{row} {probe} seed {seed} {n}x{h}x{w}: {compared} elements compared bit for bit")


# ---- the clamp ----------------------------------------------------------------------------------------------------------------------
CLAMP_SHAPE = (3, 256, 256)
CLAMP_ENV = {False: {"PNP_NO_WINOGRAD": "1"}, True: {}}        # by bf16 mode (f32: the direct kernels, exact; F(4x4) is not)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shift", [1.0, -1.0, 0.5, -0.5])
def test_probe_clamp_is_exact(shift, bf16, monkeypatch):
    """`sum` with the read-out bias moved by +-1 (every pixel clamps) and +-1/2 (about half): exact, on the fused last layer of the default
    f32 plan and of the bf16 plan, and on the layer's own kernel (keep_stages)."""
    n, h, w = CLAMP_SHAPE
    bias = 2.0 ** -5 + shift
    sd = P.probe_state_dict("sum", 0, outc_bias=bias)
    x, sigma = P.probe_inputs(0, n, h, w)
    ref_out, _ = P.cached_reference("sum", 0, n, h, w, "bf16" if bf16 else "f32", bias)
    assert float(((ref_out == 0) | (ref_out == 1)).double().mean()) >= (1.0 if abs(shift) == 1 else 0.3)
    for keep_stages in (False, True):
        e = _engine(n, h, w, bf16, keep_stages, CLAMP_ENV[bf16], monkeypatch)
        try:
            e.load_weights(sd)
            P.assert_same_bits(e.denoise(x.cuda(), sigma.cuda()), ref_out, f"clamp {shift:+} keep_stages={keep_stages}")
        finally:
            e.close()


# ---- reload on a live handle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_reload_weights_on_a_live_handle(bf16, monkeypatch):
    """pnp_load_unet_weights re-packs into fresh buffers and swaps them: dense -> probe -> dense on one handle gives the probe's exact
    answer in the middle (= a fresh handle's) and the first result again, bit for bit; a refused blob leaves the old weights in place."""
    from dt4image_restoration_amd import _lib
    from dt4image_restoration_amd._lib import PnPError
    n, h, w = 2, 128, 128
    dense = weights.generate_unet_weights(0, "unit_gain")
    probe = "lo" if bf16 else "sum"
    sd = P.probe_state_dict(probe, 1)
    x, sigma = P.probe_inputs(1, n, h, w)
    xg, sg = x.cuda(), sigma.cuda()
    env = {} if bf16 else {"PNP_NO_WINOGRAD": "1"}
    e = _engine(n, h, w, bf16, False, env, monkeypatch)
    fresh = _engine(n, h, w, bf16, False, env, monkeypatch)
    try:
        e.load_weights(dense)
        first = e.denoise(xg, sg).clone()
        e.load_weights(sd)
        second = e.denoise(xg, sg).clone()
        fresh.load_weights(sd)
        assert torch.equal(second, fresh.denoise(xg, sg))
        ref_out, ref_stages = P.cached_reference(probe, 1, n, h, w, "bf16" if bf16 else "f32")
        P.assert_probe_result(second.cpu(), {}, ref_out, ref_stages, probe, "reloaded probe")
        blob = np.ascontiguousarray(weights.flatten_state_dict(dense))
        for bad in (blob[:-1], np.concatenate([blob, blob[:1]])):                  # wrong length: refused before anything is touched
            bad = np.ascontiguousarray(bad)
            with pytest.raises(PnPError):
                _lib.check(e.lib.pnp_load_unet_weights(e._h, bad.ctypes.data, bad.size), "pnp_load_unet_weights")
        assert torch.equal(e.denoise(xg, sg), second)           # still the probe
        e.load_weights(dense)
        assert torch.equal(e.denoise(xg, sg), first)
        assert not torch.equal(first, second)
    finally:
        e.close()
        fresh.close()


# ---- a non-zero last-layer bias with dense weights -------------------------------------------------------------------------------------
_BIAS_PATHS = [
    ("f4-fused", False, {}, (3, 256, 256), 4),
    ("f4-unfused", False, {"PNP_NO_F4_FUSED_LAST": "1"}, (3, 256, 256), 1),
    ("wino2", False, {"PNP_NO_WINO_F4": "1"}, (3, 256, 256), 1),
    ("direct", False, {"PNP_NO_WINOGRAD": "1"}, (3, 256, 256), 0),
    ("bf16-direct", True, {"PNP_BF16_NO_WS": "1"}, (16, 256, 256), 0),
    ("bf16-ws", True, {}, (16, 256, 256), 5),
]


@pytest.mark.parametrize("name,bf16,env,shape,algo26", _BIAS_PATHS, ids=[p[0] for p in _BIAS_PATHS])
def test_dense_weights_with_nonzero_last_bias(name, bf16, env, shape, algo26, monkeypatch):
    """`unit_gain` has outc.conv.bias == 0, so the bias read of the five fused-last epilogues (F(4x4), F(2x2), direct f32, bf16 direct,
    bf16 producer / consumer) was never seen with dense weights, LeakyReLU's negative branch and the clamp.  Bias 0.03, one production
    handle per code path (up4.conv-2's algorithm says which), against the oracle with the suite's tolerances."""
    n, h, w = shape
    sd = dict(weights.generate_unet_weights(0, "unit_gain"))
    sd["outc.conv.bias"] = np.full((1,), 0.03, np.float32)
    from dt4image_restoration_amd import synthetic
    x = (torch.from_numpy(synthetic.hash_uniform(41, h * 1000 + w, n * h * w).reshape(n, 1, h, w)) + 1) * 0.5
    sigma = torch.linspace(5, 50, n) / 255.0
    e = _engine(n, h, w, bf16, False, env, monkeypatch)
    try:
        e.load_weights(sd)
        assert e.conv_algorithms()[26] == algo26, e.conv_algorithms()
        got = e.denoise(x.cuda(), sigma.cuda()).cpu()
    finally:
        e.close()
    sdt = O.torch_weights(sd)
    ref = torch.cat([O.denoise(sdt, x[i:i + 8], sigma[i:i + 8], bf16_operands=bf16) for i in range(0, n, 8)])
    zero = dict(sdt)
    zero["outc.conv.bias"] = torch.zeros(1)
    assert float((ref[:1] - O.denoise(zero, x[:1], sigma[:1], bf16_operands=bf16)).abs().max()) > 0.02     # the bias is in the answer
    # FLOAT TOLERANCE: f32 summation order (1e-5); bf16 operands: rounding flips reach the output at ~1e-3 (test_gpu_kernels.py)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=2e-3 if bf16 else 1e-5)
