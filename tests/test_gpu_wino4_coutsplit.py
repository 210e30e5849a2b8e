"""The cout-split schedule of the F(4x4) conv (conv3x3_wino4c_kernel: one 16-tile M-block x 128 output channels per workgroup,
PNP_WINO_F4_CS) against the schedules it stands beside, against the oracle and on the dyadic probes.

All handles: PNP_WINO_MIN_BLOCKS=1, PNP_WINO_F4_MIN_CIN=64, keep_stages (as test_winograd_f4_path_matches_oracle_per_stage).

Bit identity: the existing schedules agree among themselves in bits (default mix against PNP_NO_WINO_F4_PHASED=1 PNP_WINO_F4_MT16=1, checked
on the parent build at these shapes, profiles/wino4_coutsplit.md), a tile's arithmetic being the same in all of them; so PNP_WINO_F4_CS=2 is
compared with PNP_WINO_F4_CS=0 (the default mix) by torch.equal.

Which layers must take the schedule: every layer that is on F(4x4) in the PNP_WINO_F4_CS=0 handle and has Cout % 128 == 0, upsample +
concat layers included (winograd_plan's rule) - asserted layer by layer, and that this set is not empty.  At (2, 96, 112) it IS empty: the 128-channel level is
24 x 28 there, which F(4x4) does not take at all (it wants 32 pixels in one direction, or 16 x 16), with or without the new schedule, so
that shape runs the old kernels in both handles and only guards the plan.  (2, 144, 112) is added for what that shape was meant to
exercise: its 128-channel level is 36 x 28 - partial tile columns AND a partial last tile row on TW = 16 under the new kernel."""
import contextlib
import os

import numpy as np
import pytest
import torch

import probe_weights as P
from dt4image_restoration_amd import synthetic, unet_spec, weights
from oracle import pnp_oracle as O

pytestmark = pytest.mark.gpu

ENV = {"PNP_WINO_MIN_BLOCKS": "1", "PNP_WINO_F4_MIN_CIN": "64"}
SHAPES = [(3, 256, 256), (2, 128, 128), (1, 144, 64), (2, 96, 112), (2, 144, 112)]
NO_F4_LEVEL = {(2, 96, 112)}           # no 128-channel level that F(4x4) takes (see the module docstring)
IDS = ["x".join(map(str, s)) for s in SHAPES]
SCHED_COUT_SPLIT = 4
CS_VALUES = (2, 0)                     # PNP_WINO_F4_CS of the two handles every test here compares
PROBE_SHAPE = (2, 128, 128)            # test_dyadic_probe_weights_under_coutsplit
STEP_SHAPE = (3, 256, 256)             # test_a_stopped_slice_keeps_its_bits_and_the_live_ones_match


@pytest.fixture(scope="module")
def sd_np():
    return weights.generate_unet_weights(0, "unit_gain")


@contextlib.contextmanager
def _env(cs):
    env = dict(ENV, PNP_WINO_F4_CS=str(cs))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(n, h, w, sd, cs):
    """keep_stages handle planned under PNP_WINO_F4_CS=cs (the switches are read once, at pnp_create)"""
    from dt4image_restoration_amd.engine import PnPEngine
    with _env(cs):
        e = PnPEngine(n, h, w, keep_stages=True)
    e.load_weights(sd)
    return e


def _expected_layers(algos0):
    """layers the schedule can take: on F(4x4) without it, Cout % 128 == 0, Cin % 16 == 0 (plain and upsample + concat sources)"""
    return [l.index for l in unet_spec.UNET_LAYERS if algos0[l.index] == 4 and l.cout % 128 == 0 and l.cin % 16 == 0]


def _inputs(n, h, w):
    x = (torch.from_numpy(synthetic.hash_uniform(19, h * 100 + w, n * h * w).reshape(n, 1, h, w)) + 1) * 0.5
    return x, torch.linspace(5, 50, n) / 255.0


_RUNS = {}


def _run(sd_np, shape):
    """(per switch value: output, stages, conv_schedules, conv_algorithms) of one denoise at `shape`, computed once per module"""
    if shape not in _RUNS:
        n, h, w = shape
        x, sigma = _inputs(n, h, w)
        res = {}
        for cs in CS_VALUES:
            e = _engine(n, h, w, sd_np, cs)
            try:
                out = e.denoise(x.cuda(), sigma.cuda()).cpu()
                res[cs] = (out, [e.read_stage(k).cpu() for k in range(9)], e.conv_schedules(), e.conv_algorithms())
            finally:
                e.close()
        _RUNS[shape] = res
    return _RUNS[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_plan_takes_the_schedule_where_it_can(sd_np, shape):
    res = _run(sd_np, shape)
    _, _, sched2, algos2 = res[2]
    _, _, sched0, algos0 = res[0]
    want = _expected_layers(algos0)
    print(f"{shape}: cout-split layers {want}; schedules {sched2}")
    assert algos2 == algos0                                     # pnp_conv_algorithms keeps reporting 4 for these layers
    assert SCHED_COUT_SPLIT not in sched0
    assert [i for i, v in enumerate(sched2) if v == SCHED_COUT_SPLIT] == want
    assert all(s2 == s0 for i, (s2, s0) in enumerate(zip(sched2, sched0)) if i not in want)
    assert (len(want) == 0) == (shape in NO_F4_LEVEL), want


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_coutsplit_is_bit_identical_to_the_existing_schedules(sd_np, shape):
    res = _run(sd_np, shape)
    out2, st2, _, _ = res[2]
    out0, st0, _, _ = res[0]
    for which, (a, b) in enumerate(zip(st2, st0)):
        assert torch.equal(a, b), f"stage {which}: {int((a != b).sum())} of {a.numel()} elements differ, max {float((a - b).abs().max())}"
    assert torch.equal(out2, out0)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_coutsplit_matches_the_oracle_per_stage(sd_np, shape):
    n, h, w = shape
    out2, st2, _, _ = _run(sd_np, shape)[2]
    x, sigma = _inputs(n, h, w)
    noise_map = torch.ones(n, 1, h, w) * sigma.view(n, 1, 1, 1)
    ref_raw, stages = O.unet_forward(O.torch_weights(sd_np), torch.cat([x, noise_map], 1), return_stages=True)
    for which, (name, ref) in enumerate(stages.items()):
        err = float((st2[which] - ref).abs().max())
        print(f"{shape} stage {name}: max err {err:.3g} (bound {5e-5 * max(1.0, float(ref.abs().max())):.3g})")
        # FLOAT TOLERANCE: the bound of test_winograd_f4_path_matches_oracle_per_stage, unchanged
        assert err < 5e-5 * max(1.0, float(ref.abs().max())), f"stage {name}: max err {err}"
    np.testing.assert_allclose(out2.numpy(), torch.clamp(ref_raw, 0, 1).numpy(), rtol=0, atol=1e-5)


def test_a_stopped_slice_keeps_its_bits_and_the_live_ones_match(sd_np):
    """Two pnp_step calls at (3, 256, 256) with slice 1 stopped (done = [0, 1, 0]): its x, z, u keep their bits under the cout-split
    kernels (which skip a stopped slice's workgroups), the live slices equal the PNP_WINO_F4_CS=0 run bit for bit."""
    n, h, w = STEP_SHAPE
    data = synthetic.make_problem(n, h, w, accel=4.0, seed=911)
    st = O.reset(data)
    mu_tab, sig_tab = synthetic.param_table(n, 2, seed=77)
    tact = torch.tensor([0.0, 1.0, 0.0])
    got = {}
    for cs in (2, 0):
        e = _engine(n, h, w, sd_np, cs)
        try:
            assert (SCHED_COUT_SPLIT in e.conv_schedules()) == (cs == 2)
            x, z, u = e.reset(st["z"].cuda(), st["y0"].cuda(), st["mask"].reshape(h, w).cuda())
            x0, z0, u0 = x.clone(), z.clone(), u.clone()
            done = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            for t in range(2):
                e.step(x, z, u, torch.from_numpy(mu_tab[:, t]).cuda(), torch.from_numpy(sig_tab[:, t]).cuda(), t_action=tact.cuda(), done=done)
                assert done.tolist() == [0, 1, 0]
            for name, a, a0 in (("x", x, x0), ("z", z, z0), ("u", u, u0)):
                assert torch.equal(torch.view_as_real(a[1]) if a.is_complex() else a[1],
                                   torch.view_as_real(a0[1]) if a0.is_complex() else a0[1]), f"stopped slice: {name} moved"
                if name != "u":                             # (the check is not vacuous: the live slices did move)
                    assert not torch.equal(a[0], a0[0]), f"live slice: {name} did not move"
            got[cs] = [t.cpu() for t in (x, z, u)]
        finally:
            e.close()
    for name, a, b in zip("xzu", got[2], got[0]):
        for i in (0, 2):
            assert torch.equal(torch.view_as_real(a[i]) if a.is_complex() else a[i],
                               torch.view_as_real(b[i]) if b.is_complex() else b[i]), f"live slice {i}: {name} differs between the schedules"


@pytest.mark.parametrize("seed", P.SEEDS)
def test_dyadic_probe_weights_under_coutsplit(seed):
    """tests/probe_weights.py's `route` probe at (2, 128, 128), as test_gpu_probe.py runs it on F(4x4) (whose points +-3/4, +-3/2 are not
    exact in f32 products): within the suite's f32 bound AND equal to the float64-exact answer after rounding to the probe's grid
    (2^-4 for the stages, 2^-17 for the output) - and, the summation order being the same, the very bits of the PNP_WINO_F4_CS=0 handle."""
    n, h, w = PROBE_SHAPE
    sd = P.probe_state_dict("route", seed)
    x, sigma = P.probe_inputs(seed, n, h, w)
    ref_out, ref_stages = P.cached_reference("route", seed, n, h, w, "f32")
    res = {}
    for cs in (2, 0):
        e = _engine(n, h, w, sd, cs)
        try:
            assert (SCHED_COUT_SPLIT in e.conv_schedules()) == (cs == 2), e.conv_schedules()
            out = e.denoise(x.cuda(), sigma.cuda()).cpu()
            res[cs] = (out, {name: e.read_stage(k).cpu() for k, name in enumerate(P.STAGES)})
        finally:
            e.close()
    out, stages = res[2]
    for name, a in stages.items():
        ref = ref_stages[name]
        err = float((a - ref).abs().max())
        assert err < 5e-5 * max(1.0, float(ref.abs().max())), f"stage {name}: max err {err}"
        P.assert_same_bits(torch.round(a * 16) / 16, ref, f"cout-split route seed {seed} stage {name}, rounded to 2^-4")
        assert torch.equal(a, res[0][1][name]), f"stage {name} differs from the PNP_WINO_F4_CS=0 handle"
    np.testing.assert_allclose(out.numpy(), ref_out.numpy(), rtol=0, atol=1e-5)
    P.assert_same_bits(torch.round(out.double() * 2 ** 17) / 2 ** 17, ref_out, f"cout-split route seed {seed} output, rounded to 2^-17")
    assert torch.equal(out, res[0][0])
