"""The conv kernel variants that a default handle plans and no older GPU test ran: the shapes of variant_cases.NEW_SHAPES - many slices of
thin or tiny images, where the plan takes the full-size unsplit direct tiles on 1 x 1 ... 8 x 8 pixel levels, the Cout = 32 LDS-epilogue
tile on a 16-wide level 0, F(2x2) pooling while it stages, and the F(4x4) edge forms that need a large batch - each at DEFAULT tuning (no
PNP_* variable), on a keep_stages and a production handle.  tests/test_variant_reach_host.py proves on the CPU that the list covers every
variant key reachable at default tuning.

Per shape: (a) the handle is on the plan tests/plan_reach_host.cpp printed; (b) dense `unit_gain` weights against the oracle, per stage,
with the suite's bounds; (c) the dyadic probes of tests/probe_weights.py - `sum` and `route` bit for bit where no launch is on F(4x4),
`route` under test_gpu_probe's F(4x4) rule where one is; (d) the batch reversed gives the outputs reversed, bit for bit, on the same
handle; (e) for the shapes whose new variant carries a fused first or last layer and whose sides the k-space stage accepts, three
pnp_step iterations against the oracle with one slice stopped."""
import numpy as np
import pytest
import torch

import probe_weights as P
import variant_cases as V
from dt4image_restoration_amd import synthetic, weights
from oracle import pnp_oracle as O
from test_gpu_probe import _check_f4, _read_stages

pytestmark = pytest.mark.gpu

SHAPES = V.NEW_SHAPES
IDS = ["x".join(map(str, s)) for s in SHAPES]
# (tests/test_variant_reach_host.py: the k-space-valid shapes whose production handle runs a new variant with a fused first or last layer)
STEP_SHAPES = [(7, 320, 16), (8, 16, 400), (64, 80, 16)]
STEP_ATOL = 2e-5           # FLOAT TOLERANCE: the trajectory bound of test_batch_semantics_deterministic_and_permutation_invariant (3 iterations, f32)
PROBE_SEED = 0


@pytest.fixture(scope="module")
def sd_np():
    return weights.generate_unet_weights(0, "unit_gain")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(n, h, w, flags): Plan} of the new cases, from the host tool"""
    exe = V.build_tool(str(tmp_path_factory.mktemp("reach")))
    cases = V.new_cases()
    return {(c.n, c.h, c.w, c.flags): p for c, p in zip(cases, V.plan_cases(exe, cases))}


def _engine(shape, keep_stages, sd):
    from dt4image_restoration_amd.engine import PnPEngine
    e = PnPEngine(*shape, keep_stages=keep_stages)
    e.load_weights(sd)
    return e


def _dense_inputs(n, h, w):
    x = (torch.from_numpy(synthetic.hash_uniform(29, h * 1031 + w, n * h * w).reshape(n, 1, h, w)) + 1) * 0.5
    return x, torch.linspace(5, 50, n) / 255.0


def _dense_reference(sd_np, n, h, w):
    """(clamped output, {stage: tensor}) of the f32 oracle, eight slices at a time"""
    x, sigma = _dense_inputs(n, h, w)
    parts = [P.reference(sd_np, x[i:i + 8], sigma[i:i + 8]) for i in range(0, n, 8)]
    return torch.cat([p[0] for p in parts]), {k: torch.cat([p[1][k] for p in parts]) for k in P.STAGES}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_handle_is_on_the_plan_the_tool_printed(shape, plans, sd_np):
    for flags in V.NEW_FLAGS:
        e = _engine(shape, flags == V.KEEP_STAGES, sd_np)
        try:
            plan = plans[shape + (flags,)]
            assert e.conv_algorithms() == plan.families, (flags, e.conv_algorithms(), plan.families)
            assert e.conv_schedules() == plan.schedules, (flags, e.conv_schedules(), plan.schedules)
            assert e.bf16_weight_terms() == 0
        finally:
            e.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dense_weights_match_the_oracle_and_the_reversed_batch(shape, sd_np):
    n, h, w = shape
    x, sigma = _dense_inputs(n, h, w)
    ref_out, ref_stages = _dense_reference(sd_np, n, h, w)
    xg, sg = x.cuda(), sigma.cuda()
    for flags in V.NEW_FLAGS:
        keep = flags == V.KEEP_STAGES
        label = f"{n}x{h}x{w} {'keep_stages' if keep else 'production'}"
        e = _engine(shape, keep, sd_np)
        try:
            out = e.denoise(xg, sg)
            stages = _read_stages(e, keep)
            assert len(stages) == 9 or not keep
            for name, a in stages.items():
                ref = ref_stages[name]
                assert a.shape == ref.shape, name
                err = float((a - ref).abs().max())
                print(f"{label} stage {name}: max err {err:.3g} (bound {5e-5 * max(1.0, float(ref.abs().max())):.3g})")
                # FLOAT TOLERANCE: the per-stage bound of test_denoiser_matches_oracle_per_stage, unchanged
                assert err < 5e-5 * max(1.0, float(ref.abs().max())), f"{label} stage {name}: max err {err}"
            print(f"{label} output: max err {float((out.cpu() - ref_out).abs().max()):.3g}")
            np.testing.assert_allclose(out.cpu().numpy(), ref_out.numpy(), rtol=0, atol=1e-5)
            assert float((out - xg).abs().max()) > 1e-3                # the network did something
            # the same handle - the same plan - on the batch reversed: slice i's bits at position n - 1 - i
            rev = e.denoise(xg.flip(0).contiguous(), sg.flip(0).contiguous())
            assert torch.equal(rev.flip(0), out), f"{label}: reversed batch differs in {int((rev.flip(0) != out).sum())} elements"
            if keep:
                for which, name in enumerate(P.STAGES):
                    assert torch.equal(e.read_stage(which).cpu().flip(0), stages[name]), f"{label}: reversed batch, stage {name}"
        finally:
            e.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_probes_are_exact(shape):
    n, h, w = shape
    x, sigma = P.probe_inputs(PROBE_SEED, n, h, w)
    xg, sg = x.cuda(), sigma.cuda()
    compared = 0
    for probe in ("route", "sum"):
        sd = P.probe_state_dict(probe, PROBE_SEED)
        ref = None
        for flags in V.NEW_FLAGS:
            keep = flags == V.KEEP_STAGES
            label = f"{probe} {n}x{h}x{w} {'keep_stages' if keep else 'production'}"
            e = _engine(shape, keep, sd)
            try:
                algos = e.conv_algorithms()
                if 4 in algos and probe != "route":
                    continue                                        # F(4x4)'s points are not exact: `route` under its own rule
                if ref is None:
                    ref = P.cached_reference(probe, PROBE_SEED, n, h, w, "f32")
                out = e.denoise(xg, sg).cpu()
                stages = _read_stages(e, keep)
                if 4 in algos:
                    _check_f4(out, stages, ref[0], ref[1], label)
                else:
                    assert max(P.bit_budget(sd, "wino2" if 1 in algos else "f32", shape)) <= 24
                    compared += P.assert_probe_result(out, stages, ref[0], ref[1], probe, label)
            finally:
                e.close()
    print(f"{n}x{h}x{w}: {compared} elements compared bit for bit")


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=["x".join(map(str, s)) for s in STEP_SHAPES])
def test_three_steps_match_the_oracle_with_a_stopped_slice(shape, sd_np):
    """The production handle's fused first / last layer inside pnp_step: the image channel is Re(z - u), and slice 1, stopped by t_action
    from the second iteration on, keeps its bits."""
    n, h, w = shape
    iters = 3
    data = synthetic.make_problem(n, h, w, accel=4.0, seed=700 + h + w)
    mu_tab, sig_tab = synthetic.param_table(n, iters, seed=77)
    sd = O.torch_weights(sd_np)
    st = O.reset(data)
    e = _engine(shape, False, sd_np)
    try:
        x, z, u = e.reset(st["z"].cuda(), st["y0"].cuda(), st["mask"].reshape(h, w).cuda())
        frozen = None
        for t in range(iters):
            tact = torch.zeros(n)
            if t >= 1:
                tact[1] = 1.0
            mu, sg = torch.from_numpy(mu_tab[:, t].copy()), torch.from_numpy(sig_tab[:, t].copy())
            st, _ = O.admm_step(sd, st, mu, sg, tact)
            live = x[0].clone()
            e.step(x, z, u, mu.cuda(), sg.cuda(), t_action=tact.cuda())
            for name, got, ref in (("x", x, st["x"]), ("z", z, st["z"]), ("u", u, st["u"])):
                d = got.cpu() - ref
                err = float((torch.view_as_real(d) if d.is_complex() else d).abs().max())
                print(f"{n}x{h}x{w} iteration {t} {name}: max err {err:.3g}")
                assert err < STEP_ATOL, (t, name, err)
            if t == 0:
                frozen = [v[1].clone() for v in (x, z, u)]
            else:
                assert all(torch.equal(a[1], b) for a, b in zip((x, z, u), frozen)), t
            assert not torch.equal(x[0], live)                        # (not vacuous: a live slice moved)
    finally:
        e.close()
