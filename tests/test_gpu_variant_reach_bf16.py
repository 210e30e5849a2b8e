"""The bf16 conv kernel variants that a default BF16_CONVS handle plans and no older GPU test ran: the handles of
variant_cases.NEW_BF16_CASES - the `direct<... BF16=2 ...>` instantiations of conv_kernels.hip on the bf16 path (the two-block and split-K
tiles on small levels, POOL and upsample-concat sources, ragged grids) and the `ws<...>` forms of the producer / consumer kernel of
conv_bf16_kernels.hip (ragged in x / in y, the tile variants that need many thin slices) - each at DEFAULT tuning (no PNP_* variable), as
a production (BF16_CONVS) or a keep_stages (BF16_CONVS | KEEP_STAGES) handle, whichever the table names.
tests/test_variant_reach_host.py proves on the CPU that the table covers every variant key reachable at default tuning.

Per handle: (a) it is on the plan tests/plan_reach_host.cpp printed, with two weight terms and every 3x3 layer on a bf16 kernel; (b) dense
`unit_gain` weights against the oracle's bf16-operand mode with the bounds of test_bf16_convs_match_bf16_oracle_per_stage, and away from
the f32 oracle; (c) the dyadic probes `sum` and `lo` of tests/probe_weights.py bit for bit - all nine stages on a keep_stages handle, the
output and the stages still held in f32 (what feeds an upsample) on a production handle, whose other stages are bf16 or fused away;
(d) the batch reversed gives outputs (and kept stages) reversed, bit for bit, on the same handle.  (No new variant carries the fused last
layer - STEP_CASES below - so no handle here needs its own pnp_step run.)"""
import functools

import pytest
import torch

import probe_weights as P
import variant_cases as V
from dt4image_restoration_amd import weights
from test_gpu_probe import _read_stages
from test_gpu_variant_reach import _dense_inputs

pytestmark = pytest.mark.gpu

CASES = V.NEW_BF16_CASES
IDS = ["x".join(map(str, c[:3])) + ("-keep" if c[3] & V.KEEP_STAGES else "-prod") for c in CASES]
# The production entries with k-space-valid sides that run a new variant with a fused last layer would also run three pnp_step iterations
# against the oracle's bf16 mode (bound: the 3e-3 of test_512_accel8_bf16_convs_match_bf16_oracle).  There are none: every fused-last key a
# bf16 handle reaches is run by the older cases (tests/test_gpu_step_composition.py has the two epilogues inside pnp_step), and
# tests/test_variant_reach_host.py derives this list by that rule - it fails, and asks for the step test, once the rule names an entry.
STEP_CASES = []
PROBE_SEED = 0


@functools.lru_cache(maxsize=None)
def _dense_weights():
    return weights.generate_unet_weights(0, "unit_gain")


@pytest.fixture(scope="module")
def sd_np():
    return _dense_weights()


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(n, h, w, flags): Plan} of the table's handles, from the host tool"""
    exe = V.build_tool(str(tmp_path_factory.mktemp("reach")))
    cases = V.new_bf16_cases()
    return {(c.n, c.h, c.w, c.flags): p for c, p in zip(cases, V.plan_cases(exe, cases))}


def _engine(case, sd):
    from dt4image_restoration_amd.engine import PnPEngine
    n, h, w, flags = case
    assert flags & V.BF16_CONVS
    e = PnPEngine(n, h, w, keep_stages=bool(flags & V.KEEP_STAGES), bf16_convs=True)
    e.load_weights(sd)
    return e


def _label(case):
    return f"{case[0]}x{case[1]}x{case[2]} {'keep_stages' if case[3] & V.KEEP_STAGES else 'production'}"


@functools.lru_cache(maxsize=2)
def _dense_reference(n, h, w):
    """(clamped output, {stage: tensor}) of the bf16-operand oracle and the clamped output of the f32 oracle, eight slices at a time; the
    entries that differ in their flags alone stand side by side in the table and share it"""
    x, sigma = _dense_inputs(n, h, w)
    sd = _dense_weights()
    parts = [P.reference(sd, x[i:i + 8], sigma[i:i + 8], "bf16") for i in range(0, n, 8)]
    f32 = torch.cat([P.reference(sd, x[i:i + 8], sigma[i:i + 8], "f32")[0] for i in range(0, n, 8)])
    return torch.cat([p[0] for p in parts]), {k: torch.cat([p[1][k] for p in parts]) for k in P.STAGES}, f32


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_handle_is_on_the_plan_the_tool_printed(case, plans, sd_np):
    e = _engine(case, sd_np)
    try:
        plan = plans[case]
        assert e.conv_algorithms() == plan.families, (e.conv_algorithms(), plan.families)
        assert e.conv_schedules() == plan.schedules, (e.conv_schedules(), plan.schedules)
        assert e.bf16_weight_terms() == 2
        assert all(v in (0, 5) for v in e.conv_algorithms()[1:27])          # every 3x3 layer on a bf16 kernel (5: producer / consumer form)
    finally:
        e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dense_weights_match_the_bf16_oracle_and_the_reversed_batch(case, sd_np):
    n, h, w, flags = case
    keep = bool(flags & V.KEEP_STAGES)
    label = _label(case)
    x, sigma = _dense_inputs(n, h, w)
    ref_out, ref_stages, f32_out = _dense_reference(n, h, w)
    xg, sg = x.cuda(), sigma.cuda()
    e = _engine(case, sd_np)
    try:
        out = e.denoise(xg, sg)
        got = out.cpu()
        stages = {name: e.read_stage(which).cpu() for which, name in enumerate(P.STAGES)} if keep else {}
        for name, a in stages.items():
            ref = ref_stages[name]
            assert a.shape == ref.shape, name
            sc = float(ref.abs().max())
            emax, emean = float((a - ref).abs().max()), float((a - ref).abs().mean())
            print(f"{label} stage {name}: max err {emax:.3g} (bound {3e-2 * sc:.3g}), mean err {emean:.3g} (bound {2e-3 * sc:.3g})")
            # FLOAT TOLERANCE: the per-stage bounds of test_bf16_convs_match_bf16_oracle_per_stage, unchanged
            assert emax < 3e-2 * sc, f"{label} stage {name}: max err {emax}"
            assert emean < 2e-3 * sc, f"{label} stage {name}: mean err {emean}"
        err, off = float((got - ref_out).abs().max()), float((got - f32_out).abs().max())
        print(f"{label} output: max err {err:.3g} against the bf16 oracle, {off:.3g} away from the f32 oracle")
        assert err < 2e-3, f"{label} output: max err {err}"          # (the same test's output bound)
        assert off > 2e-5, f"{label}: the output is the f32 arithmetic's"          # (and its check that the mode is on)
        assert float((out - xg).abs().max()) > 1e-3                # the network did something
        # the same handle - the same plan - on the batch reversed: slice i's bits at position n - 1 - i
        rev = e.denoise(xg.flip(0).contiguous(), sg.flip(0).contiguous())
        assert torch.equal(rev.flip(0), out), f"{label}: reversed batch differs in {int((rev.flip(0) != out).sum())} elements"
        for which, name in enumerate(P.STAGES if keep else ()):
            assert torch.equal(e.read_stage(which).cpu().flip(0), stages[name]), f"{label}: reversed batch, stage {name}"
    finally:
        e.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probes_are_exact(case):
    """`sum` (accumulation, bf16 rounding of activations with more than 8 bits) and `lo` (weights that need both bf16 terms, either sign of
    the second).  Exactness is derived, not assumed: the widest partial sum of every conv layer fits 24 bits.  The read-out layer of `lo` does
    not (29 bits, at every shape: a 24-bit value times 2^-6 plus image and bias), which is why probe_weights compares that probe's output
    within LO_OUT_BOUND, two f32 roundings - the rule of test_probe_is_bit_exact, taken over with it."""
    n, h, w, flags = case
    keep = bool(flags & V.KEEP_STAGES)
    x, sigma = P.probe_inputs(PROBE_SEED, n, h, w)
    xg, sg = x.cuda(), sigma.cuda()
    compared = 0
    for probe in ("sum", "lo"):
        sd = P.probe_state_dict(probe, PROBE_SEED)
        assert max(P.bit_budget(sd, "bf16", (n, h, w))[:27 if probe == "lo" else 28]) <= 24
        ref_out, ref_stages = P.cached_reference(probe, PROBE_SEED, n, h, w, "bf16")
        e = _engine(case, sd)
        try:
            out = e.denoise(xg, sg).cpu()
            stages = _read_stages(e, keep)
            assert len(stages) == 9 or not keep
            compared += P.assert_probe_result(out, stages, ref_out, ref_stages, probe, f"{probe} {_label(case)}")
        finally:
            e.close()
    print(f"{_label(case)}: {compared} elements compared bit for bit")
