"""One table of the denoiser handles the GPU suite compares with the oracle or with the dyadic probes (no test in here).

A case is (n, h, w, handle flags, env tuning, where it comes from).  tests/plan_reach_host.cpp turns a case into the variant key of each of
its launches - kernel family, template arguments, the runtime switches that select code; at the edge level also "tile grid ragged in x / in
y" and "stacked F(4x4) launch with odd N" - and enumerates which keys a handle at DEFAULT tuning can reach (its header states the range).
tests/test_variant_reach_host.py requires that every reachable key, at both levels, is run by some case below: zero reachable-but-unrun keys.

The existing tests' cases are assembled from the parameter lists those tests use themselves (imported, not copied):
  test_gpu_kernels         per-stage, F(2x2), F(4x4) x schedule, bf16 per-stage, the shape sweep x mode, the fused first / last pair
  test_gpu_probe           probe_weights.MATRIX rows (keep_stages up to KEEP_MAX_N slices + production), the clamp, the last-bias paths
  test_gpu_sizes           DENOISER_SHAPES x mode, the 1024 x 1024 stages, STEP_SHAPES
  test_gpu_wino4_coutsplit SHAPES under both PNP_WINO_F4_CS values, its probe and step shapes
(Tests that compare two handles with each other, a golden file or a PSNR series only are not in the table: they cannot tell a variant
that is wrong in both.  The switches a test sets inside its body, such as PNP_WINO_MIN_BLOCKS=1 in the F(4x4) test, are restated here.)
NEW_SHAPES are the shapes of tests/test_gpu_variant_reach.py: default tuning, chosen - greedy set cover by N H W over the handles of the
tool's --reach range, k-space-valid sides preferred - to run every key the existing cases leave out.
NEW_BF16_CASES are the handles of tests/test_gpu_variant_reach_bf16.py: the bf16 variants (conv_kernels.hip with BF16=2 and the `ws`
producer / consumer kernel of conv_bf16_kernels.hip) that everything above leaves out, chosen the same way over the BF16_CONVS and
BF16_CONVS | KEEP_STAGES handles of the range."""
from __future__ import annotations

from collections import namedtuple

KEEP_STAGES, BF16_CONVS = 4, 8                       # PNP_FLAG_KEEP_STAGES, PNP_FLAG_BF16_CONVS (include/pnpadmm.h)

Case = namedtuple("Case", "n h w flags env source")

# The shapes of tests/test_gpu_variant_reach.py; each runs a keep_stages and a production handle at default tuning (no PNP_* variable).
# A literal list on purpose: tests/test_variant_reach_host.py proves that it still covers.
NEW_SHAPES = [
    (1, 16, 256), (128, 16, 16), (7, 320, 16), (64, 16, 48), (8, 16, 400), (128, 16, 32), (64, 80, 16), (32, 16, 160), (12, 592, 16),
    (48, 16, 160), (2, 400, 160), (5, 320, 80), (64, 16, 128), (48, 64, 48), (24, 320, 32), (96, 16, 160), (48, 16, 320), (64, 16, 256),
    (7, 128, 320), (8, 400, 128), (16, 400, 64), (3, 592, 272), (64, 128, 80), (6, 592, 256), (96, 80, 128), (128, 128, 64), (24, 160, 320),
]
NEW_FLAGS = (KEEP_STAGES, 0)

# The handles (n, h, w, flags) of tests/test_gpu_variant_reach_bf16.py, default tuning.  Greedy set cover over ALL bf16 handles of the reach
# range (not each key's smallest alone): first the keys some k-space-valid handle reaches, over those handles, then the rest over all; a
# handle's worth is the unrun edge keys it adds per N H W + 300,000 pixels (the constant: what a case costs whatever its size); last, an entry
# whose keys the others run between them is dropped, so each entry runs a key no other entry does.  Sorted by N H W.
_B, _BK = BF16_CONVS, BF16_CONVS | KEEP_STAGES
NEW_BF16_CASES = [
    (1, 16, 128, _B), (128, 16, 16, _B), (64, 16, 48, _B), (96, 16, 48, _B), (192, 16, 32, _BK), (3, 512, 80, _B), (128, 16, 64, _B),
    (3, 1024, 48, _B), (96, 112, 16, _B), (6, 1024, 32, _B), (12, 1024, 16, _B), (192, 16, 64, _B), (4, 1024, 48, _B), (96, 16, 160, _BK),
    (48, 32, 160, _B), (4, 400, 160, _B), (48, 112, 48, _BK), (128, 16, 128, _B), (8, 1024, 32, _B), (16, 1024, 16, _B), (6, 1024, 48, _B),
    (6, 1024, 48, _BK), (24, 400, 32, _B), (24, 16, 800, _B), (32, 64, 160, _B), (96, 112, 32, _B), (24, 112, 144, _B), (12, 1024, 32, _B),
    (192, 16, 128, _BK), (6, 1024, 64, _B), (8, 80, 640, _B), (3, 1024, 160, _B), (6, 1024, 80, _B), (6, 1024, 80, _BK), (48, 64, 160, _B),
    (16, 1024, 32, _BK), (8, 1024, 64, _B), (4, 1024, 160, _BK), (48, 112, 128, _B), (12, 112, 528, _B), (12, 1024, 64, _BK),
    (12, 1024, 64, _B), (12, 112, 1024, _B),
]


def _case(shape, flags, env, source):
    n, h, w = shape
    return Case(n, h, w, flags, tuple(sorted(env.items())), source)


def existing_cases():
    import probe_weights as P
    import test_gpu_kernels as K
    import test_gpu_probe as GP
    import test_gpu_sizes as S
    import test_gpu_wino4_coutsplit as CS

    out = []
    for shape in K._PER_STAGE_SHAPES:                                   # test_denoiser_matches_oracle_per_stage: keep_stages, then production
        out += [_case(shape, KEEP_STAGES, {}, "kernels.per_stage"), _case(shape, 0, {}, "kernels.per_stage")]
    for shape in K._WINO2_SHAPES:                                       # test_winograd_path_matches_oracle_per_stage
        env = {"PNP_NO_WINO_F4": "1"}
        if shape[0] < 64:
            env["PNP_WINO_MIN_BLOCKS"] = "1"
        out.append(_case(shape, KEEP_STAGES, env, "kernels.wino2"))
    for n, h, w, min_cin in K._F4_SHAPES:                               # test_winograd_f4_path_matches_oracle_per_stage
        for schedule, senv in K._F4_SCHEDULE_ENV.items():
            env = dict(senv, PNP_WINO_MIN_BLOCKS="1", PNP_WINO_F4_MIN_CIN=str(min_cin))
            out.append(_case((n, h, w), KEEP_STAGES, env, f"kernels.f4[{schedule}]"))
    for shape in K._BF16_SHAPES:                                        # test_bf16_convs_match_bf16_oracle_per_stage
        out.append(_case(shape, KEEP_STAGES | BF16_CONVS, {}, "kernels.bf16"))
    for shape in K._SWEEP:                                              # test_denoiser_shape_sweep
        for mode, env in K._SWEEP_MODE_ENV.items():
            out.append(_case(shape, BF16_CONVS if mode == "bf16" else 0, env, f"kernels.sweep[{mode}]"))
    out += [_case(K._FUSED_SHAPE, 0, {}, "kernels.fused"), _case(K._FUSED_SHAPE, 0, K._UNFUSED_ENV, "kernels.unfused")]

    for row, (_, _, bf16, env, _, shapes) in P.MATRIX.items():          # test_probe_is_bit_exact
        for shape in shapes:
            env_n = {k: v for k, v in env.items() if not (k == "PNP_WINO_MIN_BLOCKS" and shape[0] >= 64)}
            for keep in ((True, False) if shape[0] <= GP.KEEP_MAX_N else (False,)):
                out.append(_case(shape, (KEEP_STAGES if keep else 0) | (BF16_CONVS if bf16 else 0), env_n, f"probe.{row}"))
    for bf16, env in GP.CLAMP_ENV.items():                              # test_probe_clamp_is_exact
        for keep in (False, True):
            out.append(_case(GP.CLAMP_SHAPE, (KEEP_STAGES if keep else 0) | (BF16_CONVS if bf16 else 0), env, "probe.clamp"))
    for name, bf16, env, shape, _ in GP._BIAS_PATHS:                    # test_dense_weights_with_nonzero_last_bias
        out.append(_case(shape, BF16_CONVS if bf16 else 0, env, f"probe.bias[{name}]"))

    for shape in S.DENOISER_SHAPES:                                     # test_denoiser_at_large_and_extreme_sides
        for mode, env in S.DENOISER_MODE_ENV.items():
            out.append(_case(shape, BF16_CONVS if mode == "bf16" else 0, env, f"sizes.denoiser[{mode}]"))
    out.append(_case(S.STAGES_SHAPE, KEEP_STAGES, {}, "sizes.stages"))
    for shape in S.STEP_SHAPES:                                         # test_step_at_the_corners_of_the_size_range
        out.append(_case(shape, 0, {}, "sizes.step"))

    for cs in CS.CS_VALUES:                                             # tests/test_gpu_wino4_coutsplit.py: every handle is keep_stages
        env = dict(CS.ENV, PNP_WINO_F4_CS=str(cs))
        for shape in CS.SHAPES + [CS.PROBE_SHAPE, CS.STEP_SHAPE]:
            out.append(_case(shape, KEEP_STAGES, env, f"coutsplit[{cs}]"))
    return out


def new_cases():
    return [_case(shape, flags, {}, "variant_reach") for shape in NEW_SHAPES for flags in NEW_FLAGS]


def new_bf16_cases():
    return [_case((n, h, w), flags, {}, "variant_reach_bf16") for n, h, w, flags in NEW_BF16_CASES]


def all_cases():
    return existing_cases() + new_cases() + new_bf16_cases()


def describe(case) -> str:
    """the line tests/plan_reach_host.cpp reads for a case"""
    return " ".join([str(case.n), str(case.h), str(case.w), str(case.flags)] + [f"{k}={v}" for k, v in case.env])


# ---- running tests/plan_reach_host.cpp -------------------------------------------------------------------------------------------------
def build_tool(workdir: str) -> str:
    """compile the tool against the built library (as tests/test_wino4_coutsplit_plan_host.py does); pytest.skip without hipcc / make"""
    import os
    import shutil
    import subprocess

    import pytest
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "dt4image_restoration_amd", "csrc")
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) or shutil.which("make") is None:
        pytest.skip("no hipcc / make")
    if not os.path.exists(os.path.join(csrc, "libpnpadmm.so")):
        subprocess.run(["make", "-C", csrc, "-j", "4"], check=True, capture_output=True)
    exe = os.path.join(workdir, "plan_reach_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", os.path.join(root, "tests", "plan_reach_host.cpp"), "-o", exe,
                    "-L" + csrc, "-lpnpadmm", "-Wl,-rpath," + csrc], check=True, capture_output=True)
    return exe


def _run(exe, args, stdin=""):
    import os
    import subprocess
    env = {k: v for k, v in os.environ.items() if not k.startswith("PNP_")}
    r = subprocess.run([exe] + args, input=stdin, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


Plan = namedtuple("Plan", "families schedules layers template edge")     # layers / template / edge: one entry per launch record


def plan_cases(exe, cases):
    """[Plan] of `cases`, in order, as the tool prints them"""
    out = _run(exe, [], "".join(describe(c) + "\n" for c in cases))
    plans = {}
    for line in out.splitlines():
        word, idx, rest = line.split(" ", 2)
        assert word != "refused", line
        if word == "plan":
            fam, sched = (field.split("=")[1] for field in rest.split(" "))
            plans[int(idx)] = Plan([int(v) for v in fam.split(",")], [int(v) for v in sched.split(",")], [], [], [])
        else:
            layer, template, edge = rest.split(" | ")
            p = plans[int(idx)]
            p.layers.append(int(layer.split("=")[1]))
            p.template.append(template)
            p.edge.append(edge)
    assert sorted(plans) == list(range(len(cases))), out[-2000:]
    return [plans[i] for i in range(len(cases))]


def reach(exe):
    """({template key: (smallest handle, smallest k-space-valid handle or None)}, the same for edge keys, the tool's summary line,
    {level: {flags: number of keys that handles of this flag set alone reach}}, {level: {key: the flag sets whose handles reach it}});
    a handle is (n, h, w, flags)"""
    out = _run(exe, ["--reach"]).splitlines()
    levels = {"T": {}, "E": {}}
    only, reached_by = {"T": {}, "E": {}}, {"T": {}, "E": {}}
    for line in out[:-1]:
        head, rest = line.split(" | ", 1)
        word, level = head.split()
        if word == "only":
            flags, count = rest.split(" | ")
            only[level][int(flags)] = int(count)
            continue
        assert word == "reach", line
        key, at, kat, by = rest.split(" | ")
        levels[level][key] = (tuple(int(v) for v in at.split()), None if kat == "-" else tuple(int(v) for v in kat.split()))
        reached_by[level][key] = frozenset(int(v) for v in by.split())
    return levels["T"], levels["E"], out[-1], only, reached_by
