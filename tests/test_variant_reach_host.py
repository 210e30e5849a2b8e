"""Every conv kernel variant a default handle can plan is run by the GPU suite (no GPU): tests/plan_reach_host.cpp, linked against the
built library, names the variant of every launch of every case of tests/variant_cases.py and enumerates the variants reachable at default
tuning (H, W multiples of 16 up to 1024, N up to 256, N H W <= 64 x 256 x 256, flags 0 / BF16_CONVS / KEEP_STAGES / both).  The number of
reachable-but-unrun keys allowed is zero, at the template level and at the edge level.  A plan change that routes a default handle to an
instantiation no GPU test runs fails here, with the key and the smallest handle that reaches it."""
from collections import Counter

import pytest

import variant_cases as V
from test_gpu_sizes import kspace_len_ok


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = V.build_tool(str(tmp_path_factory.mktemp("reach")))
    template, edge, summary, only, by = V.reach(exe)
    print(summary)
    print("keys reached by handles of one flag set alone:", only)
    existing, new, bf16 = V.existing_cases(), V.new_cases(), V.new_bf16_cases()
    return {"T": template, "E": edge, "only": only, "by": by, "existing": V.plan_cases(exe, existing), "new": V.plan_cases(exe, new), "new_cases": new,
            "bf16": V.plan_cases(exe, bf16), "bf16_cases": bf16}


def _keys(plans, level):
    return {k for p in plans for k in (p.template if level == "T" else p.edge)}


def _unrun(tool, level, plans):
    run = _keys(plans, level)
    return sorted(k for k in tool[level] if k not in run)


def _report(tool, level, missing):
    name = {"T": "template", "E": "edge"}[level]
    lines = [f"{name} level: {len(tool[level])} keys reachable at default tuning, {len(missing)} run by no case"]
    for k in missing:
        at, kat = tool[level][k]
        lines.append(f"  {k}\n      smallest handle n h w flags = {at}; with k-space-valid sides: {kat if kat else 'none'}")
    return "\n".join(lines)


def test_no_plan_record_is_refused_by_its_dispatcher(tool):
    """the tool restates the four dispatchers: a record none of their branches accepts would be a launch error on the GPU"""
    for level in "TE":
        assert not [k for k in tool[level] if k.startswith("INVALID")]
    for plans in (tool["existing"], tool["new"], tool["bf16"]):
        assert not [k for k in _keys(plans, "T") if k.startswith("INVALID")]


@pytest.mark.parametrize("level", ["T", "E"], ids=["template", "edge"])
def test_every_reachable_variant_is_run_by_some_case(tool, level):
    missing = _unrun(tool, level, tool["existing"] + tool["new"] + tool["bf16"])
    print(_report(tool, level, missing))
    assert not missing, _report(tool, level, missing)


@pytest.mark.parametrize("level", ["T", "E"], ids=["template", "edge"])
def test_the_reach_holds_every_flag_set_and_both_bf16_kernels(tool, level):
    """The enumeration once wrote its flags into pnp_config.device: every handle was an f32 production one, every key was reached by all
    four "flag sets" alike, and "zero unrun" spoke about a part of what it claimed.  So: the flag sets 0, BF16_CONVS and BF16_CONVS |
    KEEP_STAGES each reach a key that no other flag set reaches (8 / 31 / 18 template keys, 13 / 89 / 53 edge keys).  KEEP_STAGES by
    itself cannot: a keep_stages f32 handle has no fused first or last layer and no pooled epilogue, and every launch it is left with is
    one an f32 production handle of some size plans too (94 / 228 keys are shared by exactly these two) - except the last layer's own
    kernel, which only a handle with the KEEP_STAGES bit launches.  Its share of the guard is therefore a key that the KEEP_STAGES
    handles reach and no handle without that bit does.  And the kernels only a bf16 handle plans are in the reach."""
    K, B = V.KEEP_STAGES, V.BF16_CONVS
    only, by = tool["only"][level], tool["by"][level]
    print(level, "keys per set of reaching flag sets:", sorted(((sorted(k), n) for k, n in Counter(by.values()).items())))
    assert sorted(only) == sorted([0, K, B, B | K]), only
    assert only == {f: sum(1 for v in by.values() if v == {f}) for f in only}          # the tool's counts are the counts of its own lines
    for flags in (0, B, B | K):
        assert only[flags] >= 1, f"no {level} key is reached by handles of flags {flags} alone: {only}"
    assert [k for k, v in by.items() if K in v and v <= {K, B | K}], f"no {level} key needs the KEEP_STAGES bit"
    assert any(k.startswith("ws<") for k in tool[level])
    assert any(k.startswith("direct<") and "BF16=2" in k for k in tool[level])


@pytest.mark.parametrize("level", ["T", "E"], ids=["template", "edge"])
def test_the_older_cases_alone_leave_variants_out(tool, level):
    """what tests/test_gpu_variant_reach.py is for: without its cases the check above fails (the report it would print is printed here)"""
    missing = _unrun(tool, level, tool["existing"])
    print(_report(tool, level, missing))
    assert missing


def test_every_new_shape_adds_a_variant_and_the_step_shapes_follow_their_rule(tool):
    """Every shape of NEW_SHAPES runs an edge-level key that the older cases leave out, all at default tuning.
    STEP_SHAPES of the GPU test: the k-space-valid shapes whose production handle runs, with a fused first or last layer, a key the older
    cases leave out.  NEW_BF16_CASES and the bf16 GPU test's STEP_CASES: the function below."""
    import test_gpu_variant_reach as G
    old = _keys(tool["existing"], "E")
    own = {}
    for case, plan in zip(tool["new_cases"], tool["new"]):
        assert case.env == ()
        own.setdefault((case.n, case.h, case.w), set()).update(k for k in plan.edge if k in tool["E"] and k not in old)
    assert list(own) == V.NEW_SHAPES
    for shape, keys in own.items():
        others = set().union(*[v for s, v in own.items() if s != shape])
        print(f"{shape}: {len(keys)} keys the older cases leave out, {len(keys - others)} of them run by no other new shape")
    # (the set cover is greedy, not minimal: a shape may stay for a k-space-valid run of keys a refused size also covers)
    assert all(keys for keys in own.values())
    step = []
    for case, plan in zip(tool["new_cases"], tool["new"]):
        fused = [k for k in plan.edge if k not in old and (" first" in k or " last" in k)]
        if case.flags == 0 and fused and kspace_len_ok(case.h) and kspace_len_ok(case.w):
            step.append((case.n, case.h, case.w))
    assert step == G.STEP_SHAPES
    _the_bf16_table_follows_the_same_rules(tool)


def _the_bf16_table_follows_the_same_rules(tool):
    """The bf16 analogue: every entry of NEW_BF16_CASES, a bf16 handle at default tuning, runs an edge-level key that the older cases, NEW_SHAPES
    and the entries before it leave out.  STEP_CASES of the bf16 GPU test: the production entries with k-space-valid sides that run, with
    a fused last layer, a key the older cases and NEW_SHAPES leave out."""
    import test_gpu_variant_reach_bf16 as GB
    assert [(c.n, c.h, c.w, c.flags) for c in tool["bf16_cases"]] == V.NEW_BF16_CASES
    assert len(set(V.NEW_BF16_CASES)) == len(V.NEW_BF16_CASES)
    old = _keys(tool["existing"] + tool["new"], "E")
    seen, step = set(old), []
    for case, plan in zip(tool["bf16_cases"], tool["bf16"]):
        assert case.env == () and case.flags in (V.BF16_CONVS, V.BF16_CONVS | V.KEEP_STAGES)
        adds = {k for k in plan.edge if k in tool["E"] and k not in seen}
        print(f"{(case.n, case.h, case.w, case.flags)}: {len(adds)} keys that everything before it leaves out")
        assert adds, case
        seen |= adds
        fused = [k for k in plan.edge if k not in old and " last" in k]
        if case.flags == V.BF16_CONVS and fused and kspace_len_ok(case.h) and kspace_len_ok(case.w):
            step.append((case.n, case.h, case.w, case.flags))
    assert step == GB.STEP_CASES
