"""Every conv kernel variant a default handle can plan is run by the GPU suite (no GPU): tests/plan_reach_host.cpp, linked against the
built library, names the variant of every launch of every case of tests/variant_cases.py and enumerates the variants reachable at default
tuning (H, W multiples of 16 up to 1024, N up to 256, N H W <= 64 x 256 x 256, flags 0 / BF16_CONVS / KEEP_STAGES / both).  The number of
reachable-but-unrun keys allowed is zero, at the template level and at the edge level.  A plan change that routes a default handle to an
instantiation no GPU test runs fails here, with the key and the smallest handle that reaches it."""
import pytest

import variant_cases as V
from test_gpu_sizes import kspace_len_ok


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = V.build_tool(str(tmp_path_factory.mktemp("reach")))
    template, edge, summary = V.reach(exe)
    print(summary)
    existing, new = V.existing_cases(), V.new_cases()
    return {"T": template, "E": edge, "existing": V.plan_cases(exe, existing), "new": V.plan_cases(exe, new), "new_cases": new}


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
    for plans in (tool["existing"], tool["new"]):
        assert not [k for k in _keys(plans, "T") if k.startswith("INVALID")]


@pytest.mark.parametrize("level", ["T", "E"], ids=["template", "edge"])
def test_every_reachable_variant_is_run_by_some_case(tool, level):
    missing = _unrun(tool, level, tool["existing"] + tool["new"])
    print(_report(tool, level, missing))
    assert not missing, _report(tool, level, missing)


@pytest.mark.parametrize("level", ["T", "E"], ids=["template", "edge"])
def test_the_older_cases_alone_leave_variants_out(tool, level):
    """what tests/test_gpu_variant_reach.py is for: without its cases the check above fails (the report it would print is printed here)"""
    missing = _unrun(tool, level, tool["existing"])
    print(_report(tool, level, missing))
    assert missing


def test_every_new_shape_adds_a_variant_and_the_step_shapes_follow_their_rule(tool):
    """Every shape of NEW_SHAPES runs an edge-level key that the older cases leave out, all at default tuning.
    STEP_SHAPES of the GPU test: the k-space-valid shapes whose production handle runs, with a fused first or last layer, a key the older
    cases leave out."""
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
