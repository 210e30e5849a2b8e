#!/usr/bin/env python3
"""Timing of the off-resonance operator and stage on the GPU (not a test): 64 slices of 256 x 256 on a 320 x 320 grid, a spiral of 16
interleaves, J = 6, a field map of 100 Hz and a readout of 10 ms, once with the number of time segments `acquisition.offres_segments` asks
for at tol = 1e-3 (capped at the library's 32) and once with L = 8.  Per L two handles of the same shape - the two-segment gather and
gridding (PNP_OFFRES_NAIVE=0) and the naive form (PNP_OFFRES_NAIVE=1: the non-Cartesian SENSE launches on all L planes between a blend and
an expansion kernel) - the shipped choice per step (unset), and the two-segment form with the gridding's other layout (PNP_OFFRES_GRID_FILTER=1:
every segment's workgroup filters the tile's whole bin instead of walking the plan's per-(segment, tile) list) are timed in alternating order, device events around `reps` back-to-back
calls after a warm-up, `rounds` times; the median of the rounds is reported with their spread.  Per form: pnp_offres_forward,
pnp_offres_adjoint, pnp_offres_normal (the cost of one CG iteration) and a whole pnp_step (K CG iterations, TV prior).  The plain
non-Cartesian stage on the same handle stands beside them: pnp_nufft_forward, pnp_nufft_adjoint, pnp_nc_normal and its pnp_step.
Writes profiles/offres_bench.json and prints it."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dt4image_restoration_amd import acquisition, synthetic  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402

NAIVE_ENV = "PNP_OFFRES_NAIVE"
FILTER_ENV = "PNP_OFFRES_GRID_FILTER"


def timed(fn, reps, warmup):
    """ms per call: device events around `reps` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def engine(n, s, naive, grid_filter=False):
    """naive True / False: PNP_OFFRES_NAIVE=1 / 0; None: unset, the shipped choice per step.  grid_filter: PNP_OFFRES_GRID_FILTER=1, the
    two-segment gridding over the tile's whole bin instead of the plan's per-(segment, tile) lists"""
    old = {k: os.environ.pop(k, None) for k in (NAIVE_ENV, FILTER_ENV)}
    try:
        if naive is not None:
            os.environ[NAIVE_ENV] = "1" if naive else "0"
        if grid_filter:
            os.environ[FILTER_ENV] = "1"
        return PnPEngine(n, s, s, device=0, denoiser=False)                         # the variables are read at pnp_create
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=320)
    ap.add_argument("--width", type=int, default=6)
    ap.add_argument("--interleaves", type=int, default=16)
    ap.add_argument("--hz", type=float, default=100.0)
    ap.add_argument("--readout-ms", type=float, default=10.0)
    ap.add_argument("--segments", type=int, nargs="*", default=None, help="the L to time (default: the chooser's, capped at 32, and 8)")
    ap.add_argument("--cg-iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offres_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("offres_bench needs a ROCm GPU: a time measured anywhere else says nothing")
    n, s, g = a.n, a.size, a.grid
    dev = torch.device("cuda", 0)
    traj = acquisition.spiral_trajectory(s, s, a.interleaves)
    m = int(traj.shape[0])
    times = acquisition.readout_times("spiral", m, m // a.interleaves, a.readout_ms * 1e-3)
    omega = torch.from_numpy((2.0 * math.pi * synthetic.field_map(s, s, a.hz, 3)).astype(np.float32)).to(dev)
    om_max, span = float(omega.abs().max()), float(times.max() - times.min())
    asked = acquisition.offres_segments(om_max, span)
    Ls = a.segments or [min(asked, acquisition.OFFRES_MAX_SEGMENTS), 8]
    gt = torch.from_numpy(np.stack([synthetic.phantom(s, s, 100 + i % 8) for i in range(n)]).astype(np.float32)).reshape(n, 1, s, s).to(dev)
    mu = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    sg = torch.full((n,), 15.0 / 255.0, dtype=torch.float32, device=dev)
    calls = ("forward", "adjoint", "normal", "step")
    res = {"n": n, "size": s, "grid": g, "width": a.width, "interleaves": a.interleaves, "samples": m, "hz": a.hz, "readout_ms": a.readout_ms,
           "segments_asked_at_tol_1e-3": asked, "cg_iters": a.cg_iters, "reps": a.reps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "unit": "ms per call, median of rounds"}
    # the plain non-Cartesian stage beside them
    e = engine(n, s, None)
    e.nufft_plan(traj, grid=(g, g), width=a.width)
    dcf = e.nufft_dcf(iters=10)
    e.set_prior("tv")
    y1, _, x1 = e.acquire_nc(gt, 5.0 / 255.0, 1, dcf=dcf)
    img1 = x1.reshape(n, s, s).contiguous()
    xp, zp, up = e.reset_nc(x1, y1, dcf, cg_iters=a.cg_iters)
    plain = {"forward": lambda: e.nufft_forward(img1), "adjoint": lambda: e.nufft_adjoint(y1, dcf), "normal": lambda: e.nc_normal(zp, mu),
             "step": lambda: e.step(xp, zp, up, mu, sg)}
    pruns = {k: [timed(plain[k], a.reps, a.warmup) for _ in range(a.rounds)] for k in calls}
    res["plain"] = {k: spread(v) for k, v in pruns.items()}
    del e
    for L in Ls:
        forms, keep = {}, []
        for name, naive in (("two_segment", False), ("naive", True), ("shipped", None), ("two_segment_filter", False)):
            eo = engine(n, s, naive, grid_filter=name == "two_segment_filter")
            eo.nufft_plan(traj, grid=(g, g), width=a.width)
            eo.offres_plan(times, L)
            eo.set_prior("tv")
            maps = eo.offres_maps(omega)
            y, _, x0 = eo.acquire_offres(gt, omega, 5.0 / 255.0, 1, dcf=dcf)
            img = x0.reshape(n, s, s).contiguous()
            x, z, u = eo.reset_offres(x0, y, omega, dcf, cg_iters=a.cg_iters)
            keep.append(eo)
            forms[name] = {"forward": lambda eo=eo, img=img, maps=maps: eo.offres_forward(img, maps),
                           "adjoint": lambda eo=eo, y=y, maps=maps: eo.offres_adjoint(y, maps, dcf),
                           "normal": lambda eo=eo, z=z: eo.offres_normal(z, mu),
                           "step": lambda eo=eo, x=x, z=z, u=u: eo.step(x, z, u, mu, sg)}
        same = {k: bool(torch.equal(forms["two_segment"][k](), forms["naive"][k]())
                        and torch.equal(forms["two_segment"][k](), forms["two_segment_filter"][k]())) for k in ("forward", "adjoint", "normal")}
        runs = {f: {k: [] for k in calls} for f in forms}
        for r in range(a.rounds):
            for k in calls:
                for f in (tuple(forms) if r % 2 == 0 else tuple(forms)[::-1]):
                    runs[f][k].append(timed(forms[f][k], a.reps, a.warmup))
        out = {"segments": L, "model_error_bound": acquisition.offres_bound(om_max, span, L) if L > 1 else None, "numbers_equal": same}
        for f in forms:
            out[f] = {k: spread(v) for k, v in runs[f].items()}
        out["two_segment_over_naive"] = {k: out["two_segment"][k]["median"] / out["naive"][k]["median"] for k in calls}
        out["filter_over_lists"] = {k: out["two_segment_filter"][k]["median"] / out["two_segment"][k]["median"] for k in calls}
        out["shipped_over_naive"] = {k: out["shipped"][k]["median"] / out["naive"][k]["median"] for k in calls}
        out["shipped_over_plain"] = {k: out["shipped"][k]["median"] / res["plain"][k]["median"] for k in calls}
        res[f"L{L}"] = out
        print(f"L = {L} timed", file=sys.stderr, flush=True)
        del forms, keep
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
