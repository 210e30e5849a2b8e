#!/usr/bin/env python3
"""Time pnp_residuals and one FixedScheduleSolver iteration with HIP events (profiles/residuals_kernel_stats.md).

    python tools/residuals_time.py [--n 64 --size 256] [--reps 200] [--warmup 20] [--out file.json]

Per call: median, min and max over `--reps` event-bracketed calls after `--warmup` calls, and the achieved bytes per second from the
bytes the algorithm needs (computed from the shape here), cache-warm (the same buffers call after call) and cold (a 1 GiB buffer
overwritten before every timed call):
  * residuals, PNP_RES_DELTA alone : 40 B per pixel (x, z, u and the three previous planes, read once)
  * residuals, PNP_RES_DC alone    : 12 (primal: x, z) + 4 + 8 (row pass) + 8 + 8 (column pass) + 8 + 8 + 1 (misfit) = 57 B per pixel
  * both                           : 40 + 45
  * pnp_psnr                       : 8 B per pixel (the yardstick the delta pass is held against)
  * pnp_snapshot                   : 40 B per pixel (20 read, 20 written)
and the solver's iteration (snapshot + pnp_step + residuals with PNP_RES_DELTA) against pnp_step alone on the same handle, alternating
the two, as a ratio.  Needs the GPU; there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dt4image_restoration_amd import synthetic, weights  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402


def timed(fn, reps, warmup, flush=None):
    """flush: called before every timed call, outside the event pair (cold figures: it overwrites a buffer larger than the last-level cache)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if flush is not None:
            flush()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "reps": reps}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("residuals_time.py needs the GPU")
    n, h, w = args.n, args.size, args.size
    px = n * h * w
    dev = torch.device("cuda", 0)
    eng = PnPEngine(n, h, w, device=0)
    eng.load_weights(weights.generate_unet_weights(0, "unit_gain"))
    p = synthetic.make_problem(n, h, w, accel=4.0, seed=1234)
    cx = lambda a: torch.view_as_complex(torch.from_numpy(np.ascontiguousarray(a))).reshape(n, 1, h, w).to(dev).contiguous()
    x, z, u = eng.reset(cx(p["x0"]), cx(p["y0"]), torch.from_numpy(p["mask"]).to(dev))
    gt = torch.from_numpy(p["gt"]).to(dev)
    mu_tab, sg_tab = synthetic.param_table(n, 30)
    mu, sg = torch.from_numpy(mu_tab[:, 0].copy()).to(dev), torch.from_numpy(sg_tab[:, 0].copy()).to(dev)
    snap = eng.snapshot(x, z, u)
    for _ in range(3):
        eng.step(x, z, u, mu, sg)
    out6 = torch.empty((n, 6), dtype=torch.float32, device=dev)
    res = {"shape": [n, h, w], "pixels": px}

    def rate(r, bytes_per_px):
        r["bytes"] = bytes_per_px * px
        r["gb_per_s"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
        return r

    # the inputs of the repeated calls below (168 MB at 64 x 256 x 256) stay in the 256 MB last-level cache from one call to the next: those
    # are cache-warm figures.  The "_cold" ones overwrite a 1 GiB buffer before every timed call, so every byte comes from HBM - which
    # is how the solver meets `prev` (written before the step, evicted by the step's activation planes).
    trash = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    cold = lambda: trash.fill_(1.0)
    creps = max(10, args.reps // 4)
    res["residuals_delta_cold"] = rate(timed(lambda: eng.residuals(x, z, u, prev=snap, out=out6), creps, 3, cold), 40)
    res["residuals_dc_cold"] = rate(timed(lambda: eng.residuals(x, z, u, dc=True, out=out6), creps, 3, cold), 57)
    res["residuals_both_cold"] = rate(timed(lambda: eng.residuals(x, z, u, prev=snap, dc=True, out=out6), creps, 3, cold), 85)
    res["psnr_cold"] = rate(timed(lambda: eng.psnr(x, gt), creps, 3, cold), 8)
    res["snapshot_cold"] = rate(timed(lambda: eng.snapshot(x, z, u, out=snap), creps, 3, cold), 40)
    res["residuals_delta"] = rate(timed(lambda: eng.residuals(x, z, u, prev=snap, out=out6), args.reps, args.warmup), 40)
    res["residuals_dc"] = rate(timed(lambda: eng.residuals(x, z, u, dc=True, out=out6), args.reps, args.warmup), 57)
    res["residuals_both"] = rate(timed(lambda: eng.residuals(x, z, u, prev=snap, dc=True, out=out6), args.reps, args.warmup), 85)
    res["residuals_primal_only"] = rate(timed(lambda: eng.residuals(x, z, u, out=out6), args.reps, args.warmup), 12)
    res["psnr"] = rate(timed(lambda: eng.psnr(x, gt), args.reps, args.warmup), 8)
    res["snapshot"] = rate(timed(lambda: eng.snapshot(x, z, u, out=snap), args.reps, args.warmup), 40)

    # one solver iteration against one pnp_step on the same handle, alternating (the iterate keeps moving: both see the same kind of data)
    def solver_iteration():
        eng.snapshot(x, z, u, out=snap)
        eng.step(x, z, u, mu, sg)
        eng.residuals(x, z, u, prev=snap, out=out6)

    step_ms, iter_ms = [], []
    for k in range(4):
        step_ms.append(timed(lambda: eng.step(x, z, u, mu, sg), args.step_reps, 5 if k else args.warmup)["median_ms"])
        iter_ms.append(timed(solver_iteration, args.step_reps, 5)["median_ms"])
    res["step_ms"] = step_ms
    res["solver_iteration_ms"] = iter_ms
    res["solver_iteration_over_step"] = float(np.median(iter_ms) / np.median(step_ms))
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
