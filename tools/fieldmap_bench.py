"""Timing of the field map estimator with device events: pnp_fieldmap_estimate as the fused kernel beside the one-launch-per-sweep form
(PNP_FIELDMAP_NAIVE=1, read at pnp_create), alternating on one box, and pnp_fieldmap_cost.

    python tools/fieldmap_bench.py [--size 64x256x256] [--coils 1,8] [--iters 200] [--rounds 5] [--calls 3] [--warmup 2] [--out FILE.json]

Every event pair brackets `--calls` back-to-back calls and the time is divided by it: device time per call.  A round times the fused form,
then the naive form, then the calls with iters = 0 (the prepare and finish launches alone) and the cost; the figure of a form is the median
of its `--rounds` rounds.  Prints one JSON line per coil count with the times in microseconds, the bytes each form of the ALGORITHM moves
computed from the shapes here (not measured: the halo re-reads of the fused kernel, which its neighbours' tiles leave in the cache, are
not counted) and the resulting TB/s of the sweeps alone.  Writes profiles/fieldmap_bench.json by default.
A kernel trace is a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/fieldmap_bench.py --rounds 1 --out /dev/null
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dt4image_restoration_amd._lib import PNP_FIELDMAP_T as FUSE_T  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402


def sweep_bytes(n, h, w, iters):
    """Bytes the sweeps of one call move, per form.  A launch of either form reads theta, phi, w and rd (16 B a pixel) and writes theta (4 B);
    the fused form does so once per FUSE_T sweeps."""
    px, launches = n * h * w, -(-iters // FUSE_T)
    return {"fused": px * 20 * launches, "naive": px * 20 * iters, "fused_launches": launches, "naive_launches": iters}


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def make_engine(n, h, w, naive):
    if naive:
        os.environ["PNP_FIELDMAP_NAIVE"] = "1"
    try:
        return PnPEngine(n, h, w, device=0, denoiser=False)
    finally:
        os.environ.pop("PNP_FIELDMAP_NAIVE", None)


def echoes(n, coils, h, w, dte, dev):
    """two echo images of a smooth object under a smooth map of at most 100 Hz, with noise: what the kernels see in use"""
    g = torch.Generator(device="cpu").manual_seed(7)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    mag = torch.exp(-2.0 * (yy ** 2 + xx ** 2)).expand(n, coils, h, w)
    om = 2.0 * math.pi * 100.0 * torch.sin(2.0 * yy) * torch.cos(1.5 * xx)
    out = []
    for t in (1e-3, 1e-3 + dte):
        x = torch.polar(mag, (-om * t).expand(n, coils, h, w)) + 0.02 * torch.view_as_complex(torch.randn((n, coils, h, w, 2), generator=g))
        out.append(x.to(torch.complex64).to(dev).contiguous())
    return out


def bench(n, h, w, coils, iters, rounds, calls, warmup, dte=2e-3, beta=0.05):
    dev = torch.device("cuda", 0)
    x1, x2 = echoes(n, coils, h, w, dte, dev)
    eng = {"fused": make_engine(n, h, w, False), "naive": make_engine(n, h, w, True)}
    res = {k: e.fieldmap_estimate(x1, x2, dte, beta=beta, iters=iters) for k, e in eng.items()}
    torch.cuda.synchronize()
    same = bool(torch.equal(res["fused"].view(torch.int32), res["naive"].view(torch.int32)))
    om = res["fused"]
    fns = {"fused": lambda: eng["fused"].fieldmap_estimate(x1, x2, dte, beta=beta, iters=iters),
           "naive": lambda: eng["naive"].fieldmap_estimate(x1, x2, dte, beta=beta, iters=iters),
           "prepare_finish": lambda: eng["fused"].fieldmap_estimate(x1, x2, dte, beta=beta, iters=0),
           "cost": lambda: eng["fused"].fieldmap_cost(x1, x2, dte, beta, om)}
    us = {k: [] for k in fns}
    for _ in range(rounds):                                  # the forms alternate inside a round
        for k, fn in fns.items():
            us[k].append(timed(fn, calls, warmup))
    t = {k: float(np.median(v)) for k, v in us.items()}
    by = sweep_bytes(n, h, w, iters)
    sweeps = {k: max(t[k] - t["prepare_finish"], 1e-3) for k in ("fused", "naive")}
    for e in eng.values():
        e.close()
    return {"shape": [n, h, w], "coils": coils, "iters": iters, "fuse_t": FUSE_T, "rounds": rounds, "calls_per_pair": calls,
            "fused_us": t["fused"], "naive_us": t["naive"], "naive_over_fused": t["naive"] / t["fused"], "prepare_finish_us": t["prepare_finish"],
            "cost_us": t["cost"], "us_rounds": us, "sweep_bytes": by,
            "fused_sweeps_TBps": by["fused"] / (sweeps["fused"] * 1e-6) / 1e12, "naive_sweeps_TBps": by["naive"] / (sweeps["naive"] * 1e-6) / 1e12,
            "fused_ns_per_pixel_sweep": 1e3 * sweeps["fused"] / (n * h * w * iters), "naive_ns_per_pixel_sweep": 1e3 * sweeps["naive"] / (n * h * w * iters),
            "fused_and_naive_same_bits": same}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", default="64x256x256")
    ap.add_argument("--coils", default="1,8")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldmap_bench.json"))
    args = ap.parse_args(argv)
    if not 1 <= args.iters <= 4096:
        raise SystemExit(f"--iters must be 1..4096, got {args.iters}")
    if not torch.cuda.is_available():
        raise SystemExit("fieldmap_bench needs a ROCm GPU: a timing taken anywhere else says nothing")
    n, h, w = (int(v) for v in args.size.split("x"))
    rows = []
    for c in (int(v) for v in args.coils.split(",")):
        rows.append(bench(n, h, w, c, args.iters, args.rounds, args.calls, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out and args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
