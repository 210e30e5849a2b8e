"""Timing of the total-variation prior with device events: pnp_tv_denoise and a whole pnp_step under PNP_PRIOR_TV, the fused kernel beside
the one-launch-per-iteration form (PNP_TV_NAIVE=1, read at pnp_create), on one box in alternating blocks.

    python tools/tv_bench.py [--sizes 64x256x256,16x512x512] [--iters 20] [--reps 20] [--warmup 3] [--calls 10] [--blocks 4] [--out FILE.json]

Every event pair brackets `--calls` back-to-back calls and the time is divided by it: device time per call.  The figure of a form is the
median of its block medians (`--blocks` each: warm-up, then `--reps` pairs).  Prints one JSON line per size with the times in microseconds,
the bytes each form of the ALGORITHM moves computed from the shapes here (not measured: halo re-reads of the fused kernel, which its
neighbours' tiles leave in the cache, are not counted) and the resulting TB/s.
A kernel trace is a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/tv_bench.py --blocks 1 --reps 3
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dt4image_restoration_amd import synthetic  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402

FUSE_T = 10                                                # kTvT of csrc/pnp_internal.h


def denoise_bytes(n, h, w, iters):
    """Bytes per pnp_tv_denoise call (out not aliasing x_in), per form.  fused: every launch reads v (4 B) and, but the first, p (8 B); every
    launch but the last writes p (8 B), the last writes out (4 B).  naive: an iteration reads v and p (p of the first is zero: not read) and
    writes p, the closing launch reads v and p and writes out."""
    px, launches = n * h * w, -(-iters // FUSE_T)
    fused = px * (4 * launches + 8 * (launches - 1) + 8 * (launches - 1) + 4)
    naive = px * (iters * (4 + 8) + (iters - 1) * 8 + 4 + 8 + 4)
    return {"fused": fused, "naive": naive, "fused_launches": launches, "naive_launches": iters + 1}


def block(fn, reps, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / calls)
    return us


def make_engine(n, h, w, naive):
    if naive:
        os.environ["PNP_TV_NAIVE"] = "1"
    try:
        return PnPEngine(n, h, w, device=0, denoiser=False)
    finally:
        os.environ.pop("PNP_TV_NAIVE", None)


def bench(n, h, w, iters, reps, warmup, calls, blocks):
    dev = torch.device("cuda", 0)
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=1234)
    cplx = lambda a: torch.from_numpy(np.ascontiguousarray(a[..., 0] + 1j * a[..., 1]).astype(np.complex64)).to(dev)
    x0, y0, mask = cplx(d["x0"]), cplx(d["y0"]), torch.from_numpy(d["mask"]).to(dev)
    v = x0.real.contiguous()
    lam = torch.full((n,), 0.1, dtype=torch.float32, device=dev)
    mu = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    out = torch.empty_like(v)
    fns, engines, results = {}, [], {}
    for name, naive in (("fused", False), ("naive", True)):
        eng = make_engine(n, h, w, naive)
        eng.set_prior("tv", 1.0, iters)
        x, z, u = eng.reset(x0, y0, mask)
        engines.append(eng)
        results[name] = eng.tv_denoise(v, lam, iters).clone()
        fns[name + "_denoise"] = (lambda eng=eng: eng.tv_denoise(v, lam, iters, out=out))
        fns[name + "_step"] = (lambda eng=eng, x=x, z=z, u=u: eng.step(x, z, u, mu, lam))
        fns[name + "_prox"] = (lambda eng=eng, x=x, z=z, u=u: eng.prox_dual(x, z, u, mu))
    torch.cuda.synchronize()
    same = bool(torch.equal(results["fused"].view(torch.int32), results["naive"].view(torch.int32)))
    med = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            med[k].append(float(np.median(block(fn, reps, warmup, calls))))
    t = {k: float(np.median(vs)) for k, vs in med.items()}
    by = denoise_bytes(n, h, w, iters)
    for eng in engines:
        eng.close()
    return {"shape": [n, h, w], "iters": iters, "calls_per_pair": calls, "reps": reps, "blocks": blocks,
            "fused_denoise_us": t["fused_denoise"], "naive_denoise_us": t["naive_denoise"], "naive_over_fused": t["naive_denoise"] / t["fused_denoise"],
            "fused_step_us": t["fused_step"], "naive_step_us": t["naive_step"], "prox_dual_us": t["fused_prox"], "us_blocks": med,
            "bytes": by, "fused_TBps": by["fused"] / (t["fused_denoise"] * 1e-6) / 1e12, "naive_TBps": by["naive"] / (t["naive_denoise"] * 1e-6) / 1e12,
            "fused_ns_per_pixel_iteration": 1e3 * t["fused_denoise"] / (n * h * w * iters), "fused_and_naive_same_bits": same}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="64x256x256,16x512x512")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not 1 <= args.iters <= 64:
        raise SystemExit(f"--iters must be 1..64, got {args.iters}")
    if not torch.cuda.is_available():
        raise SystemExit("tv_bench needs a ROCm GPU: a timing taken anywhere else says nothing")
    rows = []
    for s in args.sizes.split(","):
        n, h, w = (int(v) for v in s.split("x"))
        rows.append(bench(n, h, w, args.iters, args.reps, args.warmup, args.calls, args.blocks))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
