#!/usr/bin/env python3
"""Timing of the multi-coil off-resonance operator and stage on the GPU (not a test): tools/offres_bench.py's workload with C = 8 coils of
`synthetic.coil_maps` - 16 slices of 256 x 256 on a 320 x 320 grid, a spiral of 16 interleaves, J = 6, a field map of 100 Hz over a readout
of 10 ms - once with L = 8 least-squares segments and once with L = 32 linear ones.  Per plan these handles of the same shape are timed in
alternating order, device events around `reps` back-to-back calls after a warm-up, `rounds` times, the median of the rounds reported with
their spread:
  single_coil_calls  what a caller could do before include/pnpadmm_offres_mc.h existed: C calls of pnp_offres_forward / pnp_offres_adjoint at
                     batch N on coil images multiplied beforehand (the multiplication and the final combine are NOT in the time); forward
                     and adjoint only - there is no stage to step
  composed           PNP_OFFRES_MC_NAIVE=1
  fused_cb1 / 2 / 4  PNP_OFFRES_MC_NAIVE=0 at PNP_OFFRES_MC_COIL_BLOCK = 1, 2, 4
  shipped            nothing set
Per form: pnp_offres_forward_mc, pnp_offres_adjoint_mc, pnp_offres_mc_normal (the cost of one CG iteration) and a whole pnp_step (K CG
iterations, TV prior).  Writes profiles/offres_mc_bench.json and prints it."""
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

NAIVE_ENV, BLOCK_ENV = "PNP_OFFRES_MC_NAIVE", "PNP_OFFRES_MC_COIL_BLOCK"


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


def engine(n, s, naive=None, block=None):
    old = {k: os.environ.pop(k, None) for k in (NAIVE_ENV, BLOCK_ENV)}
    try:
        if naive is not None:
            os.environ[NAIVE_ENV] = "1" if naive else "0"
        if block is not None:
            os.environ[BLOCK_ENV] = str(int(block))
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
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=320)
    ap.add_argument("--width", type=int, default=6)
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--interleaves", type=int, default=16)
    ap.add_argument("--hz", type=float, default=100.0)
    ap.add_argument("--readout-ms", type=float, default=10.0)
    ap.add_argument("--cg-iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offres_mc_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("offres_mc_bench needs a ROCm GPU: a time measured anywhere else says nothing")
    n, s, g, C = a.n, a.size, a.grid, a.coils
    dev = torch.device("cuda", 0)
    traj = acquisition.spiral_trajectory(s, s, a.interleaves)
    m = int(traj.shape[0])
    times = acquisition.readout_times("spiral", m, m // a.interleaves, a.readout_ms * 1e-3)
    omega = torch.from_numpy((2.0 * math.pi * synthetic.field_map(s, s, a.hz, 3)).astype(np.float32)).to(dev)
    om_max = float(omega.abs().max()) * (1.0 + 1e-6)
    sens = torch.from_numpy(synthetic.coil_maps(C, s, s).astype(np.complex64)).to(dev)
    gt = torch.from_numpy(np.stack([synthetic.phantom(s, s, 100 + i % 8) for i in range(n)]).astype(np.float32)).reshape(n, 1, s, s).to(dev)
    mu = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    sg = torch.full((n,), 15.0 / 255.0, dtype=torch.float32, device=dev)
    calls = ("forward", "adjoint", "normal", "step")
    res = {"n": n, "size": s, "grid": g, "width": a.width, "coils": C, "interleaves": a.interleaves, "samples": m, "hz": a.hz,
           "readout_ms": a.readout_ms, "cg_iters": a.cg_iters, "reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "unit": "ms per call, median of rounds"}
    dcf = None
    for label, L, ls in (("L8_ls", 8, True), ("L32_linear", 32, False)):
        forms, keep = {}, []
        for name, naive, block in (("composed", True, None), ("fused_cb1", False, 1), ("fused_cb2", False, 2), ("fused_cb4", False, 4),
                                   ("shipped", None, None)):
            e = engine(n, s, naive, block)
            e.nufft_plan(traj, grid=(g, g), width=a.width)
            if dcf is None:
                dcf = e.nufft_dcf(iters=10)
            if ls:
                e.offres_plan_ls(times, L, om_max)
            else:
                e.offres_plan(times, L)
            e.set_prior("tv")
            maps = e.offres_maps(omega)
            y, _, x0 = e.acquire_offres_mc(gt, sens, omega, 5.0 / 255.0, 1, dcf=dcf)
            img = x0.reshape(n, s, s).contiguous()
            x, z, u = e.reset_offres_mc(x0, y, sens, omega, dcf, cg_iters=a.cg_iters)
            keep.append(e)
            forms[name] = {"forward": lambda e=e, img=img, maps=maps: e.offres_forward_mc(img, maps, sens),
                           "adjoint": lambda e=e, y=y, maps=maps: e.offres_adjoint_mc(y, maps, sens, dcf),
                           "normal": lambda e=e, z=z: e.offres_mc_normal(z, mu),
                           "step": lambda e=e, x=x, z=z, u=u: e.step(x, z, u, mu, sg)}
            if name == "shipped":                                                   # the caller's loop over the coils, on the same handle
                coil_img = [(sens[c][None] * img).contiguous() for c in range(C)]
                coil_y = [y[:, c].contiguous() for c in range(C)]
                forms["single_coil_calls"] = {"forward": lambda e=e, ci=coil_img, maps=maps: [e.offres_forward(v, maps) for v in ci],
                                              "adjoint": lambda e=e, cy=coil_y, maps=maps: [e.offres_adjoint(v, maps, dcf) for v in cy]}
        same = {k: all(bool(torch.equal(forms["composed"][k](), forms[f][k]())) for f in ("fused_cb1", "fused_cb2", "fused_cb4", "shipped"))
                for k in ("forward", "adjoint", "normal")}
        runs = {f: {k: [] for k in forms[f]} for f in forms}
        for r in range(a.rounds):
            for k in calls:
                order = [f for f in forms if k in forms[f]]
                for f in (order if r % 2 == 0 else order[::-1]):
                    runs[f][k].append(timed(forms[f][k], a.reps, a.warmup))
        out = {"segments": L, "interpolator": "ls" if ls else "linear", "bits_equal": same}
        for f in forms:
            out[f] = {k: spread(v) for k, v in runs[f].items()}
        for f in ("fused_cb1", "fused_cb2", "fused_cb4", "shipped"):
            out[f + "_over_composed"] = {k: out[f][k]["median"] / out["composed"][k]["median"] for k in calls}
        out["shipped_over_single_coil_calls"] = {k: out["shipped"][k]["median"] / out["single_coil_calls"][k]["median"] for k in ("forward", "adjoint")}
        res[label] = out
        print(f"{label} timed", file=sys.stderr, flush=True)
        del forms, keep
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
