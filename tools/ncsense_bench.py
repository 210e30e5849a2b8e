#!/usr/bin/env python3
"""Timing of the non-Cartesian SENSE stage on the GPU (not a test): 16 slices of 256 x 256 on a 320 x 320 grid, 8 coils, 64 golden-angle
spokes of 512 samples, J = 6.  Three handles of the same shape - every step coil-batched (PNP_NCSENSE_NAIVE=0), every step in the naive form
(PNP_NCSENSE_NAIVE=1: the single-coil launches at batch N C between an expand and a combine kernel) and the shipped choice per step
(unset) - are timed in alternating order, device
events around `reps` back-to-back calls after a warm-up, `rounds` times; the median of the rounds is reported with their spread.  Per form:
pnp_nufft_forward_mc (pad + grid transform + gather), pnp_nufft_adjoint_mc (gridding + grid transform + crop and combine), the whole
pnp_ncsense_normal and a whole pnp_step (K CG iterations, TV prior).  The forms share the grid transform, so a difference between them is the
difference of the pad / gather or of the gridding / crop launches.  The reference point is the single-coil pnp_nc_normal on the same handle
times C: what C independent single-coil operators cost.  Writes profiles/ncsense_bench.json and prints it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dt4image_restoration_amd import acquisition, synthetic  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402

NAIVE_ENV = "PNP_NCSENSE_NAIVE"


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


def engine(n, s, naive):
    """naive True / False: PNP_NCSENSE_NAIVE=1 / 0 (every step naive / coil-batched); None: unset, the shipped choice per step"""
    old = os.environ.pop(NAIVE_ENV, None)
    try:
        if naive is not None:
            os.environ[NAIVE_ENV] = "1" if naive else "0"
        return PnPEngine(n, s, s, device=0, denoiser=False)                         # the variable is read at pnp_create
    finally:
        os.environ.pop(NAIVE_ENV, None)
        if old is not None:
            os.environ[NAIVE_ENV] = old


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--grid", type=int, default=320)
    ap.add_argument("--width", type=int, default=6)
    ap.add_argument("--readout", type=int, default=512)
    ap.add_argument("--spokes", type=int, default=64)
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--cg-iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-single", action="store_true", help="skip the single-coil reference point and write no file (kernel traces: the "
                    "single-coil launches then all belong to the naive form)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncsense_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ncsense_bench needs a ROCm GPU: a time measured anywhere else says nothing")
    n, s, g, c = a.n, a.size, a.grid, a.coils
    dev = torch.device("cuda", 0)
    traj = acquisition.radial_trajectory(s, s, a.spokes, readout=a.readout)
    dcf = torch.from_numpy(acquisition.radial_dcf(traj, s, s)).to(dev)
    sens = torch.from_numpy(synthetic.coil_maps(c, s, s).astype(np.complex64)).to(dev)
    gt = torch.from_numpy(np.stack([synthetic.phantom(s, s, 100 + i % 8) for i in range(n)]).astype(np.float32)).reshape(n, 1, s, s).to(dev)
    mu = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    sg = torch.full((n,), 15.0 / 255.0, dtype=torch.float32, device=dev)
    forms = {}
    for name, naive in (("batched", False), ("naive", True), ("shipped", None)):
        e = engine(n, s, naive)
        e.nufft_plan(traj, grid=(g, g), width=a.width)
        e.set_prior("tv")
        y, _, x0 = e.acquire_ncsense(gt, sens, 5.0 / 255.0, 1, dcf=dcf)
        img = x0.reshape(n, s, s).contiguous()
        x, z, u = e.reset_ncsense(x0, y, sens, dcf, cg_iters=a.cg_iters)
        forms[name] = {"forward_mc": lambda e=e, img=img: e.nufft_forward_mc(img, sens),
                       "adjoint_mc": lambda e=e, y=y: e.nufft_adjoint_mc(y, sens, dcf),
                       "normal": lambda e=e, z=z: e.ncsense_normal(z, mu),
                       "step": lambda e=e, x=x, z=z, u=u: e.step(x, z, u, mu, sg)}
    same = bool(torch.equal(torch.view_as_real(forms["batched"]["normal"]()), torch.view_as_real(forms["naive"]["normal"]())))
    calls = ("forward_mc", "adjoint_mc", "normal", "step")
    runs = {f: {k: [] for k in calls} for f in forms}
    for r in range(a.rounds):
        for k in calls:
            for f in (("batched", "naive", "shipped") if r % 2 == 0 else ("shipped", "naive", "batched")):
                runs[f][k].append(timed(forms[f][k], a.reps, a.warmup))
    res = {"n": n, "size": s, "grid": g, "width": a.width, "coils": c, "spokes": a.spokes, "readout": a.readout, "samples": int(traj.shape[0]),
           "cg_iters": a.cg_iters, "reps": a.reps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "ms per call, median of rounds",
           "normal_bits_equal": same}
    for f in forms:
        res[f] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in runs[f].items()}
    res["batched_over_naive"] = {k: res["batched"][k]["median"] / res["naive"][k]["median"] for k in calls}
    res["shipped_over_naive"] = {k: res["shipped"][k]["median"] / res["naive"][k]["median"] for k in calls}
    if a.no_single:
        print(json.dumps(res, indent=1))
        return
    # the reference point: C independent single-coil normal operators
    e = engine(n, s, None)
    e.nufft_plan(traj, grid=(g, g), width=a.width)
    y1, _, x1 = e.acquire_nc(gt, 5.0 / 255.0, 1, dcf=dcf)
    _, z1, _ = e.reset_nc(x1, y1, dcf, cg_iters=a.cg_iters)
    single = [timed(lambda: e.nc_normal(z1, mu), a.reps, a.warmup) for _ in range(a.rounds)]
    res["single_coil_normal"] = {"median": statistics.median(single), "min": min(single), "max": max(single)}
    res["single_coil_normal_times_coils"] = statistics.median(single) * c
    res["shipped_normal_over_single_times_coils"] = res["shipped"]["normal"]["median"] / res["single_coil_normal_times_coils"]
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
