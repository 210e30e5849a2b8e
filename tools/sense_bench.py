"""Timing of the multi-coil (SENSE) data-fidelity stage with device events: the whole stage (pnp_prox_dual in multi-coil mode, K CG
iterations) and one normal operator Nop (pnp_mc_normal), beside the denoiser's time on the same handle, at the two timed sizes.

    python tools/sense_bench.py [--sizes 64x256x256,16x512x512] [--coils 8] [--cg-iters 8] [--reps 20] [--warmup 3] [--out FILE.json]

Prints one JSON line per size: times (median, min over `reps` runs, in ms), the bytes the ALGORITHM moves computed from the shapes
here (not measured: every array a pass must read or write once, per launch as the stage is structured), the resulting TB/s, and the
launch count (from the structure, checked against the handle's own count of event pairs on a profiling handle).
A kernel trace is a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/sense_bench.py --reps 3
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

from dt4image_restoration_amd import synthetic, weights  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402


def nop_bytes(n, c, h, w, accel):
    """Bytes one Nop moves as the stage is structured (seven launches), and as the three-launch fused shape would."""
    px, cpx = n * h * w, n * c * h * w
    unfused = {
        "expand": px * 8 + cpx * 8 + cpx * 8,                  # p once per slice (L2 serves the coils), S, scratch out
        "rows_fwd": cpx * 16, "cols_fwd": cpx * 16,
        "mask": cpx * 1 + int(cpx * 8 * (1 - 1 / accel)),      # mask bytes in, zeros out on the unsampled bins
        "cols_inv": cpx * 16, "rows_inv": cpx * 16,
        "combine": cpx * 16 + px * 16,                         # scratch, S in; p in, q out
    }
    fused = {"rows_fwd+expand": px * 8 + cpx * 16, "cols_fwd+mask+cols_inv": cpx * 17, "rows_inv+combine": cpx * 16 + px * 16}
    return unfused, fused


def stage_bytes(n, c, h, w, accel, k):
    unfused, _ = nop_bytes(n, c, h, w, accel)
    px = n * h * w
    vec = {"cg_init": px * 44, "cg_update": px * 48, "cg_dir": px * 24, "dual": px * 28}
    return (k + 1) * sum(unfused.values()) + vec["cg_init"] + k * (vec["cg_update"] + vec["cg_dir"]) + vec["dual"]


def stage_launches(k):
    return (k + 1) * 7 + 2 + 4 * k + 1                          # Nops, init + scalar, (scalar, update, scalar, dir) per iteration, dual


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def bench(n, h, w, coils, k, reps, warmup, accel=8.0):
    dev = torch.device("cuda", 0)
    eng = PnPEngine(n, h, w, device=0)
    eng.load_weights(weights.generate_unet_weights(0, "unit_gain"))
    gt = torch.from_numpy(np.stack([synthetic.phantom(h, w, 300 + i) for i in range(n)]).astype(np.float32)).reshape(n, 1, h, w).to(dev)
    sens = torch.from_numpy(synthetic.coil_maps(coils, h, w).astype(np.complex64)).to(dev)
    mask = torch.from_numpy(synthetic.radial_mask(h, w, accel)).to(dev)
    y, _, x0 = eng.acquire(gt, mask, 10.0 / 255.0, 7, sens=sens)
    x, z, u = eng.reset(x0, y, mask, sens=sens, cg_iters=k)
    mu = torch.full((n,), 0.3, device=dev)
    sg = torch.full((n,), 20.0 / 255.0, device=dev)
    q = torch.empty_like(z)
    t_den = timed(lambda: eng.denoise(x, sg, out=x), reps, warmup)
    t_stage = timed(lambda: eng.prox_dual(x, z, u, mu), reps, warmup)
    t_nop = timed(lambda: eng.lib.pnp_mc_normal(eng._h, z.data_ptr(), mu.data_ptr(), q.data_ptr(), eng._stream()), reps, warmup)
    t_step = timed(lambda: eng.step(x, z, u, mu, sg), reps, warmup)
    res = eng.cg_residual().cpu().numpy()
    eng.close()
    # the launch count from a profiling handle's own event pairs
    pe = PnPEngine(n, h, w, device=0, denoiser=False, profile=True)
    pe.set_kspace(y, mask, sens=sens, cg_iters=k)
    torch.cuda.synchronize()
    pe.profile_reset()
    pe.prox_dual(x, z, u, mu)
    torch.cuda.synchronize()
    counted = sum(v["launches"] for name, v in pe.profile_collect().items() if name != "layers")
    pe.close()
    unf, fus = nop_bytes(n, coils, h, w, accel)
    nb, sb = sum(unf.values()), stage_bytes(n, coils, h, w, accel, k)
    return {"shape": [n, h, w], "coils": coils, "cg_iters": k, "accel": accel,
            "denoiser_ms": t_den[0], "stage_ms": t_stage[0], "stage_ms_min": t_stage[1], "nop_ms": t_nop[0], "nop_ms_min": t_nop[1],
            "step_ms": t_step[0], "stage_share_of_step": t_stage[0] / t_step[0],
            "nop_bytes": nb, "nop_bytes_fused_shape": sum(fus.values()), "nop_bytes_per_coil_pixel": nb / (n * coils * h * w),
            "nop_TBps": nb / (t_nop[0] * 1e-3) / 1e12, "stage_bytes": sb, "stage_TBps": sb / (t_stage[0] * 1e-3) / 1e12,
            "nop_launches": 7, "stage_launches": stage_launches(k), "stage_launches_counted": int(counted),
            "us_per_launch": 1e3 * t_stage[0] / stage_launches(k), "cg_res_max": float(res.max())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="64x256x256,16x512x512")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--cg-iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    rows = []
    for s in args.sizes.split(","):
        n, h, w = (int(v) for v in s.split("x"))
        rows.append(bench(n, h, w, args.coils, args.cg_iters, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
