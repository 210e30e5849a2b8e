"""Timing of the ESPIRiT coil map estimate (pnp_espirit_sens) with device events, beside pnp_estimate_sens on the same input for scale.

    python tools/espirit_bench.py [--sizes 64x256x256,16x512x512] [--coils 8] [--acs 24 24] [--ksize 6] [--iters 16] [--reps 20] [--warmup 3]
                                  [--out FILE.json]

Every event pair brackets ONE call (a call is milliseconds long); the figure is the median of `--reps` pairs after `--warmup` calls.  There is
no earlier route to beat and no ratio is fixed in advance.  Prints one JSON line per size with the times in microseconds and the
floating-point work of the stages computed from the shapes here (not measured): the Gram matrix, an estimate of the Jacobi solver (12 sweeps
assumed), the kernel auto-correlation for the measured nkept, and the pixel kernel.
The C ABI is one call, so the split into stages comes from a kernel trace, a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/espirit_bench.py --reps 3 --warmup 1
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

from dt4image_restoration_amd import _lib, synthetic  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402


def stage_flops(n, c, h, w, acs, k, iters, nkept, sweeps=12):
    """Real floating-point operations per call, from the shapes (a complex multiply-add counts 8).  gram, eig, kern are float64; pixels float32."""
    nn, d = c * k * k, 2 * k - 1
    windows = (acs[0] - k + 1) * (acs[1] - k + 1)
    gram = n * 8 * windows * nn * (nn + 1) // 2
    # a round of nn / 2 rotations: 16 complex multiply-adds per 2 x 2 block (pair k, pair l), k > l, and 4 per (row, pair) of the vectors
    eig = n * sweeps * (nn - 1) * 8 * (16 * (nn // 2) * (nn // 2 - 1) // 2 + 4 * nn * (nn // 2))
    kern = int(sum(8 * nk * (k * k) ** 2 * c * c for nk in nkept))           # all (i, j) pairs of every (a, b), once per kept vector
    per_pixel = 8 * (d * c * (c + 1) // 2 + (iters + 1) * c * c) + iters * (8 * c + 2) + 16 * c
    rows = n * h * 8 * d * d * c * (c + 1) // 2                               # the d_y contraction, once per image row
    return {"gram": gram, "eig_estimate": eig, "kern": kern, "pixels": n * h * w * per_pixel + rows}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    return float(np.median(us)), us


def bench(n, h, w, coils, acs, k, iters, reps, warmup):
    dev = torch.device("cuda", 0)
    eng = PnPEngine(n, h, w, device=0, denoiser=False)
    gt = torch.from_numpy(np.stack([synthetic.phantom(h, w, 300 + i) for i in range(n)]).astype(np.float32)).reshape(n, 1, h, w).to(dev)
    true = torch.from_numpy(synthetic.coil_maps(coils, h, w).astype(np.complex64)).to(dev)
    ones = torch.ones((h, w), dtype=torch.bool, device=dev)
    y = eng.acquire(gt, ones, 10.0 / 255.0, 7, sens=true)[0]
    sens, low = torch.empty_like(y), torch.empty_like(y)
    ev = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    d = 2 * k - 1
    kern = torch.empty((n, coils, coils, d, d), dtype=torch.complex64, device=dev)
    nkept = torch.empty((n,), dtype=torch.int32, device=dev)
    code = _lib.SENS_WINDOWS["hann"]

    def call():
        _lib.check(eng.lib.pnp_espirit_sens(eng._h, y.data_ptr(), coils, acs[0], acs[1], k, 0.02, 0.9, iters, code, 0.05, 0, sens.data_ptr(),
                                            ev.data_ptr(), kern.data_ptr(), nkept.data_ptr(), eng._stream()), "pnp_espirit_sens")

    def lowres():
        _lib.check(eng.lib.pnp_estimate_sens(eng._h, y.data_ptr(), coils, acs[0], acs[1], code, 0.05, 0, low.data_ptr(), None, eng._stream()),
                   "pnp_estimate_sens")

    t_call, all_call = timed(call, reps, warmup)
    t_low, _ = timed(lowres, reps, warmup)
    nk = nkept.cpu().tolist()
    kept = float((sens.abs().pow(2).sum(dim=1) > 0.5).float().mean())
    rms = float((sens - true[None]).abs().pow(2).sum(dim=1)[gt[:, 0] > 0.1].mean().sqrt() / np.sqrt(coils))
    rms_low = float((low - true[None]).abs().pow(2).sum(dim=1)[gt[:, 0] > 0.1].mean().sqrt() / np.sqrt(coils))
    eng.close()
    return {"shape": [n, h, w], "coils": coils, "acs": list(acs), "ksize": k, "iters": iters, "reps": reps, "espirit_us": t_call,
            "espirit_us_min_max": [min(all_call), max(all_call)], "estimate_sens_us": t_low, "espirit_over_estimate_sens": t_call / t_low,
            "nkept_min_max": [min(nk), max(nk)], "kept_share": kept, "rms_map_error_on_gt_above_0.1": rms, "rms_map_error_lowres": rms_low,
            "flops_from_shapes": stage_flops(n, coils, h, w, acs, k, iters, nk)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="64x256x256,16x512x512")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--acs", type=int, nargs=2, default=(24, 24))
    ap.add_argument("--ksize", type=int, default=6)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("espirit_bench needs a ROCm GPU: a timing taken anywhere else says nothing")
    rows = []
    for s in args.sizes.split(","):
        n, h, w = (int(v) for v in s.split("x"))
        rows.append(bench(n, h, w, args.coils, tuple(args.acs), args.ksize, args.iters, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
