#!/usr/bin/env python3
"""Time pnp_acquire with HIP events (profiles/acquire_kernel_stats.md).

    python tools/acquire_bench.py [--shapes 64x256x256,16x512x512] [--reps 200] [--warmup 20] [--out file.json]

Per shape, all three outputs stored, radial mask at acceleration 4, sigma_n = 10 / 255:
  * pnp_acquire: median / min / max over `--reps` event-bracketed calls after `--warmup` calls, cache-warm (the same buffers call after
    call) and cold (a 1 GiB buffer overwritten before every timed call), and the achieved bytes per second over the bytes the launches
    move, counted from the shape here: 12 (rows: gt 4, scratch 8) + 16 (columns) + 8 f + 1 + 8 (epilogue: scratch read on the sampled
    fraction f, mask, y0) + 8 (scratch written) + 16 (columns back) + 16 (rows back -> ATy0) + 16 (clamp -> x0) B per pixel;
  * the route the library offered before, on the same handle: complex copy of gt, pnp_fft2c forward, torch noise, add and mask,
    pnp_fft2c inverse, torch clamp - timed in blocks that alternate with blocks of pnp_acquire, the ratio of the block medians reported.
    A single call of either route is short enough (150-200 us, six launches against a dozen) for the host's launch time to show in an
    event pair around ONE call, so the blocks and the `_x<inner>` rows bracket `--inner` back-to-back calls and divide: device time per call;
  * synthetic.make_problem's CPU time for the same shape (phantoms, mask and transforms in numpy float64), from `--cpu-slices` slices.
Needs the GPU; there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dt4image_restoration_amd import _lib, synthetic  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402


def timed(fn, reps, warmup, flush=None, inner=1):
    """flush: called before every timed call, outside the event pair (cold figures: it overwrites a buffer larger than the last-level cache).
    inner: calls enqueued back to back inside one event pair, the pair's time divided by it - with inner > 1 the host enqueues ahead of the
    device, so the figure is the device's time per call and not the host's launch time."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if flush is not None:
            flush()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev]) / inner
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "reps": reps}


def bench_shape(n, h, w, args, trash):
    dev = torch.device("cuda", 0)
    px = n * h * w
    eng = PnPEngine(n, h, w, device=0, denoiser=False)
    sigma, seed = 10.0 / 255.0, 1234
    mask_np = synthetic.radial_mask(h, w, 4.0)
    frac = float(mask_np.mean())
    mask = torch.from_numpy(mask_np).to(dev).to(torch.uint8).contiguous()
    maskc = mask.to(torch.complex64)
    gt = torch.from_numpy(np.stack([synthetic.phantom(h, w, seed + i) for i in range(min(n, 4))]).astype(np.float32))
    gt = gt.repeat((n + gt.shape[0] - 1) // gt.shape[0], 1, 1)[:n].reshape(n, 1, h, w).to(dev).contiguous()
    y0 = torch.empty((n, 1, h, w), dtype=torch.complex64, device=dev)
    aty0, x0 = torch.empty_like(y0), torch.empty_like(y0)

    def acquire():
        _lib.check(eng.lib.pnp_acquire(eng._h, gt.data_ptr(), mask.data_ptr(), 1, sigma, seed, 0, y0.data_ptr(), aty0.data_ptr(),
                                       x0.data_ptr(), eng._stream()), "pnp_acquire")

    def composed():
        c = gt.to(torch.complex64)                         # complex copy of gt
        f = eng.fft2c(c)                                   # pnp_fft2c forward
        noise = torch.view_as_complex(torch.randn((n, 1, h, w, 2), device=dev) * sigma)
        yy = (f + noise) * maskc                           # add and mask
        a = eng.fft2c(yy, inverse=True)                    # pnp_fft2c inverse
        return yy, a, torch.view_as_complex(torch.view_as_real(a).clamp_min(0))

    bytes_per_px = 12 + 16 + 8 * frac + 1 + 8 + 8 + 16 + 16 + 16
    res = {"shape": [n, h, w], "pixels": px, "sampled_fraction": frac, "bytes_per_px": bytes_per_px}
    cold = lambda: trash.fill_(1.0)
    creps = max(10, args.reps // 4)
    for name, fn in (("acquire", acquire), ("composed", composed)):
        res[name + "_cold"] = timed(fn, creps, 3, cold)
        res[name] = timed(fn, args.reps, args.warmup)
        res[name + "_x%d" % args.inner] = timed(fn, max(10, args.reps // args.inner), 3, inner=args.inner)
    for k in ("acquire", "acquire_cold"):
        res[k]["gb_per_s"] = bytes_per_px * px / (res[k]["median_ms"] * 1e-3) / 1e9
    # alternating blocks on the same handle
    blocks = {"acquire": [], "composed": []}
    for k in range(4):
        for name, fn in (("acquire", acquire), ("composed", composed)):
            blocks[name].append(timed(fn, max(10, args.reps // 4 // args.inner), 2, inner=args.inner)["median_ms"])
    res["blocks_ms"] = blocks
    res["composed_over_acquire"] = float(np.median(blocks["composed"]) / np.median(blocks["acquire"]))
    res["composed_over_acquire_cold"] = res["composed_cold"]["median_ms"] / res["acquire_cold"]["median_ms"]
    t0 = time.perf_counter()
    synthetic.make_problem(args.cpu_slices, h, w, accel=4.0, sigma_n=sigma, seed=seed)
    res["make_problem_cpu_s_per_slice"] = (time.perf_counter() - t0) / args.cpu_slices
    res["make_problem_cpu_s_for_batch"] = res["make_problem_cpu_s_per_slice"] * n
    eng.close()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x256x256,16x512x512")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per event pair of the `_x<inner>` rows and the alternating blocks")
    ap.add_argument("--cpu-slices", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("acquire_bench.py needs the GPU")
    trash = torch.empty(1 << 28, dtype=torch.float32, device="cuda:0")
    out = []
    for s in args.shapes.split(","):
        n, h, w = (int(v) for v in s.split("x"))
        out.append(bench_shape(n, h, w, args, trash))
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
