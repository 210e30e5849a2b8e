"""Timing of the coil compression (pnp_coil_compress_matrix, pnp_coil_compress_apply) with device events, beside the composed torch route
a caller had before it - gather the block, `einsum` the covariance, `torch.linalg.eigh`, `einsum` over the planes - and of what the
compression buys: one `pnp_prox_dual` (K = 8) on the uncompressed problem and on the compressed one.

    python tools/coilcomp_bench.py [--sizes 64x256x256,16x512x512] [--compress 16:8,32:8] [--acs 24 24] [--reps 20] [--warmup 3]
                                   [--calls 10] [--blocks 4] [--cg-iters 8] [--out FILE.json]

Every event pair brackets `--calls` back-to-back calls and the time is divided by it: device time per call.  The routes run in alternating
blocks on one box (`--blocks` each: warm-up, then `--reps` pairs); the figure of a route is the median of its block medians.  Prints one
JSON line per (size, compression) with the times in microseconds, the bytes the launches move computed from the shapes here (not
measured), and the resulting TB/s.  No ratio is fixed in advance.
A kernel trace is a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/coilcomp_bench.py --blocks 1 --reps 3
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


def gram_chunks(acs):
    bins = acs[0] * acs[1]
    per = max(1024, -(-(-(-bins // 64)) // 32) * 32)
    return -(-bins // per)


def call_bytes(n, c, v, h, w, acs):
    """Bytes per launch of the two calls as they are structured ("Coil compression")."""
    blk, cc, g = n * c * acs[0] * acs[1], n * c * c, gram_chunks(acs)
    matrix = {"gram": blk * 8 + cc * g * 16, "gram_sum": cc * g * 16 + cc * 16, "eig": cc * 16 + cc * 8 + n * c * 4}
    return matrix, {"apply": n * h * w * 8 * (c + v) + (n * c * c * 8)}


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


def bench(n, h, w, coils, v, acs, reps, warmup, calls, blocks, cg_iters):
    dev = torch.device("cuda", 0)
    eng = PnPEngine(n, h, w, device=0, denoiser=False)
    small = PnPEngine(n, h, w, device=0, denoiser=False)             # the compressed problem's handle
    gt = torch.from_numpy(np.stack([synthetic.phantom(h, w, 300 + i) for i in range(n)]).astype(np.float32)).reshape(n, 1, h, w).to(dev)
    true = torch.from_numpy(synthetic.coil_maps(coils, h, w).astype(np.complex64)).to(dev)
    mask = torch.from_numpy(synthetic.radial_mask(h, w, 4.0)).to(dev)
    full = torch.ones((h, w), dtype=torch.bool, device=dev)
    y = eng.acquire(gt, full, 10.0 / 255.0, 7, sens=true)[0]        # fully sampled: any centred block is a calibration block
    sens_b = true[None].expand(n, coils, h, w).contiguous()
    cmat = torch.empty((n, coils, coils), dtype=torch.complex64, device=dev)
    eig = torch.empty((n, coils), dtype=torch.float32, device=dev)
    out = torch.empty((n, v, h, w), dtype=torch.complex64, device=dev)
    y0, y1, x0, x1 = h // 2 - acs[0] // 2, h // 2 + acs[0] // 2, w // 2 - acs[1] // 2, w // 2 + acs[1] // 2

    def matrix():
        _lib.check(eng.lib.pnp_coil_compress_matrix(eng._h, y.data_ptr(), coils, acs[0], acs[1], 0, cmat.data_ptr(), eig.data_ptr(), None,
                                                    eng._stream()), "pnp_coil_compress_matrix")

    def apply():
        _lib.check(eng.lib.pnp_coil_compress_apply(eng._h, y.data_ptr(), coils, cmat.data_ptr(), n, v, out.data_ptr(), eng._stream()),
                   "pnp_coil_compress_apply")

    state = {}

    def composed_matrix():
        b = y[:, :, y0:y1, x0:x1].reshape(n, coils, -1).to(torch.complex128)
        g = torch.einsum("nap,nbp->nab", b, b.conj())
        lam, u = torch.linalg.eigh(g)
        state["a"] = u.flip(-1).conj().transpose(1, 2).to(torch.complex64).contiguous()
        state["lam"] = lam.flip(-1)

    def composed_apply():
        return torch.einsum("nvc,nchw->nvhw", state["a"][:, :v], y)

    matrix(); apply()
    eigh_error = None
    try:
        composed_matrix()
        torch.cuda.synchronize()
    except RuntimeError as e:                                        # a torch build without a device eigen-solver: reported, not hidden
        eigh_error = str(e).split("\n")[0]
        state["a"] = cmat.clone()
    torch.cuda.synchronize()
    # the two routes keep the same energy (the vectors themselves are ill-conditioned where eigenvalues are close)
    energy = float((out.abs() ** 2).sum() / (y.abs() ** 2).sum())
    energy_composed = float((composed_apply().abs() ** 2).sum() / (y.abs() ** 2).sum())
    routes = [("matrix", matrix), ("apply", apply), ("composed_apply", composed_apply)]
    if eigh_error is None:
        routes.append(("composed_matrix", composed_matrix))

    # what the compression buys: one data-fidelity step on C coils and on V
    mu = torch.full((n,), 0.3, dtype=torch.float32, device=dev)
    xz = torch.zeros((n, 1, h, w), dtype=torch.complex64, device=dev)
    x, z, u = eng.reset(xz, y * mask, mask, sens=true, cg_iters=cg_iters)
    sens_v = torch.empty((n, v, h, w), dtype=torch.complex64, device=dev)
    _lib.check(eng.lib.pnp_coil_compress_apply(eng._h, sens_b.data_ptr(), coils, cmat.data_ptr(), n, v, sens_v.data_ptr(), eng._stream()),
               "pnp_coil_compress_apply")
    xs, zs, us = small.reset(xz, (out * mask).contiguous(), mask, sens=sens_v, cg_iters=cg_iters)
    routes += [("prox_dual_full", lambda: eng.prox_dual(x, z, u, mu)), ("prox_dual_compressed", lambda: small.prox_dual(xs, zs, us, mu))]

    med = {name: [] for name, _ in routes}
    for _ in range(blocks):
        for name, fn in routes:
            med[name].append(float(np.median(block(fn, reps, warmup, calls))))
    t = {name: float(np.median(vv)) for name, vv in med.items()}
    bm, ba = call_bytes(n, coils, v, h, w, acs)
    ws = {"full": eng.workspace_bytes, "compressed": small.workspace_bytes}
    eng.close(); small.close()
    row = {"shape": [n, h, w], "coils": coils, "out_coils": v, "acs": list(acs), "cg_iters": cg_iters, "calls_per_pair": calls, "reps": reps,
           "blocks": blocks, "us": t, "us_blocks": med, "matrix_bytes": bm, "apply_bytes": ba,
           "apply_TBps": sum(ba.values()) / (t["apply"] * 1e-6) / 1e12, "apply_flop_per_byte": 8.0 * coils * v / (8 * (coils + v)),
           "composed_apply_over_apply": t["composed_apply"] / t["apply"],
           "prox_dual_full_over_compressed": t["prox_dual_full"] / t["prox_dual_compressed"], "workspace_bytes": ws,
           "kept_energy": energy, "kept_energy_composed": energy_composed, "eigh_error": eigh_error}
    if eigh_error is None:
        row["composed_matrix_over_matrix"] = t["composed_matrix"] / t["matrix"]
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="64x256x256,16x512x512")
    ap.add_argument("--compress", default="16:8,32:8", help="comma-separated C:V pairs")
    ap.add_argument("--acs", type=int, nargs=2, default=(24, 24))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--cg-iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("coilcomp_bench needs a ROCm GPU: a timing taken anywhere else says nothing")
    rows = []
    for s in args.sizes.split(","):
        n, h, w = (int(x) for x in s.split("x"))
        for cv in args.compress.split(","):
            c, v = (int(x) for x in cv.split(":"))
            rows.append(bench(n, h, w, c, v, tuple(args.acs), args.reps, args.warmup, args.calls, args.blocks, args.cg_iters))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    main()
