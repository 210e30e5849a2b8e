"""Command line with the reference's sub-commands (/root/reference/main.py:133-240, scripts.sh):

    python -m dt4image_restoration_amd.cli --block_size 18 --n_embeds 9 eval --rtg 10 --max_timesteps 30
    python -m dt4image_restoration_amd.cli --block_size 18 --n_embeds 9 mcts --rtg 5  --max_timesteps 30
    python -m dt4image_restoration_amd.cli --block_size 18 --n_embeds 6 flex --max_timesteps 30

plus `fixed`, which the reference does not have: plain PnP-ADMM with a fixed mu and a geometric sigma_d schedule, stopped per slice
by the fixed-point criterion delta <= tol (drivers/fixed.py; no policy involved):

    python -m dt4image_restoration_amd.cli --block_size 18 --n_embeds 9 --size 320 fixed --mu 0.3 --sigma-start 50 --sigma-end 5 \
        --tol 0.005 --max_iter 30 --dc

`eval` and `flex` take `--residuals` (adds the final iterate's primal residual and k-space data misfit to their lines), `mcts` takes
`--scorer neg_dc` (rollouts scored by minus the data misfit - a reference-free number - instead of the smoothness stub).

Evaluation data made on the GPU (acquisition.py, pnp_acquire) instead of read from `.mat` files or built on the CPU:

    ... --gt DIR [DIR ...] --tasks 4x_10,8x_10 --mask cartesian eval ...    one set per (folder of ground-truth images, task)
    ... --acquire device eval ...                                           the synthetic sets, phantoms acquired on the device
    ... acquire --gt DIR --out DIR                                          writes DIR/<task>/gt_<accel>_<sigma>_<image>.mat

Multi-coil (SENSE) problems, on synthetic data and on --gt folders, with the analytic maps of `synthetic.coil_maps`; the k-space
subproblem is then solved by K conjugate-gradient iterations per step (`acquire` has no coil axis to write: the reference's `.mat`
layout has none):

    ... --coils 4 --cg-iters 8 eval|flex|mcts|fixed ...
    ... --traj radial [--spokes S] [--nufft-width 4|6|8] [--nufft-grid GH GW] [--nc-weights none|dcf|pipe] [--cg-iters K] eval|flex|mcts|fixed|acquire ...
    ... --traj spiral [--interleaves L] | --traj rosette [--petals P]  [--nc-weights none|dcf|pipe] [--dcf-iters I] eval|flex|mcts|fixed|acquire ...
    ... --traj radial --nc-coils 4 [--cg-iters K] eval|flex|mcts|fixed|acquire ...      (non-Cartesian SENSE: the radial acquisition of C coils)
    ... --traj spiral --b0 HZ --readout-ms T --b0-coils 4 [--b0-interp ls] [--b0-segments L] eval|flex|mcts|fixed ...   (coils x segments stage)
    ... --traj spiral --b0 HZ --readout-ms T [--b0-coils 4] --b0-normal toeplitz eval|flex|mcts|fixed ...   (the CG on the Toeplitz form of A^H W A)
    ... --coils 4 --sens estimate [--sens-window hann|box] [--sens-thresh 0.05] [--acs H W] --mask cartesian fixed ...

    ... --coils 8 --sens espirit [--espirit-kernel 6] [--espirit-sv 0.02] [--espirit-crop 0.9] [--espirit-iters 16] --mask cartesian fixed ...

    ... --coils 16 --compress 8 [--sens true|estimate|espirit] [--acs H W] eval|flex|mcts|fixed ...
    ... --coils 8 --mask uniform --grappa [--grappa-kernel 5 4] [--grappa-lambda 0.01] eval|flex|mcts|fixed ...

`--mask uniform` samples an integer comb of columns (every accel-th, under the centre block) instead of `cartesian`'s random ones.
`--grappa` starts every set from the map-combined image of its GRAPPA-filled k-space (pnp_grappa_weights / pnp_grappa_apply: the missing
columns synthesised from their acquired neighbours with weights calibrated on the set's own centre) instead of the zero-filled ATy0;
the data fidelity keeps the measured y0 and the mask.  It runs after --prewhiten and --compress, before the maps are estimated, and
takes a comb (--mask uniform).

`--compress V` mixes each set's C coils down to V virtual coils before the solver sees them (coil compression: the leading eigenvectors
of the channel covariance of the calibration block, per slice, pnp_coil_compress_matrix / pnp_coil_compress_apply); every cost of the
multi-coil stage is linear in the coils it is handed.  With `--sens true` the analytic maps are mixed by the same matrices; with
`--sens estimate` the maps are estimated from the compressed k-space.  With --residuals each line carries `compress_energy`, the share of
the block's energy the kept virtual coils hold (mean over the set).

`--sens estimate` does not hand the solver the maps that generated the measurements: the maps are estimated on the device from the
fully sampled centre of each set's own y0 (pnp_estimate_sens; the block is the largest one the set's mask samples completely, or
--acs).  `--sens espirit` estimates them by ESPIRiT instead (pnp_espirit_sens: at most 16 coils after --compress; the block is cropped to
24 x 24; --sens-window and --sens-thresh apply as well).  The initial iterate x0 stays the one the set brings.

The classical baseline beside the U-Net: `--prior tv [--tv-scale 1.0] [--tv-iters 20]` runs every mode's x-update as total variation
(Chambolle's dual projection with weight tv-scale * sigma_d, pnp_set_prior) on k-space-only handles: no --denoiser-ckpt, no weights:

    ... --prior tv fixed --mu 0.3 --sigma-start 50 --sigma-end 5 --max_iter 30

The other classical baseline: `--prior haar [--haar-scale 1.0] [--haar-levels 3] [--haar-mode ti|ortho]` runs the x-update as Haar wavelet
shrinkage with threshold haar-scale * sigma_d (pnp_set_prior_haar; ti = translation-invariant, fully cycle-spun; ortho = the decimated
transform), again on k-space-only handles without weights:

    ... --prior haar fixed --mu 0.3 --sigma-start 50 --sigma-end 5 --max_iter 30

Multi-GPU (BASELINE configs[2]): launch the same command under `python -m torch.distributed.run --nproc-per-node N
--master-addr 127.0.0.1 -m dt4image_restoration_amd.cli ... eval|mcts|flex ...`: every rank takes a contiguous shard of each
set's images (drivers/sharded.py), the per-image PSNR / stop iteration are gathered over RCCL, rank 0 prints.

Differences: `train` is out of scope; checkpoint and data locations are options instead of
hard-coded paths (main.py:175,178,181-183); without `--data` the run uses the seeded synthetic problems and without
`--denoiser-ckpt` / `--policy-ckpt` the seeded stand-in weights (the real ones are external downloads); images of one
directory are evaluated as ONE batch instead of `DataLoader(batch_size=1)` (main.py:232, eval.py:232).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch


def _denoiser(args):
    """The regulariser object of the run: the U-Net (checkpoint or seeded stand-in), or under --prior tv / haar the weightless TV / Haar
    denoiser."""
    if args.prior == "haar":
        from .denoiser import HaarDenoiser2D
        return HaarDenoiser2D(scale=args.haar_scale, levels=args.haar_levels, mode=args.haar_mode)
    if args.prior == "tv":
        from .denoiser import TVDenoiser2D
        return TVDenoiser2D(scale=args.tv_scale, iters=args.tv_iters)
    from .denoiser import UNetDenoiser2D
    return UNetDenoiser2D(ckpt_path=args.denoiser_ckpt) if args.denoiser_ckpt else UNetDenoiser2D.seeded(args.seed)


def _build(args, mode):
    from . import weights
    from .env import PnPEnv
    from .policy import DecisionTransformer, DecisionTransformerConfig
    model = DecisionTransformer(DecisionTransformerConfig(block_size=args.block_size, n_embeds=args.n_embeds, mode=mode))
    if args.policy_ckpt:
        model.load_state_dict(torch.load(args.policy_ckpt, map_location="cpu"))
    else:
        model.load_state_dict(weights.generate_policy_weights(model, args.seed, t_bias=-1.0, head_gain=8.0))
    den = _denoiser(args)
    scorer = (lambda st: 1.0 / (1e-3 + (st["x"] - torch.nn.functional.avg_pool2d(st["x"], 3, 1, 1)).pow(2).mean(dim=(1, 2, 3))))
    env = PnPEnv(max_episode_step=30, denoiser=den, device_type="cuda", no_ref_scorer=None, cg_iters=args.cg_iters,
                 nufft_width=args.nufft_width, nufft_grid=args.nufft_grid, nc_normal=args.nc_normal,
                 offres_mc=bool(getattr(args, "b0_coils", 0)), offres_normal=getattr(args, "b0_normal", "nufft"))
    if getattr(args, "scorer", "stub") == "neg_dc":            # minus the k-space data misfit of the rollout's final iterate (pnp_residuals)
        scorer = (lambda st: -env.residuals(st, dc=True)[:, 5])
    return model, env, scorer


def _mat(batch):
    """Batch dict -> tensors; what the device acquisition returns stays where it is."""
    return {k: v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v)) for k, v in batch.items()}


def _tasks(args):
    from . import acquisition, data as D
    tasks = [t for t in (args.tasks.split(",") if args.tasks else D.OPTIMAL_TASKS) if t]
    for t in tasks:
        acquisition.parse_task(t)
    return tasks


def _psi(args):
    """--noise-cov RHO[,GAIN_SPREAD]: the channel noise covariance of the run's --coils problems (synthetic.noise_cov_model), or None."""
    if not args.noise_cov:
        return None
    from . import synthetic
    return synthetic.noise_cov_model(args.coils, args.noise_cov[0], args.noise_cov[1], args.seed)


def _prewhitened(args, env, batch):
    """--prewhiten: the batch with its y0 (and, under --sens true, its maps) mixed by W = L^-1 of the covariance measured on a noise-only
    scan (acquisition.prewhiten).  The scan has the run's covariance at the level that makes the mean channel variance 1, so the data
    keep their overall scale (and --mu its meaning); x0 stays the one the set brings."""
    if not args.prewhiten:
        return batch
    from . import acquisition
    batch = dict(batch)
    psi = _psi(args)
    scan = acquisition.noise_scan(env, args.coils, acquisition.SCAN_SAMPLES, noise_cov=psi, sigma_n=acquisition.unit_scan_sigma(psi),
                                  seed=args.seed + acquisition.SCAN_SEED)
    y, sens, _, _ = acquisition.prewhiten(env, batch["y0"], scan, sens=batch.get("sens") if args.sens == "true" else None)
    batch["y0"] = torch.view_as_real(y)
    if sens is not None:
        batch["sens"] = sens
    return batch


def _compressed(args, env, batch):
    """--compress V: the batch with its y0 (and, under --sens true, its maps) mixed down to V virtual coils on the device."""
    if not args.compress:
        return batch
    from . import acquisition
    batch = dict(batch)
    try:
        r = acquisition.compress_coils(env, batch["y0"], mask=batch["mask"], acs=args.acs, out_coils=args.compress,
                                       sens=batch.get("sens") if args.sens == "true" else None)
    except ValueError as e:                                    # a mask without a sampled centre, a block that does not fit
        raise SystemExit(f"--compress: {e}")
    batch["y0"] = torch.view_as_real(r["y0"])
    if "sens" in r:
        batch["sens"] = r["sens"]
    if getattr(args, "residuals", False):                      # reporting only: one host read per set
        eig = r["eig"].double()
        args.compress_energy.append(float((eig[:, :args.compress].sum(dim=1) / eig.sum(dim=1).clamp_min(1e-300)).mean()))
    return batch


def _with_sens(args, env, batch):
    """--prewhiten, then --compress, then --sens estimate / espirit: the batch with its coil maps replaced by the estimate from its own y0 and mask (on the
    device)."""
    batch = _compressed(args, env, _prewhitened(args, env, batch))
    filled = None
    if args.grappa:
        from . import acquisition
        try:
            filled = acquisition.grappa(env, batch["y0"], batch["mask"], kernel=tuple(args.grappa_kernel), lam=args.grappa_lambda)["y0"]
        except ValueError as e:                                # a mask that is no comb, a block that holds no kernel
            raise SystemExit(f"--grappa: {e}")
    if args.sens == "true":
        return _grappa_start(env, batch, filled)
    from . import acquisition
    batch = dict(batch)
    try:
        batch["sens"] = acquisition.estimate_sens(env, batch["y0"], mask=batch["mask"], acs=args.acs, window=args.sens_window,
                                                  thresh=args.sens_thresh, method="espirit" if args.sens == "espirit" else "lowres",
                                                  ksize=args.espirit_kernel, sv_thresh=args.espirit_sv, crop=args.espirit_crop,
                                                  iters=args.espirit_iters)
    except ValueError as e:                                    # a mask without a sampled centre, a block that does not fit
        raise SystemExit(f"--sens {args.sens}: {e}")
    return _grappa_start(env, batch, filled)


def _grappa_start(env, batch, filled):
    """--grappa: the batch with x0 replaced by max(Re sum_c conj(S_c) ifft_c(filled_c), 0), the map-combined image of its GRAPPA-filled
    k-space `filled`, with the maps the run uses; y0, ATy0 and the mask stay what was measured."""
    if filled is None:
        return batch
    batch = dict(batch)
    n, c, h, w = (int(v) for v in filled.shape)
    eng = env._engine_for(n, h, w, filled.device)
    sens = torch.as_tensor(batch["sens"]).to(filled.device, torch.complex64)
    from . import acquisition
    x = (sens.conj() * acquisition.coil_images(eng, filled)).sum(dim=1, keepdim=True).real.clamp_min(0.0)
    batch["x0"] = torch.stack([x, torch.zeros_like(x)], dim=-1)
    return batch


def _nc_kwargs(args):
    """--traj radial: what `acquisition.task_problem` needs for the non-Cartesian acquisition of a task."""
    kw = dict(mask_kind=f"{args.traj}-nc", spokes=args.spokes, nc_weights=args.nc_weights, nufft_width=args.nufft_width,
              nufft_grid=args.nufft_grid, coils=args.nc_coils, interleaves=args.interleaves, petals=args.petals, dcf_iters=args.dcf_iters)
    if args.b0 is not None:                                  # --b0: the acquisition under a field map and the off-resonance stage
        kw.update(b0_hz=args.b0, readout_ms=args.readout_ms, b0_segments=args.b0_segments)
        if getattr(args, "b0_interp", "linear") != "linear": # --b0-interp ls: the least-squares temporal interpolator
            kw.update(b0_interp=args.b0_interp)
        if getattr(args, "b0_map", "true") != "true":        # --b0-map estimate: the solver gets a map estimated from a two-echo scan
            kw.update(b0_map=args.b0_map, b0_dte_ms=args.b0_dte, b0_beta=0.05 if args.b0_beta is None else args.b0_beta,
                      b0_iters=200 if args.b0_iters is None else args.b0_iters)
        if getattr(args, "b0_coils", 0):                     # --b0-coils C: the multi-coil acquisition under the field map, coils x segments stage
            kw.update(b0_coils=args.b0_coils)
    return kw


def _sets(args, flex_target=None, env=None):
    """(name, number of images, load(start, stop) -> (batch dict, task tokens)) per evaluation set."""
    from . import _lib, acquisition, data as D, synthetic
    if args.traj and args.data:
        raise SystemExit("--traj: the reference's .mat layout (--data) holds Cartesian k-space and a mask; use the synthetic sets or --gt")
    if args.traj:                                            # a true radial acquisition of the --gt images, or of make_problem's phantoms
        def nc_load(images, task, a, b):
            try:
                batch = acquisition.task_problem(task, images(a, b), env, seed=args.seed, first_slice=a, **_nc_kwargs(args))
            except (ValueError, RuntimeError) as e:          # a grid the rule refuses, a slice side without a grid
                raise SystemExit(f"--traj {args.traj}: task {task}: {e}")
            if args.nc_normal == "toeplitz":                 # refused here, in the library's words, before any episode is set up
                why = _lib.toeplitz_size_error("pnp_toeplitz_plan", *batch["gt"].shape[-2:])
                if why:
                    raise SystemExit(f"--nc-normal toeplitz: task {task}: {why}")
            if getattr(args, "b0_normal", "nufft") == "toeplitz":   # likewise: the slice size and the plan's spectra are known here
                interp = "ls" if batch.get("b0_interp") in ("ls", _lib.OFFRES_INTERPOLATORS["ls"]) else "linear"
                why = (_lib.toeplitz_size_error("pnp_offres_tz_plan", *batch["gt"].shape[-2:])
                       or _lib.offres_tz_pairs_error("pnp_offres_tz_plan", interp, int(batch["segments"])))
                if why:
                    raise SystemExit(f"--b0-normal toeplitz: task {task}: {why}")
            return batch, D.task_tokens([task] * (b - a), flex_target)
        if args.gt:
            for d in args.gt:
                for task in _tasks(args):
                    images = (lambda a, b, d=d: D.load_gt_dir(d, limit=args.limit, start=a, stop=b)[0])
                    yield f"{d} {task} {args.traj}-nc", D.count_gt_dir(d, args.limit), (lambda a, b, im=images, t=task: nc_load(im, t, a, b))
        else:
            for accel, sig in ((4, 10), (8, 10)):
                images = (lambda a, b, accel=accel: np.stack([synthetic.phantom(args.size, args.size, args.seed + accel + i)
                                                              for i in range(a, b)]).astype(np.float32))
                yield (f"synthetic {accel}x_{sig} {args.traj}-nc", args.limit or 7,
                       (lambda a, b, im=images, t=f"{accel}x_{sig}": nc_load(im, t, a, b)))
        return
    if args.gt:
        for d in args.gt:
            for task in _tasks(args):
                def load(a, b, d=d, task=task):
                    gt, _ = D.load_gt_dir(d, limit=args.limit, start=a, stop=b)
                    mask = None
                    if args.mask == "uniform":                     # a task whose acceleration does not divide the width has no comb
                        try:
                            mask = acquisition.make_mask(gt.shape[-2], gt.shape[-1], acquisition.parse_task(task)[0], "uniform", args.seed)
                        except ValueError as e:
                            raise SystemExit(f"--mask uniform: task {task}: {e}")
                    batch = acquisition.task_problem(task, gt, env, seed=args.seed, first_slice=a, mask_kind=args.mask, mask=mask,
                                                    coils=args.coils, noise_cov=_psi(args))
                    return _with_sens(args, env, batch), D.task_tokens([task] * (b - a), flex_target)
                yield f"{d} {task}", D.count_gt_dir(d, args.limit), load
    elif args.data:
        if args.coils:
            raise SystemExit("--coils: the reference's .mat layout (--data) has no coil axis; use the synthetic sets or --gt")
        for d in args.data:
            def load(a, b, d=d):
                batch, tasks = D.load_dir(d, limit=args.limit, start=a, stop=b)
                return batch, D.task_tokens(tasks, flex_target)
            yield d, len(D.list_dir(d, args.limit)), load
    else:
        for accel, sig in ((4, 10), (8, 10)):
            def load(a, b, accel=accel, sig=sig):
                # the synthetic sets are radial; a --sens estimate run may ask for --mask cartesian, whose calibration block is H x the
                # centre columns, and --mask uniform (the comb --grappa works on) always applies (None: the radial mask of make_problem, as
                # every other run gets)
                try:
                    mask = acquisition.make_mask(args.size, args.size, accel, args.mask, args.seed) \
                        if args.mask == "uniform" or (args.sens != "true" and args.mask != "radial") else None
                except ValueError as e:                        # --mask uniform at a size the acceleration does not divide
                    raise SystemExit(f"--mask {args.mask}: {e}")
                if args.acquire == "device" or args.noise_cov:   # (correlated noise is mixed on the device) make_problem's phantoms, mask and noise; the transforms on the GPU
                    gt = np.stack([synthetic.phantom(args.size, args.size, args.seed + accel + i) for i in range(a, b)])
                    sens = synthetic.coil_maps(args.coils, args.size, args.size).astype(np.complex64) if args.coils else None
                    p = acquisition.simulate(env, gt.astype(np.float32), synthetic.radial_mask(args.size, args.size, accel) if mask is None else mask,
                                             sig / 255.0, args.seed + accel, first_slice=a, sens=sens, noise_cov=_psi(args))
                    return (_with_sens(args, env, p) if args.coils else p), D.task_tokens([f"{accel}x_{sig}"] * (b - a), flex_target)
                if args.coils:
                    p = synthetic.make_problem_mc(b - a, args.size, args.size, args.coils, accel=accel, sigma_n=sig / 255.0,
                                                  seed=args.seed + accel, first_slice=a, mask=mask)
                    return _with_sens(args, env, p), D.task_tokens([f"{accel}x_{sig}"] * (b - a), flex_target)
                p = synthetic.make_problem(b - a, args.size, args.size, accel=accel, sigma_n=sig / 255.0, seed=args.seed + accel,
                                           first_slice=a)
                return p, D.task_tokens([f"{accel}x_{sig}"] * (b - a), flex_target)
            yield f"synthetic {accel}x_{sig}", args.limit or 7, load


def acquired_name(task: str, image: str) -> str:
    """File name of one acquired image: carries `_<accel>_<sigma>_` first, so that `data.task_from_filename` (the reference's
    `extract_task`, which takes the FIRST `<digits>_<digits>`) reads the task back whatever digits the image name holds."""
    accel, sig = task.split("x_")
    return f"gt_{accel}_{sig}_{image}.mat"


def _acquire(args):
    """`acquire`: every image of every --gt folder through pnp_acquire for every task, written by `data.save_mat` into
    <out>/<task>/ (one folder per task, as the reference's data is laid out); with several folders, <out>/<folder name>/<task>/."""
    from . import acquisition, data as D
    from .engine import PnPEngine
    if not args.gt:
        raise SystemExit("acquire: --gt DIR is required")
    out, engines = [], {}
    tasks, step = _tasks(args), max(args.batch, 1)
    for d in args.gt:
        index = D.gt_index(d, args.limit)                      # the folder's headers, read once
        total = sum(n for _, n, _ in index)
        dsts = {t: os.path.join(args.out, t) if len(args.gt) == 1 else os.path.join(args.out, os.path.basename(os.path.normpath(d)), t)
                for t in tasks}
        for dst in dsts.values():
            os.makedirs(dst, exist_ok=True)
        for a in range(0, total, step):                        # every batch is read once and acquired for every task
            gt, names = D.load_gt_dir(d, limit=args.limit, start=a, stop=min(a + step, total), index=index)
            key = gt.shape[0], gt.shape[-2], gt.shape[-1]
            if key not in engines:
                engines[key] = PnPEngine(*key, denoiser=False)
            for task in tasks:
                try:
                    p = acquisition.task_problem(task, gt, engines[key], seed=args.seed, first_slice=a,
                                                 **(_nc_kwargs(args) if args.traj else dict(mask_kind=args.mask)))
                except ValueError as e:
                    if args.traj:
                        raise SystemExit(f"--traj {args.traj}: task {task}: {e}")
                    if args.mask != "uniform":
                        raise
                    raise SystemExit(f"--mask uniform: task {task}: {e}")
                host = {k: v.cpu().numpy() for k, v in p.items()}
                for i, name in enumerate(names):
                    D.save_mat(os.path.join(dsts[task], acquired_name(task, name)), host, i)
        for task in tasks:
            out.append({"set": d, "task": task, "n": total, "dir": dsts[task], "mask": f"{args.traj}-nc" if args.traj else args.mask})
            print(json.dumps(out[-1]), flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="PnP-ADMM CS-MRI restoration with a decision-transformer policy (MI355X)")
    ap.add_argument("--block_size", type=int, required=True)
    ap.add_argument("--n_embeds", type=int, required=True)
    ap.add_argument("--denoiser-ckpt", default=None)
    ap.add_argument("--policy-ckpt", default=None)
    ap.add_argument("--data", nargs="*", default=None, help="directories of .mat files (one batch each)")
    ap.add_argument("--gt", nargs="+", default=None, help="directories of ground-truth images (.npy / .mat with a `gt` key), "
                    "acquired on the device: one set per (directory, task)")
    ap.add_argument("--tasks", default=None, help="comma-separated tasks for --gt, e.g. 4x_10,8x_15 (default: the reference's nine)")
    ap.add_argument("--mask", choices=("radial", "cartesian", "uniform"), default="radial", help="sampling mask of the --gt sets "
                    "(cartesian: and of the synthetic sets of a --sens estimate run; uniform: of the synthetic sets too); uniform: every accel-th "
                    "column under a centre block of at least 3 accel + 4 columns")
    ap.add_argument("--grappa", action="store_true", help="start a --coils run from the map-combined image of the GRAPPA-filled k-space "
                    "(needs a comb: --mask uniform)")
    ap.add_argument("--grappa-kernel", type=int, nargs=2, default=(5, 4), metavar=("BY", "BX"), help="--grappa: rows (1, 3, 5 or 7) by "
                    "acquired columns (2 or 4) of the interpolation kernel, coils * BY * BX <= 512")
    ap.add_argument("--grappa-lambda", type=float, default=1e-2, metavar="L", help="--grappa: Tikhonov weight of the calibration, relative "
                    "to the mean diagonal of its normal matrix (in [0, 1])")
    ap.add_argument("--acquire", choices=("cpu", "device"), default="cpu",
                    help="where the synthetic sets are acquired: synthetic.make_problem on the CPU, or pnp_acquire on the GPU")
    ap.add_argument("--limit", type=int, default=None, help="images per directory (default 7: the reference averages the first 7; "
                    "`acquire` defaults to all)")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--coils", type=int, default=0, help="multi-coil (SENSE) problems with this many analytic coil maps (1..32; "
                    "default 0: single-coil)")
    ap.add_argument("--cg-iters", type=int, default=8, help="conjugate-gradient iterations per step of a multi-coil or --traj problem (1..64)")
    ap.add_argument("--traj", choices=("radial", "spiral", "rosette"), default=None, help="a non-Cartesian acquisition: golden-angle radial "
                    "spokes, interleaved spirals or a rosette, whose samples lie off the grid (NUFFT data fidelity, CG solve), single-coil: the "
                    "synthetic sets or --gt, not --data")
    ap.add_argument("--interleaves", type=int, default=None, metavar="L", help="--traj spiral: interleaves (default: ceil(H / (2 acceleration)) "
                    "of the task)")
    ap.add_argument("--petals", type=int, default=None, metavar="P", help="--traj rosette: petals (default: an odd count near H / acceleration)")
    ap.add_argument("--dcf-iters", type=int, default=30, metavar="I", help="--traj: iterations of the density weights of --nc-weights pipe, and "
                    "of dcf on a spiral or a rosette (1..256)")
    ap.add_argument("--nc-coils", type=int, default=0, metavar="C", help="--traj radial: non-Cartesian SENSE, the radial acquisition of C "
                    "coils with analytic coil maps (1..32; default 0: single-coil)")
    ap.add_argument("--nc-normal", choices=("nufft", "toeplitz"), default="nufft", help="--traj radial: the normal operator A^H W A inside the "
                    "CG of eval / flex / mcts / fixed: the NUFFT pair, or its Toeplitz form - two transforms of the 2H x 2W grid and a multiply "
                    "by a spectrum built once per trajectory (sides up to 512)")
    ap.add_argument("--spokes", type=int, default=None, metavar="S", help="--traj radial: spokes (default: ceil(H / acceleration) of the task)")
    ap.add_argument("--nufft-width", type=int, choices=(4, 6, 8), default=6, help="--traj: width of the gridding kernel in grid points")
    ap.add_argument("--nufft-grid", type=int, nargs=2, default=None, metavar=("GH", "GW"), help="--traj: sides of the oversampled grid (sides "
                    "the k-space stage accepts, at least 1.25 x the slice; default: the smallest such)")
    ap.add_argument("--nc-weights", choices=("none", "dcf", "pipe"), default="dcf", help="--traj: sample weights of the data term and of ATy0: "
                    "none; pipe, the density weights iterated on the device for any trajectory; dcf, the analytic ramp on radial spokes and "
                    "the iterated weights on a spiral or a rosette")
    ap.add_argument("--b0", type=float, default=None, metavar="HZ", help="--traj: acquire under a smooth main-field inhomogeneity map of at most "
                    "HZ hertz and reconstruct with the time-segmented off-resonance stage (eval / flex / mcts / fixed; single-coil, NUFFT normal "
                    "operator); needs --readout-ms")
    ap.add_argument("--readout-ms", type=float, default=None, metavar="T", help="--b0: the length of every readout (spoke, interleaf, shot) in ms")
    ap.add_argument("--b0-segments", default="auto", metavar="L|auto", help="--b0: time segments, 1..32, or auto: the smallest count whose "
                    "interpolation error stays within 1e-3, at most 32")
    ap.add_argument("--b0-interp", choices=("linear", "ls"), default="linear", help="--b0: the temporal interpolator between the time segments: "
                    "linear (two segments per sample), or ls: least-squares coefficients for every segment, fitted over the map's band - the "
                    "same accuracy from about a quarter of the segments")
    ap.add_argument("--b0-normal", choices=("nufft", "toeplitz"), default="nufft", help="--b0: the normal operator A^H W A inside the CG of the "
                    "off-resonance stage, single-coil or --b0-coils: the gridding pair, or its Toeplitz form - 2 L transforms of the 2H x 2W grid "
                    "and one mix with spectra built once per trajectory, times plan and weights (sides up to 512; at most 136 spectra: 32 "
                    "segments linear, 16 with --b0-interp ls)")
    ap.add_argument("--b0-coils", type=int, default=0, metavar="C", help="--b0: the multi-coil acquisition under the field map, C coils with "
                    "analytic coil maps (1..32; default 0: single-coil), reconstructed with the coils x segments off-resonance stage (eval / flex / "
                    "mcts / fixed; not with --nc-coils, --coils, --nc-normal toeplitz or --b0-map estimate)")
    ap.add_argument("--b0-map", choices=("true", "estimate"), default="true", help="--b0: the field map the solver is given: the map that made "
                    "the data, or one estimated on the device from a simulated two-echo scan of the same object (regularised fit, no phase "
                    "unwrapping)")
    ap.add_argument("--b0-dte", type=float, default=None, metavar="MS", help="--b0-map estimate: echo spacing of the field map scan in ms "
                    "(default: the largest with 2 pi HZ dte <= 0.8 pi); HZ * MS must stay below 500")
    ap.add_argument("--b0-beta", type=float, default=None, metavar="B", help="--b0-map estimate: roughness weight of the fit (default 0.05)")
    ap.add_argument("--b0-iters", type=int, default=None, metavar="K", help="--b0-map estimate: sweeps of the fit, 0..4096 (default 200; 0: the "
                    "raw phase difference)")
    ap.add_argument("--sens", choices=("true", "estimate", "espirit"), default="true", help="coil maps of a --coils run: the analytic maps that "
                    "generated the measurements, or maps estimated on the device from the calibration block of each set's own y0 (estimate: "
                    "the low-resolution estimate; espirit: ESPIRiT, at most 16 coils)")
    ap.add_argument("--espirit-kernel", type=int, default=6, metavar="K", help="--sens espirit: side of the calibration kernels (2..8, coils * "
                    "K^2 <= 512)")
    ap.add_argument("--espirit-sv", type=float, default=0.02, help="--sens espirit: singular values above this fraction of the largest span "
                    "the signal space (in (0, 1))")
    ap.add_argument("--espirit-crop", type=float, default=0.9, help="--sens espirit: pixels whose eigenvalue is not above this get zero maps "
                    "(in [0, 1))")
    ap.add_argument("--espirit-iters", type=int, default=16, help="--sens espirit: power iterations per pixel (1..64)")
    ap.add_argument("--sens-window", choices=("hann", "box"), default="hann", help="window of the calibration block (--sens estimate)")
    ap.add_argument("--sens-thresh", type=float, default=0.05, help="--sens estimate: pixels whose root-sum-of-squares is not above this "
                    "fraction of the slice's largest get zero maps (in [0, 1))")
    ap.add_argument("--compress", type=int, default=0, metavar="V", help="coil compression of a --coils run: the solver gets the V "
                    "strongest virtual coils of each set (1..--coils; default 0: no compression)")
    ap.add_argument("--noise-cov", default=None, metavar="RHO[,GAIN_SPREAD]", help="correlated receiver noise for the --coils problems: "
                    "neighbouring channels correlate by RHO (in [0, 1)) and the channel gains ramp from 1 to GAIN_SPREAD (>= 1, default 1); "
                    "the synthetic sets are then acquired on the device")
    ap.add_argument("--prewhiten", action="store_true", help="measure the channel noise covariance on a noise-only scan and whiten y0 (and "
                    "the maps of --sens true) on the device, before --compress and --sens estimate|espirit")
    ap.add_argument("--acs", type=int, nargs=2, default=None, metavar=("H", "W"), help="--sens estimate / --compress: even sides of the centred "
                    "calibration block (default: the largest block the mask samples completely)")
    ap.add_argument("--prior", choices=("unet", "tv", "haar"), default="unet", help="the x-update of eval / flex / mcts / fixed: the U-Net, total "
                    "variation or Haar wavelet shrinkage (the last two need no --denoiser-ckpt and load no weights)")
    ap.add_argument("--tv-scale", type=float, default=1.0, help="--prior tv: the TV weight is this times sigma_d (finite, >= 0)")
    ap.add_argument("--tv-iters", type=int, default=20, help="--prior tv: dual projection steps per x-update (1..64)")
    ap.add_argument("--haar-scale", type=float, default=1.0, help="--prior haar: the threshold is this times sigma_d (finite, >= 0)")
    ap.add_argument("--haar-levels", type=int, default=3, help="--prior haar: levels of the transform (1..4)")
    ap.add_argument("--haar-mode", default="ti", help="--prior haar: ti (translation-invariant, the default) or ortho (decimated)")
    ap.add_argument("--seed", type=int, default=0)
    sub = ap.add_subparsers(dest="mode", required=True)
    for name in ("eval", "mcts"):
        sp = sub.add_parser(name)
        sp.add_argument("--rtg", type=float, default=10.0)
        sp.add_argument("--max_timesteps", type=int, default=30)
        if name == "mcts":
            sp.add_argument("--rollouts", type=int, default=30)
            sp.add_argument("--scorer", choices=("stub", "neg_dc"), default="stub",
                            help="no-reference score of a rollout: the smoothness stub, or minus the k-space data misfit")
        else:
            sp.add_argument("--residuals", action="store_true", help="add `primal` and `dc` of the final iterates to each line")
    sp = sub.add_parser("flex")
    sp.add_argument("--max_timesteps", type=int, default=30)
    sp.add_argument("--residuals", action="store_true", help="add `primal` and `dc` of the final iterates to each line")
    sp = sub.add_parser("fixed", help="plain PnP-ADMM: fixed mu, geometric sigma_d schedule, stopped by delta <= tol")
    sp.add_argument("--mu", type=float, default=0.3)
    sp.add_argument("--sigma-start", type=float, default=50.0, help="sigma_d of the first iteration, in /255 units")
    sp.add_argument("--sigma-end", type=float, default=5.0, help="sigma_d of iteration max_iter (geometric decay), in /255 units")
    sp.add_argument("--tol", type=float, default=None, help="stop a slice once delta <= tol (default: run max_iter iterations)")
    sp.add_argument("--max_iter", type=int, default=30)
    sp.add_argument("--dc", action="store_true", help="add the final k-space data misfit to each line")
    sp = sub.add_parser("acquire", help="write the reference's evaluation .mat files for a folder of ground-truth images")
    sp.add_argument("--gt", nargs="+", default=argparse.SUPPRESS, help="directories of ground-truth images")
    sp.add_argument("--out", required=True, help="output directory: one sub-folder per task")
    sp.add_argument("--batch", type=int, default=16, help="images acquired per call")
    args = ap.parse_args(argv)
    if args.limit is None:
        args.limit = 0 if args.mode == "acquire" else 7
    if args.coils and not 1 <= args.coils <= 32:
        raise SystemExit(f"--coils must be 1..32, got {args.coils}")
    if not 1 <= args.cg_iters <= 64:
        raise SystemExit(f"--cg-iters must be 1..64, got {args.cg_iters}")
    if args.b0_coils:
        if not 1 <= args.b0_coils <= 32:
            raise SystemExit(f"--b0-coils must be 1..32, got {args.b0_coils}")
        if args.b0 is None:
            raise SystemExit("--b0-coils needs --b0 (the multi-coil acquisition under a field map)")
        if args.coils:
            raise SystemExit("--b0-coils with --coils: refused - --coils selects the Cartesian multi-coil chain")
        if args.nc_coils:
            raise SystemExit("--b0-coils with --nc-coils: refused - --b0-coils is the coil count of the off-resonance acquisition")
        if args.nc_normal == "toeplitz":
            raise SystemExit("--b0-coils with --nc-normal toeplitz: the off-resonance stage has no Toeplitz form")
        if args.b0_map != "true":
            raise SystemExit("--b0-coils with --b0-map estimate: estimating the field map inside a multi-coil episode is out of scope")
    if args.traj:
        if args.coils:
            raise SystemExit("--traj with --coils: refused - --coils selects the Cartesian multi-coil chain; the multi-coil radial acquisition "
                             "is --traj radial --nc-coils C")
        if args.nc_coils and not 1 <= args.nc_coils <= 32:
            raise SystemExit(f"--nc-coils must be 1..32, got {args.nc_coils}")
        if args.spokes is not None and args.spokes < 1:
            raise SystemExit(f"--spokes must be >= 1, got {args.spokes}")
        for flag, value, traj in (("--spokes", args.spokes, "radial"), ("--interleaves", args.interleaves, "spiral"),
                                  ("--petals", args.petals, "rosette")):
            if value is not None and args.traj != traj:
                raise SystemExit(f"{flag} needs --traj {traj} (got --traj {args.traj})")
            if value is not None and value < 1:
                raise SystemExit(f"{flag} must be >= 1, got {value}")
        if not 1 <= args.dcf_iters <= 256:
            raise SystemExit(f"--dcf-iters must be 1..256, got {args.dcf_iters}")
        if args.grappa or args.mask != "radial":
            raise SystemExit("--traj takes no --mask / --grappa: its samples are a trajectory, not a mask")
        if args.b0 is not None:
            if args.readout_ms is None or not (np.isfinite(args.readout_ms) and args.readout_ms > 0.0):
                raise SystemExit(f"--b0 needs --readout-ms T with T > 0, got {args.readout_ms}")
            if not (np.isfinite(args.b0) and args.b0 >= 0.0):
                raise SystemExit(f"--b0 must be finite and >= 0, got {args.b0}")
            if args.nc_coils:
                raise SystemExit("--b0 with --nc-coils: the off-resonance stage is single-coil")
            if args.nc_normal == "toeplitz":
                raise SystemExit("--b0 with --nc-normal toeplitz: the off-resonance stage has no Toeplitz form")
            if args.b0_normal == "toeplitz" and args.mode == "acquire":
                raise SystemExit("acquire runs no CG: drop --b0-normal toeplitz")
            if args.mode == "acquire":
                raise SystemExit("--b0 is for eval / flex / mcts / fixed")
            if args.b0_segments != "auto":
                if not str(args.b0_segments).isdigit() or not 1 <= int(args.b0_segments) <= 32:
                    raise SystemExit(f"--b0-segments must be 1..32 or auto, got {args.b0_segments}")
                args.b0_segments = int(args.b0_segments)
            if args.b0_normal == "toeplitz":                 # what is known here is refused here, in the library's words
                from ._lib import offres_tz_pairs_error, toeplitz_size_error
                why = None if getattr(args, "gt", None) else toeplitz_size_error("pnp_offres_tz_plan", args.size, args.size)
                if not why and args.b0_segments != "auto":
                    why = offres_tz_pairs_error("pnp_offres_tz_plan", args.b0_interp, args.b0_segments)
                if why:
                    raise SystemExit(f"--b0-normal toeplitz: {why}")
        elif args.readout_ms is not None or args.b0_segments != "auto":
            raise SystemExit("--readout-ms / --b0-segments need --b0")
        elif args.b0_interp != "linear":
            raise SystemExit("--b0-interp needs --b0")
        if args.nc_normal == "toeplitz" and args.mode == "acquire":
            raise SystemExit("acquire runs no CG: drop --nc-normal toeplitz")
        if args.nc_normal == "toeplitz" and not getattr(args, "gt", None):      # the synthetic sets: the size is known here
            from ._lib import toeplitz_size_error
            why = toeplitz_size_error("pnp_toeplitz_plan", args.size, args.size)
            if why:
                raise SystemExit(f"--nc-normal toeplitz: {why}")
    elif args.nc_normal != "nufft":
        raise SystemExit(f"--nc-normal {args.nc_normal} needs --traj radial")
    elif args.nc_coils:
        raise SystemExit(f"--nc-coils needs --traj radial (got --nc-coils {args.nc_coils} without it)")
    elif args.spokes is not None or args.nufft_grid is not None or args.nufft_width != 6 or args.nc_weights != "dcf":
        raise SystemExit("--spokes / --nufft-width / --nufft-grid / --nc-weights need --traj radial")
    elif args.interleaves is not None:
        raise SystemExit("--interleaves needs --traj spiral")
    elif args.petals is not None:
        raise SystemExit("--petals needs --traj rosette")
    elif args.dcf_iters != 30:
        raise SystemExit("--dcf-iters needs --traj")
    elif args.b0 is not None or args.readout_ms is not None or args.b0_segments != "auto":
        raise SystemExit("--b0 / --readout-ms / --b0-segments need --traj")
    elif args.b0_interp != "linear":
        raise SystemExit("--b0-interp needs --b0")
    if args.b0 is None and args.b0_normal != "nufft":
        raise SystemExit(f"--b0-normal {args.b0_normal} needs --b0")
    if args.b0 is None:
        if args.b0_map != "true" or args.b0_dte is not None or args.b0_beta is not None or args.b0_iters is not None:
            raise SystemExit("--b0-map / --b0-dte / --b0-beta / --b0-iters need --b0")
    elif args.b0_map == "true":
        if args.b0_dte is not None or args.b0_beta is not None or args.b0_iters is not None:
            raise SystemExit("--b0-dte / --b0-beta / --b0-iters need --b0-map estimate")
    else:
        if args.b0_dte is not None and not (np.isfinite(args.b0_dte) and args.b0_dte > 0.0):
            raise SystemExit(f"--b0-dte must be finite and > 0, got {args.b0_dte}")
        if args.b0_dte is not None and args.b0 * args.b0_dte >= 500.0:
            raise SystemExit(f"--b0-map estimate has no phase unwrapping: --b0 times --b0-dte must stay below 500, got {args.b0} * {args.b0_dte}")
        if args.b0_beta is not None and not (np.isfinite(args.b0_beta) and args.b0_beta > 0.0):
            raise SystemExit(f"--b0-beta must be finite and > 0, got {args.b0_beta}")
        if args.b0_iters is not None and not 0 <= args.b0_iters <= 4096:
            raise SystemExit(f"--b0-iters must be 0..4096, got {args.b0_iters}")
    if args.prior == "tv":
        if not (args.tv_scale >= 0.0 and np.isfinite(args.tv_scale)):
            raise SystemExit(f"--tv-scale must be finite and >= 0, got {args.tv_scale}")
        if not 1 <= args.tv_iters <= 64:
            raise SystemExit(f"--tv-iters must be 1..64, got {args.tv_iters}")
        if args.denoiser_ckpt:
            raise SystemExit("--prior tv loads no weights: drop --denoiser-ckpt")
        if args.mode == "acquire":
            raise SystemExit("acquire has no x-update: drop --prior tv")
    if args.prior == "haar":
        if not (args.haar_scale >= 0.0 and np.isfinite(args.haar_scale)):
            raise SystemExit(f"--haar-scale must be finite and >= 0, got {args.haar_scale}")
        if not 1 <= args.haar_levels <= 4:
            raise SystemExit(f"--haar-levels must be 1..4, got {args.haar_levels}")
        if args.haar_mode not in ("ti", "ortho"):
            raise SystemExit(f"--haar-mode must be ti or ortho, got {args.haar_mode!r}")
        if args.denoiser_ckpt:
            raise SystemExit("--prior haar loads no weights: drop --denoiser-ckpt")
        if args.mode == "acquire":
            raise SystemExit("acquire has no x-update: drop --prior haar")
    if args.noise_cov is not None:
        try:
            v = [float(t) for t in args.noise_cov.split(",")]
        except ValueError:
            v = []
        if len(v) not in (1, 2) or not 0.0 <= v[0] < 1.0 or (len(v) == 2 and not (v[1] >= 1.0 and np.isfinite(v[1]))):
            raise SystemExit(f"--noise-cov takes RHO[,GAIN_SPREAD] with 0 <= RHO < 1 and a finite GAIN_SPREAD >= 1, got {args.noise_cov!r}")
        if not args.coils:
            raise SystemExit("--noise-cov needs --coils: a single-coil problem has one channel")
        if args.mode == "acquire" or args.data:
            raise SystemExit("--noise-cov applies to the synthetic sets and --gt of eval|flex|mcts|fixed")
        args.noise_cov = (v[0], v[1] if len(v) == 2 else 1.0)
    if args.prewhiten and args.mode == "acquire":
        raise SystemExit("--prewhiten applies to eval|flex|mcts|fixed: acquire writes the measurements as they are")
    if args.prewhiten and not args.coils:
        raise SystemExit("--prewhiten needs --coils: there are no channels to whiten on a single-coil problem")
    if args.grappa:
        if args.mode == "acquire":
            raise SystemExit("--grappa applies to eval|flex|mcts|fixed: acquire writes the measurements as they are")
        if not args.coils:
            raise SystemExit("--grappa needs --coils: GRAPPA interpolates across the channels of a multi-coil problem")
        if args.mask != "uniform":
            raise SystemExit(f"--grappa needs a comb of acquired columns: --mask uniform (got --mask {args.mask})")
        by, bx = args.grappa_kernel
        c = args.compress or args.coils
        if by not in (1, 3, 5, 7) or bx not in (2, 4) or c * by * bx > 512:
            raise SystemExit(f"--grappa-kernel takes BY in 1, 3, 5, 7 and BX in 2, 4 with coils * BY * BX <= 512, got {by} {bx} at {c} coils")
        if not 0.0 <= args.grappa_lambda <= 1.0:
            raise SystemExit(f"--grappa-lambda must be in [0, 1], got {args.grappa_lambda}")
    args.compress_energy = []
    if args.compress:
        if not args.coils:
            raise SystemExit("--compress needs --coils: there are no coils to compress on a single-coil problem")
        if not 1 <= args.compress <= args.coils:
            raise SystemExit(f"--compress must be 1..--coils = {args.coils}, got {args.compress}")
        if args.acs is not None and any(v < 2 or v % 2 for v in args.acs):
            raise SystemExit(f"--acs: sides must be even and >= 2, got {args.acs}")
    if args.sens != "true":
        if not args.coils:
            raise SystemExit(f"--sens {args.sens} needs --coils: there are no coil maps to estimate on a single-coil problem")
        if not 0.0 <= args.sens_thresh < 1.0:
            raise SystemExit(f"--sens-thresh must be in [0, 1), got {args.sens_thresh}")
        if args.acs is not None and any(v < 2 or v % 2 for v in args.acs):
            raise SystemExit(f"--acs: sides must be even and >= 2, got {args.acs}")
    if args.sens == "espirit":
        c = args.compress or args.coils
        if c > 16:
            raise SystemExit(f"--sens espirit takes at most 16 coils, got {c}: add --compress V with V <= 16")
        if not 2 <= args.espirit_kernel <= 8 or c * args.espirit_kernel ** 2 > 512:
            raise SystemExit(f"--espirit-kernel must be 2..8 with coils * K^2 <= 512, got {args.espirit_kernel} at {c} coils")
        if not 0.0 < args.espirit_sv < 1.0:
            raise SystemExit(f"--espirit-sv must be in (0, 1), got {args.espirit_sv}")
        if not 0.0 <= args.espirit_crop < 1.0:
            raise SystemExit(f"--espirit-crop must be in [0, 1), got {args.espirit_crop}")
        if not 1 <= args.espirit_iters <= 64:
            raise SystemExit(f"--espirit-iters must be 1..64, got {args.espirit_iters}")
    if args.mode == "acquire":
        if args.coils:
            raise SystemExit("acquire --coils: refused - the reference's .mat layout this command writes has no coil axis")
        return _acquire(args)

    from . import data as D
    from .drivers.greedy import GreedyEvaluator
    from .drivers.mcts import MCTS
    from .drivers.sharded import run_sharded_fixed, run_sharded_greedy, run_sharded_mcts
    out = []
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dist = None
    if world > 1:                                            # one process per GPU under torch.distributed.run
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
    if args.mode == "fixed":
        from .drivers.fixed import FixedScheduleSolver
        from .env import PnPEnv
        den = _denoiser(args)
        env = PnPEnv(max_episode_step=args.max_iter, denoiser=den, device_type="cuda", cg_iters=args.cg_iters,
                     nufft_width=args.nufft_width, nufft_grid=args.nufft_grid, nc_normal=args.nc_normal,
                     offres_mc=bool(getattr(args, "b0_coils", 0)), offres_normal=getattr(args, "b0_normal", "nufft"))
        solver = FixedScheduleSolver(env, max_iter=args.max_iter, tol=args.tol, sync_every=5, dc=args.dc,
                                     device_type=torch.device("cuda", torch.cuda.current_device()))
        t = np.arange(args.max_iter) / max(args.max_iter - 1, 1)
        sigma = (args.sigma_start * (args.sigma_end / args.sigma_start) ** t / 255.0).astype(np.float32)
        for name, total, load in _sets(args, env=env):
            def load_shard(a, b, load=load):
                batch, _ = load(a, b)
                mat = _mat(batch)
                return mat, np.full((b - a, args.max_iter), args.mu, dtype=np.float32), np.tile(sigma, (b - a, 1))
            r = run_sharded_fixed(solver, total, load_shard, sync=torch.cuda.synchronize)
            out.append({"set": name, "n": total, "psnr": float(r.psnr.mean()),
                        "psnr_increment": float((r.psnr - r.initial_psnr).mean()),
                        "mean_stop_iteration": float(r.iterations.float().mean()), "ranks": world,
                        "iterations": [int(v) for v in r.iterations], "delta": float(r.delta.mean()), "primal": float(r.primal.mean())})
            if args.dc:
                out[-1]["dc"] = float(r.dc.mean())
            if rank == 0:
                print(json.dumps(out[-1]), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return out
    if args.mode == "eval":
        model, env, _ = _build(args, "norm")
        ev = GreedyEvaluator(model, env, max_timesteps=args.max_timesteps, block_size=args.block_size,
                             device_type=torch.device("cuda", torch.cuda.current_device()), sync_every=5, ssim=True,
                             residuals=args.residuals)
        for name, total, load in _sets(args, env=env):
            def load_shard(a, b, load=load):
                batch, tokens = load(a, b)
                mat = _mat(batch)
                return mat, torch.full((b - a,), D.normalised_rtg(args.rtg)), torch.from_numpy(tokens)
            r = run_sharded_greedy(ev, total, load_shard, sync=torch.cuda.synchronize)
            out.append({"set": name, "n": total, "psnr": float(r.reward.mean()),
                        "psnr_increment": float((r.reward - r.initial_reward).mean()),
                        "mean_stop_iteration": float(r.stop_time.float().mean()), "ranks": world,
                        "ssim": float(r.ssim.mean()), "ssim_increment": float((r.ssim - r.initial_ssim).mean())})
            if args.residuals:
                out[-1].update(primal=float(r.residuals[:, 0].mean()), dc=float(r.residuals[:, 5].mean()))
                if args.compress_energy:
                    out[-1]["compress_energy"] = float(np.mean(args.compress_energy))
                    args.compress_energy.clear()
            if rank == 0:
                print(json.dumps(out[-1]), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return out
    if args.mode == "mcts":
        model, env, scorer = _build(args, "norm")
        ev = GreedyEvaluator(model, env, max_timesteps=args.max_timesteps, block_size=args.block_size,
                             device_type=torch.device("cuda", torch.cuda.current_device()), sync_every=4)
        for name, total, load in _sets(args, env=env):
            def load_shard(a, b, load=load):
                batch, tokens = load(a, b)
                mat = _mat(batch)
                return mat, torch.full((b - a,), D.normalised_rtg(args.rtg)), torch.from_numpy(tokens)
            # all images of a rank's shard are searched at once: one tree per image, children and rollouts batched over images;
            # the policy's first token is the UNclipped Re x0 (datasets.py:162; `x0_raw` of the batch)
            tree = MCTS(ev, scorer, rounds=args.rollouts, seed=args.seed)
            psnr, rollouts, secs = run_sharded_mcts(tree, total, load_shard)
            out.append({"set": name, "n": total, "mcts_psnr": float(psnr.mean()),
                        "rollouts_per_s": round(rollouts / secs, 2) if secs > 0 else 0.0, "ranks": world})
            if rank == 0:
                print(json.dumps(out[-1]), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return out
    if True:
        # main.py:187-209: the greedy evaluation once per return-to-go target, PSNR increment averaged over the sets; sharded over
        # the ranks like `eval` (every rank a contiguous shard of each set, one gather per set)
        model, env, _ = _build(args, "flex")
        ev = GreedyEvaluator(model, env, max_timesteps=args.max_timesteps, block_size=args.block_size,
                             device_type=torch.device("cuda", torch.cuda.current_device()), ssim=True, residuals=args.residuals)
        for target in (1.5, 3, 3.5, 4, 4.5):                       # main.py:198
            incs, ssims, ssim_incs, primals, dcs = [], [], [], [], []
            for name, total, load in _sets(args, flex_target=target, env=env):
                def load_shard(a, b, load=load):
                    batch, tokens = load(a, b)
                    mat = _mat(batch)
                    return mat, torch.full((b - a,), D.normalised_rtg(target, flex=True)), torch.from_numpy(tokens)
                r = run_sharded_greedy(ev, total, load_shard, sync=torch.cuda.synchronize)
                incs.append(float((r.reward - r.initial_reward).mean()))
                ssims.append(float(r.ssim.mean()))
                ssim_incs.append(float((r.ssim - r.initial_ssim).mean()))
                if args.residuals:
                    primals.append(float(r.residuals[:, 0].mean()))
                    dcs.append(float(r.residuals[:, 5].mean()))
            out.append({"rtg_target": target, "average_increment": float(np.mean(incs)), "ranks": world,
                        "ssim": float(np.mean(ssims)), "ssim_increment": float(np.mean(ssim_incs))})
            if args.residuals:
                out[-1].update(primal=float(np.mean(primals)), dc=float(np.mean(dcs)))
                if args.compress_energy:
                    out[-1]["compress_energy"] = float(np.mean(args.compress_energy))
                    args.compress_energy.clear()
            if rank == 0:
                print(json.dumps(out[-1]), flush=True)
        if dist is not None:
            dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
