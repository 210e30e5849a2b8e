#!/usr/bin/env python3
"""Headline benchmark: PnP-ADMM iterations/s on 256x256 CS-MRI, 64 slices per GPU (BASELINE.json
configs[1]); one rank per GPU, slices sharded with no data-path collective (weak scaling).

    python bench.py --gpus 1 --steps 30 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one `pnp_step` over the 64 slices resident on a GPU: U-Net denoiser forward, centred
2-D FFT data-fidelity solve, dual update (the body of the reference's PnPEnv.step, env.py:74-100).
Inputs are synthetic and already resident in HBM when the timed region starts.  Rank 0 prints ONE
JSON line; see DESIGN.md "Measurement" for how `roofline` and `cpu_baseline` are obtained.

A plain run does only what the headline needs: set-up, ONE episode of W warm-up + exactly K timed
steps, the result line.  `--full` adds the rest of the record: 10 repetitions (median reported), the
DT-driven leg, the configs[4] leg, the CPU baseline and the PSNR check against the CPU oracle.
`--dump-outputs DIR` writes what the timed path returned after its last step as DIR/<name>.npy
(float32; arrays above DUMP_CAP scalars as a fixed seeded sample), so two builds can be compared.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from dt4image_restoration_amd import synthetic, unet_spec, weights  # noqa: E402
from dt4image_restoration_amd.engine import PnPEngine  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~8 TB/s
BF16_MFMA_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA
F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense, spec


def mfma_conv_flops(n, h, w):
    """Algorithmic FLOPs of the 26 conv3x3 layers that run on the MFMA kernel (all but the 2->32 first
    layer and the 1x1 last layer), per step."""
    return n * sum(2 * l.macs_per_out_pixel * (h >> l.level) * (w >> l.level)
                   for l in unet_spec.UNET_LAYERS[1:27])


TRAFFIC_ROUNDS = ("r05", "r04", "r03", "r02", "r01")     # newest first

DUMP_CAP = 1 << 22         # scalars per dumped array (16 MB of float32): x, z, u stay under 64 MB together
DUMP_SEED = 20240607


def dump_outputs(path, arrays):
    """Write each tensor as <path>/<name>.npy in float32 (complex as a trailing (re, im) axis).  An array of more than
    DUMP_CAP scalars is written as [k, 2] (complex) or [k] elements at a fixed seeded sample of k of its flat element
    indices (sorted): the same elements in every run of the same shape."""
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach().cpu()
        a = (torch.view_as_real(t) if t.is_complex() else t).numpy().astype(np.float32)
        if a.size > DUMP_CAP:
            per = a.size // t.numel()
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(t.numel(), DUMP_CAP // per, replace=False))
            a = a.reshape(t.numel(), per)[idx]
            if per == 1:
                a = a[:, 0]
        np.save(os.path.join(path, f"{name}.npy"), a)


def pmc_traffic(n, h, w, which, mode="f32"):
    """PMC-measured HBM bytes per step (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, separate rocprofv3 passes of this
    same command, folded by tools/refresh_profiles.py into profiles/rNN_traffic[_<n>x<h>x<w>_<mode>].json; the unsuffixed file is
    configs[1] = 64x256x256 f32).  The file is picked by (n, h, w, mode): a size or mode nobody profiled prints null, never
    another configuration's bytes.  which: "conv" (the 26 conv3x3 launches) or "fft" (the three data-fidelity launches).
    Returns (bytes, file) or (None, None)."""
    names = [f"{r}_traffic_{n}x{h}x{w}_{mode}.json" for r in TRAFFIC_ROUNDS]
    if (n, h, w, mode) == (64, 256, 256, "f32"):
        names += [f"{r}_traffic.json" for r in TRAFFIC_ROUNDS]
    for name in names:
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        with open(path) as f:
            t = json.load(f)
        kf, kw = f"{which}_kernels_fetch_bytes_per_step", f"{which}_kernels_write_bytes_per_step"
        if kf in t and kw in t:
            return int(t[kf] + t[kw]), "profiles/" + name
    return None, None


def g8_reference(h, w, accel, total_iters, mu_tab, sig_tab):
    """tests/golden/g8_config4.npz - the REFERENCE's own f32 trajectory of configs[4] (2 slices of 512x512, 8x mask, 53
    iterations of this bench's parameter table) - when this invocation steps exactly that problem; else None."""
    path = os.path.join(ROOT, "tests", "golden", "g8_config4.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    if (h, w) != (512, 512) or float(accel) != float(g["accel"]) or total_iters != g["psnr"].shape[1] or mu_tab.shape[0] < 2:
        return None
    if not (np.array_equal(mu_tab[:2], g["mu_tab"]) and np.array_equal(sig_tab[:2], g["sig_tab"])):
        return None
    return g["psnr"]


def host_cores():
    """Cores this process may actually use: affinity mask and cgroup quota, not the machine's core count
    (a 1-GPU box exposes 256 logical CPUs but grants a 16-core share)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    cap = int(os.environ.get("PNP_CPU_THREADS", "16"))
    return max(1, min(n, cap))


def cpu_baseline(sd_np, h, w, batch, slices, iters, mu_tab, sig_tab, accel=4.0, long_ref_iters=0):
    """Time the CPU oracle (oracle/pnp_oracle.py, torch CPU fp32) on `slices` slices x `iters`
    iterations of the same workload; scaled linearly to batch-iterations/s.  long_ref_iters > 0 (bf16 mode on a problem
    the committed reference fixture does not cover): also the f32 oracle's per-iteration PSNR of slices 0-1 over that
    many iterations (untimed; the checker of `psnr_delta_vs_oracle_db`)."""
    from oracle import pnp_oracle as O
    threads = host_cores()
    torch.set_num_threads(threads)
    data = synthetic.make_problem(slices, h, w, accel=accel, sigma_n=10.0 / 255.0, seed=1234)
    sd = O.torch_weights(sd_np)
    with torch.no_grad():
        O.run_episode(sd, data, mu_tab[:slices], sig_tab[:slices], 1, record_psnr=False)      # warm-up
        t0 = time.perf_counter()
        st, hist = O.run_episode(sd, data, mu_tab[:slices], sig_tab[:slices], iters)
        dt = time.perf_counter() - t0
    slice_iters_per_s = slices * iters / dt
    long_ref = None
    if long_ref_iters > 0:
        k = min(2, slices)                                         # (data holds `slices` slices)
        few = {key: (v[:k] if key != "mask" else v) for key, v in data.items()}
        with torch.no_grad():
            long_ref = O.run_episode(sd, few, mu_tab[:k], sig_tab[:k], long_ref_iters)[1].numpy()
    return {"value": slice_iters_per_s / batch, "unit": "batch-iterations/s", "cores": threads, "kind": "port",
            "sample": f"{slices} slices x {iters} iterations of the {h}x{w} workload in {dt:.1f} s "
                      f"({slice_iters_per_s:.2f} slice-iterations/s), scaled linearly to batch {batch}",
            "slice_iters_per_s": slice_iters_per_s}, data, hist, long_ref


def greedy_leg(args, dev, sd_np, n, h, w, world):
    """End-to-end DT-driven episode (BASELINE configs[2], drivers/sharded.run_sharded_greedy): every rank rolls its shard
    of n slices out for `--steps` iterations with the decision-transformer policy choosing (T, sigma_d, mu) per slice and
    step, then the per-slice PSNR / stop iteration are gathered (the path's only collective).  Seeded policy whose stop logit
    is far below threshold, so every slice runs all steps.  Inputs are moved to the GPU before the timed region."""
    from dt4image_restoration_amd import data as D
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.drivers.greedy import GreedyEvaluator
    from dt4image_restoration_amd.drivers.sharded import run_sharded_greedy
    from dt4image_restoration_amd.env import PnPEnv
    from dt4image_restoration_amd.policy import DecisionTransformer, DecisionTransformerConfig
    model = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    model.load_state_dict(weights.generate_policy_weights(model, 7, t_bias=-8.0, head_gain=1.0))
    den = UNetDenoiser2D(state_dict=sd_np, bf16_convs=args.convs == "bf16")
    # the policy's time embedding has 30 entries (decision_transformer.py:283 max_timestep): a DT-driven episode is at most 30 steps
    ep_steps = min(args.steps, model.time_embed.num_embeddings)
    ev = GreedyEvaluator(model, PnPEnv(ep_steps, den, dev), max_timesteps=ep_steps, device_type=dev, sync_every=10)
    total = n * world
    shard = {}

    def load_shard(a, b):
        if (a, b) not in shard:
            p = synthetic.make_problem(b - a, h, w, accel=args.accel, sigma_n=10.0 / 255.0, seed=1234, first_slice=a)
            shard[(a, b)] = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in p.items()}
        return shard[(a, b)], torch.full((b - a,), D.normalised_rtg(10.0)), torch.full((b - a,), 4)

    run_sharded_greedy(ev, total, load_shard, sync=torch.cuda.synchronize, pipeline=args.pipeline)      # warm-up episode
    secs, res = [], None
    for _ in range(max(1, min(args.reps, 5))):
        res = run_sharded_greedy(ev, total, load_shard, sync=torch.cuda.synchronize, pipeline=args.pipeline)
        secs.append(res.seconds)
    secs.sort()
    med = secs[(len(secs) - 1) // 2]
    return {"what": "DT-driven rollout end to end: per step one policy call (steady state: ONE decision-transformer forward with both "
                    "heads over the 6-step context - the reference's two forwards read identical tokens from step 6 on -, state embeddings "
                    "cached, both captured in hipGraphs; the first 6 steps two eager forwards) + one pnp_step, all slices of a rank as one batch; reset, first policy call "
                    "and the final PSNR gather included",
            "pipeline": (f"{args.pipeline} sub-batches per rank on their own streams, one's policy call under another's env step"
                         if args.pipeline > 1 else "off (one batch per rank: policy and env step alternate on one stream)"),
            "steps": res.steps, "slices": total, "seconds_median": round(med, 5), "ms_per_step": round(1e3 * med / max(res.steps, 1), 4),
            "batch_iterations_per_sec": round(world * res.steps / med, 3), "episodes_timed": len(secs),
            "psnr_mean_db": round(float(res.reward.mean()), 4), "stop_iteration_mean": float(res.stop_time.float().mean())}, res


def config4_leg(args, dev, sd_np, local_rank):
    """BASELINE configs[4] beside the headline (the same hot loop, /root/reference/evaluation/env.py:74-100, on the config the
    baseline labels "HBM-bound FFT stress"): 16 slices of 512x512 per GPU, 8x radial mask, bf16-operand denoiser convs (weights as
    two bf16 terms), 50 timed + 3 warm-up iterations of the seeded parameter table - the problem tests/golden/g8_config4.npz holds
    the REFERENCE's own f32 trajectory of, for slices 0-1.  Timed like the headline (reset, W untimed steps, K steps between
    synchronize brackets; median of 3), kernel time from the engine's HIP events on the launch stream; then one more episode with the
    PSNR of every iteration, compared with the fixture."""
    n, h, w, accel, steps, warm = 16, 512, 512, 8.0, 50, 3
    total = steps + warm
    data = synthetic.make_problem(n, h, w, accel=accel, sigma_n=10.0 / 255.0, seed=1234)
    mu_tab, sig_tab = synthetic.param_table(n, total, seed=77)
    eng = PnPEngine(n, h, w, device=local_rank, profile=True, bf16_convs=True)
    eng.load_weights(sd_np)
    x0 = torch.view_as_complex(torch.from_numpy(data["x0"])).to(dev)
    y0 = torch.view_as_complex(torch.from_numpy(data["y0"])).to(dev)
    mask = torch.from_numpy(data["mask"]).to(dev)
    gt = torch.from_numpy(data["gt"]).to(dev)
    mu_d = torch.from_numpy(mu_tab).to(dev).t().contiguous()
    sg_d = torch.from_numpy(sig_tab).to(dev).t().contiguous()
    times, profs = [], []
    for _ in range(3):
        x, z, u = eng.reset(x0, y0, mask)
        for t in range(warm):
            eng.step(x, z, u, mu_d[t], sg_d[t])
        torch.cuda.synchronize()
        eng.profile_reset()
        t0 = time.perf_counter()
        for t in range(warm, total):
            eng.step(x, z, u, mu_d[t], sg_d[t])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        profs.append(eng.profile_collect())
    med = sorted(range(3), key=lambda i: times[i])[1]
    conv_ms = sum(p["conv3x3_mfma"]["ms"] for p in profs) / 3 / steps
    fft_ms = sum(p["fft_rows"]["ms"] + p["fft_cols_prox"]["ms"] for p in profs) / 3 / steps
    terms = eng.bf16_weight_terms()
    flops = mfma_conv_flops(n, h, w)
    x, z, u = eng.reset(x0, y0, mask)
    hist = []
    for t in range(total):
        eng.step(x, z, u, mu_d[t], sg_d[t])
        hist.append(eng.psnr(x, gt)[:2])
    hist = torch.stack(hist, dim=1).cpu().numpy()
    g8 = g8_reference(h, w, accel, total, mu_tab, sig_tab)
    out = {"what": "BASELINE configs[4] on one GPU: 16 slices of 512x512, 8x radial mask, bf16 conv operands (weights as "
                   f"{terms} bf16 terms), {steps} timed + {warm} warm-up iterations; median of 3 repetitions",
           "value": round(steps / times[med], 3), "unit": "batch-iterations/s", "ms_per_step": round(1e3 * times[med] / steps, 4),
           "slice_iterations_per_sec": round(n * steps / times[med], 1),
           "conv_kernels_ms_per_step": round(conv_ms, 4), "fft_kernels_ms_per_step": round(fft_ms, 4),
           "conv_frac_of_bf16_mfma_peak_issued": round(terms * flops / (conv_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
           "conv_frac_of_bf16_mfma_peak_algorithmic": round(flops / (conv_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
           "fft_frac_of_hbm_peak_algorithmic": round(37.0 * n * h * w / (fft_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "psnr_mean_db": round(float(eng.psnr(x, gt).mean()), 4)}
    if g8 is not None:
        d = np.abs(hist - g8)
        out["psnr_delta_vs_oracle_db"] = float(d[:, -1].max())
        out["psnr_delta_max_over_iterations_db"] = float(d.max())
        out["psnr_delta_what"] = (f"slices 0-1 of the timed 16-slice handle against the reference's own f32 trajectory (tests/golden/g8_config4.npz) at "
                                  f"iteration {total} and the maximum over all {total} iterations; north_star's bound is 0.01 dB")
    else:
        out["psnr_delta_vs_oracle_db"] = None
        out["psnr_delta_what"] = "tests/golden/g8_config4.npz does not hold this problem"
    del eng
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="the whole record, not just the headline: 10 repetitions unless --reps says otherwise, the DT-driven leg, "
                         "the configs[4] leg, the CPU baseline and the PSNR check against the CPU oracle (each --no-* switch drops one)")
    ap.add_argument("--reps", type=int, default=None,
                    help="repetitions of the [reset, W warm-up steps, K timed steps] episode; the line reports the MEDIAN "
                         "repetition (each one is exactly K steps between barrier + synchronize brackets, max over ranks); "
                         "default 1, with --full 10")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path returned after its last step as DIR/<name>.npy (float32)")
    ap.add_argument("--batch", type=int, default=64, help="slices per GPU")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--convs", choices=("f32", "bf16"), default="f32",
                    help="bf16: BASELINE configs[4]'s bf16-operand denoiser convs (PNP_FLAG_BF16_CONVS); not the headline line")
    ap.add_argument("--accel", type=float, default=4.0, help="undersampling factor of the radial mask (configs[4]: 8)")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="experiment: no per-kernel HIP events in the timed region (roofline fields become null)")
    ap.add_argument("--mode", choices=("engine", "greedy"), default="engine",
                    help="engine (headline): K pnp_step calls driven by a parameter table; greedy: BASELINE configs[2]'s DT-driven "
                         "sharded episode end to end is the timed thing (value = its batch-iterations/s)")
    ap.add_argument("--no-greedy", action="store_true", help="skip the end-to-end DT-driven leg of the --full line")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="DT-driven leg: sub-batches per rank that advance on their own streams (GreedyEvaluator.run_pipelined; "
                         "1 = off, the default: two sub-batches of 32 measured 9.64 against 9.39 ms per step - the policy's chain "
                         "of ~110 small kernels stretches under the other sub-batch's convs and two 32-slice steps cost more than "
                         "one 64-slice step)")
    ap.add_argument("--no-config4", action="store_true", help="skip the BASELINE configs[4] leg of the --full line (N = 1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU baseline and oracle check of the --full line")
    ap.add_argument("--cpu-slices", type=int, default=16)
    ap.add_argument("--cpu-iters", type=int, default=6)
    ap.add_argument("--dump-layers", default=None, help="write the per-layer kernel time table (JSON) here")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 10 if args.full else 1

    # stdout carries exactly ONE line, the JSON result: libraries that print banners to fd 1 (RCCL prints its version block
    # when the first communicator is created) are sent to stderr for the duration of the run
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run --nproc-per-node N")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or "RANK" in os.environ:      # under torch.distributed.run the RCCL path runs even with one rank
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)

    n, h, w = args.batch, args.size, args.size
    total_iters = args.steps + args.warmup
    sd_np = weights.generate_unet_weights(0, "unit_gain")
    # this rank's shard of the job: slices [rank*n, rank*n + n)
    data = synthetic.make_problem(n, h, w, accel=args.accel, sigma_n=10.0 / 255.0, seed=1234, first_slice=rank * n)
    mu_tab, sig_tab = synthetic.param_table(n, total_iters, seed=77 + rank)

    bf16 = args.convs == "bf16"
    eng = PnPEngine(n, h, w, device=local_rank, profile=not args.no_kernel_events, bf16_convs=bf16,
                    profile_layers=args.dump_layers is not None)      # the per-layer table costs an event pair per launch
    eng.load_weights(sd_np)
    x0 = torch.view_as_complex(torch.from_numpy(data["x0"])).to(dev)
    y0 = torch.view_as_complex(torch.from_numpy(data["y0"])).to(dev)
    mask = torch.from_numpy(data["mask"]).to(dev)
    gt = torch.from_numpy(data["gt"]).to(dev)
    mu_d = torch.from_numpy(mu_tab).to(dev).t().contiguous()       # [iters, n]
    sg_d = torch.from_numpy(sig_tab).to(dev).t().contiguous()
    def barrier():
        if dist is not None:
            dist.barrier()

    def episode():
        """reset (untimed), W warm-up steps (untimed), then EXACTLY K steps between barrier + synchronize brackets."""
        x, z, u = eng.reset(x0, y0, mask)
        p0 = eng.psnr(x, gt)
        for t in range(args.warmup):
            eng.step(x, z, u, mu_d[t], sg_d[t])
        torch.cuda.synchronize()
        eng.profile_reset()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.warmup, total_iters):
            eng.step(x, z, u, mu_d[t], sg_d[t])
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        pr = eng.profile_collect()
        el = torch.tensor([dt], dtype=torch.float64, device=dev)
        if dist is not None:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        return float(el.item()), pr, p0, eng.psnr(x, gt), (x, z, u)

    reps = max(1, args.reps)
    times, profs = [], []
    for _ in range(reps):
        dt, pr, psnr0, psnr1, xzu = episode()
        times.append(dt)
        profs.append(pr)
    order = sorted(range(reps), key=lambda i: times[i])
    med = order[(reps - 1) // 2]                 # the median repetition (lower median for an even count)
    elapsed = times[med]
    # kernel-time fields: averaged over ALL repetitions (every repetition brackets the same launches with the same events)
    prof = {k: ({"ms": sum(p[k]["ms"] for p in profs) / reps, "launches": profs[0][k]["launches"]} if k != "layers"
                else {"ms": [sum(p["layers"]["ms"][i] for p in profs) / reps for i in range(len(profs[0]["layers"]["ms"]))],
                      "launches": profs[0]["layers"]["launches"]}) for k in profs[0]}

    if dist is not None:
        # the path's only collective: gather the per-slice PSNR of every shard
        allp = [torch.empty_like(psnr1) for _ in range(world)]
        dist.all_gather(allp, psnr1)
        psnr_all = torch.cat(allp)
    else:
        psnr_all = psnr1
    if args.dump_outputs and rank == 0:
        # the iterate pnp_step updates in place, after the last timed step of the last repetition (rank 0's shard)
        dump_outputs(args.dump_outputs, dict(zip("xzu", xzu)))

    greedy = None
    if (args.full and not args.no_greedy) or args.mode == "greedy":
        greedy, gres = greedy_leg(args, dev, sd_np, n, h, w, world)     # collective inside: every rank takes part
        if args.dump_outputs and rank == 0 and args.mode == "greedy":
            dump_outputs(args.dump_outputs, {"greedy_psnr": gres.reward, "greedy_stop_iteration": gres.stop_time.float()})

    if rank == 0:
        steps = args.steps
        value = world * steps / elapsed                           # batch-iterations/s over the whole job
        conv_ms = prof["conv3x3_mfma"]["ms"]
        conv_launches = prof["conv3x3_mfma"]["launches"]
        flops_step = mfma_conv_flops(n, h, w)
        algorithmic = flops_step * steps / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else None
        algos = eng.conv_algorithms()
        mfma_peak = BF16_MFMA_PEAK_TFLOPS if bf16 else F32_MFMA_PEAK_TFLOPS
        # MFMA flops actually ISSUED: a Winograd F(2x2,3x3) layer multiplies 16 instead of 36 times per 2x2 outputs, an
        # F(4x4,3x3) layer 36 instead of 144 per 4x4 outputs
        ratio = {0: 1.0, 1: 16.0 / 36.0, 4: 36.0 / 144.0}
        # bf16 mode: a weight rides as `terms` bf16 terms (2 = hi + lo, the default), one MFMA each per k-step
        terms = eng.bf16_weight_terms() if bf16 else 1
        exec_step = n * terms * sum(2 * l.macs_per_out_pixel * (h >> l.level) * (w >> l.level) * ratio.get(algos[l.index], 1.0)
                                    for l in unet_spec.UNET_LAYERS[1:27])
        executed = exec_step * steps / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else None
        mode = "bf16" if bf16 else "f32"
        conv_traffic, conv_traffic_src = pmc_traffic(n, h, w, "conv", mode)
        ms_all = sorted(1e3 * t / steps for t in times)
        out = {
            "metric": "pnp_admm_iterations_per_sec", "value": round(value, 4), "unit": "batch-iterations/s",
            "n_gpus": world, "world_size_reported_by_rccl": (dist.get_world_size() if dist is not None else None), "steps": steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": (f"bf16 conv operands (weights as {terms} bf16 term{'s hi + lo' if terms == 2 else ''}), f32 accumulate / bias / "
                      "pooling / upsampling / k-space") if bf16 else "f32", "data": "synthetic",
            "config": {"workload": f"{'configs[4] geometry' if bf16 else 'configs[1]'}: {h}x{w} CS-MRI slices, batch {n} per GPU, "
                                   f"U-Net denoiser{' (bf16 conv operands)' if bf16 else ''} + FFT prox, "
                                   f"seeded per-slice (mu, sigma) table, {args.accel:g}x radial mask", "slices_per_gpu": n,
                       "global_slices": n * world, "h": h, "w": w, "sharding": f"slices over {world} rank(s), no data-path collective"},
            "repetitions": {"n": reps, "what": "each = reset + W untimed warm-up steps + K timed steps (barrier + synchronize on both "
                                               "sides, max over ranks); value / ms_per_step are the MEDIAN repetition",
                            "ms_per_step_median": round(ms_all[(reps - 1) // 2], 4), "ms_per_step_min": round(ms_all[0], 4),
                            "ms_per_step_max": round(ms_all[-1], 4), "ms_per_step_all": [round(1e3 * t / steps, 4) for t in times]},
            "slice_iterations_per_sec": round(value * n, 2),
            "psnr_mean_db": round(float(psnr_all.mean()), 4),
            "roofline": {
                "kernel": "conv3x3_wino4_kernel + conv3x3_wino4p_kernel + conv3x3_winograd_kernel + conv3x3_mfma_kernel + conv3x3_bf16ws_kernel "
                          f"(26 launches/step: all denoiser conv3x3 layers with Cin>=32; {sum(1 for v in algos if v == 4)} on Winograd F(4x4,3x3), "
                          f"{sum(1 for v in algos if v == 1)} on Winograd F(2x2,3x3), {sum(1 for v in algos[1:27] if v == 0)} direct, "
                          f"{sum(1 for v in algos if v == 5)} bf16 producer/consumer)",
                "bound": "mfma", "achieved": round(executed, 3) if executed else None, "peak": mfma_peak,
                "unit": "TFLOP/s", "frac": round(executed / mfma_peak, 4) if executed else None,
                "traffic": conv_traffic, "traffic_source": conv_traffic_src,
                "traffic_note": "HBM bytes per step of the same kernels from rocprofv3 PMC passes of this command (FETCH_SIZE x2 gfx950 "
                                "correction + WRITE_SIZE, separate passes), not measured in this run",
                "timing": "one HIP event pair on the launch stream around the run of consecutive conv3x3 launches of each step "
                          "(26 launches, nothing else in between), averaged over the timed steps of all repetitions; --dump-layers "
                          "switches to a pair per launch (costs ~0.2 ms per step)",
                "note": "achieved / frac = MFMA FLOPs actually ISSUED by these kernels / kernel time (a true pipe fraction, <= 1).  "
                        "algorithmic_tflops = the direct-convolution FLOPs of the same layers (SURVEY 8d) / the same time: Winograd "
                        "layers issue winograd_multiply_ratio of those multiplies, so it may exceed the f32 MFMA peak.",
                "algorithmic_tflops": round(algorithmic, 3) if algorithmic else None,
                "algorithmic_frac_of_direct_peak": round(algorithmic / mfma_peak, 4) if algorithmic else None,
                "winograd_multiply_ratio": round(exec_step / flops_step, 4),
                "flops_per_step": flops_step, "mfma_flops_issued_per_step": int(exec_step),
                "kernel_ms_per_step": round(conv_ms / steps, 4),
                "launches_per_step": conv_launches / steps,
                "other_kernels_ms_per_step": {k: round(v["ms"] / steps, 4) for k, v in prof.items()
                                              if k not in ("layers", "conv3x3_mfma")},
            },
        }
        # data-fidelity stage (fft_rows fwd + fft_cols_prox + fft_rows inv): HBM-bound; SURVEY 8(d): 37 B/px/iteration
        fft_ms = (prof["fft_rows"]["ms"] + prof["fft_cols_prox"]["ms"]) / steps
        if fft_ms > 0:
            alg = 37.0 * n * h * w
            moved = 81.0 * n * h * w          # + the two round trips of the complex scratch between the three passes
            out["roofline_fft"] = {
                "kernel": "fft_rows_kernel<1> + fft_cols_kernel<1> + fft_rows_kernel<2> (3 launches/step)", "bound": "hbm",
                "achieved": round(alg / (fft_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(alg / (fft_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(n, h, w, "fft", mode)[0],
                "traffic_source": pmc_traffic(n, h, w, "fft", mode)[1],
                "bytes_per_step": int(alg), "kernel_ms_per_step": round(fft_ms, 4),
                "moved_gbs": round(moved / (fft_ms * 1e-3) / 1e9, 1),
                "note": "achieved = algorithmic 37 B/px (x 4 + u 8 + y0 8 + mask 1 read, z 8 + u 8 written) / kernel time; the "
                        "three LDS-resident passes actually move 81 B/px (two round trips of the complex scratch, which a "
                        "256x256 slice = 512 KiB > LDS cannot avoid) = moved_gbs",
            }
        if args.full and world == 1 and not args.no_config4 and not bf16 and (n, h, w) == (64, 256, 256):
            out["config4"] = config4_leg(args, dev, sd_np, local_rank)
        if greedy is not None:
            out["greedy"] = greedy
            out["greedy_ms_per_step"] = greedy["ms_per_step"]
            if args.mode == "greedy":                             # the DT-driven episode is the headline of this invocation
                out["engine_only"] = {"value": out["value"], "ms_per_step": out["ms_per_step"]}
                out["value"] = greedy["batch_iterations_per_sec"]
                out["ms_per_step"] = greedy["ms_per_step"]
                out["config"]["workload"] = out["config"]["workload"].replace("configs[1]", "configs[2] (DT-driven, sharded)")
        if args.dump_layers:
            rows = []
            for l, ms, cnt in zip(unet_spec.UNET_LAYERS, prof["layers"]["ms"], prof["layers"]["launches"]):
                fl = 2 * l.macs_per_out_pixel * (h >> l.level) * (w >> l.level) * n
                per = ms / max(cnt, 1)
                rows.append({"layer": l.key, "cin": l.cin, "cout": l.cout, "hw": [h >> l.level, w >> l.level],
                             "gflop": round(fl / 1e9, 2), "ms": round(per, 4),
                             "tflops": round(fl / (per * 1e-3) / 1e12, 2) if per > 0 else None})
            with open(args.dump_layers, "w") as f:
                json.dump(rows, f, indent=1)
        if args.full and world == 1 and not args.no_cpu_baseline:
            args.cpu_slices = min(args.cpu_slices, n)              # the sample is a prefix of the batch
            mu_c, sg_c = synthetic.param_table(n, total_iters, seed=77)
            g8 = g8_reference(h, w, args.accel, total_iters, mu_tab, sig_tab) if bf16 else None
            cb, cdata, chist, long_ref = cpu_baseline(sd_np, h, w, n, args.cpu_slices, args.cpu_iters, mu_c, sg_c, args.accel,
                                                      long_ref_iters=total_iters if (bf16 and g8 is None) else 0)
            # PSNR delta vs the oracle ON THE TIMED HANDLE (same tile plan, same launches as the timed region): reset it, run the
            # oracle's parameter prefix over all n slices, compare the sampled slices (the oracle's data are a prefix of this batch)
            assert np.array_equal(cdata["gt"], data["gt"][:args.cpu_slices]) and np.array_equal(mu_c, mu_tab)
            x2, z2, u2 = eng.reset(x0, y0, mask)
            gpu_hist = []
            for t in range(total_iters if bf16 else args.cpu_iters):
                eng.step(x2, z2, u2, mu_d[t], sg_d[t])
                gpu_hist.append(eng.psnr(x2, gt))
            gpu_hist = torch.stack(gpu_hist, dim=1).cpu()          # [n, iterations]
            cb.pop("slice_iters_per_s")
            out["cpu_baseline"] = cb
            if not bf16:
                dpsnr = (gpu_hist[:args.cpu_slices, args.cpu_iters - 1] - chist[:, -1]).abs().max()
                out["psnr_delta_vs_oracle_db"] = float(dpsnr)      # the oracle here is always the f32 reference arithmetic
                out["psnr_delta_what"] = (f"max over the first {args.cpu_slices} slices after {args.cpu_iters} iterations, computed on the TIMED "
                                          f"{n}-slice handle (same plan and kernels as the timed region) against the f32 CPU oracle")
            else:
                # bf16 mode: the offset to the f32 reference GROWS with the iteration count, so it is evaluated at the LAST timed
                # iteration (warm-up + steps), against the reference's own trajectory where this invocation steps the committed
                # fixture's problem (tests/golden/g8_config4.npz), else against the f32 CPU oracle run that long on two slices
                ref, src = g8, "the reference's own f32 trajectory, tests/golden/g8_config4.npz"
                if ref is None:
                    ref, src = long_ref, "the f32 CPU oracle stepped over the same iterations"
                if ref is None:
                    out["psnr_delta_vs_oracle_db"] = None
                    out["psnr_delta_what"] = "no reference trajectory for this invocation"
                    ref = np.zeros((0, total_iters), dtype=np.float32)
                d = np.abs(gpu_hist[:ref.shape[0]].numpy() - ref)
                if ref.shape[0]:
                    out["psnr_delta_vs_oracle_db"] = float(d[:, -1].max())
                    out["psnr_delta_max_over_iterations_db"] = float(d.max())
                    marks = sorted({0, 5, 9, 19, 29, 39, total_iters - 4, total_iters - 1} & set(range(total_iters)))
                    out["psnr_delta_by_iteration_db"] = {str(m + 1): round(float(d[:, m].max()), 5) for m in marks}
                    out["psnr_delta_what"] = (f"max over slices 0-{ref.shape[0] - 1} at the LAST iteration ({total_iters} = warm-up + timed steps) and per "
                                          f"iteration count, computed on the TIMED {n}-slice handle against {src}; north_star's bound is 0.01 dB")
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
