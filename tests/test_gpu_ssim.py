"""SSIM on the MI355X (pnp_ssim): against the reference's own calculate_ssim (G9, tests/golden/g9_ssim.npz) and a float64
restatement over a sweep of shapes, reproducibility, the clamp flag, every handle kind, argument errors, and the layers above
it - GreedyEvaluator(ssim=True), run_pipelined, the CLI's JSON lines."""
import json
import os

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import _lib, data as D, synthetic, weights
from dt4image_restoration_amd.drivers.greedy import GreedyEvaluator
from dt4image_restoration_amd.policy import DecisionTransformer, DecisionTransformerConfig
from test_ssim_host import PAIRS, PARAMS, ssim_ref

pytestmark = pytest.mark.gpu


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def _pair(n, h, w, seed):
    """Smooth image in [0, 1] and a noisy, partly out-of-range version of it."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.nn.functional.avg_pool2d(torch.rand(n, 1, h + 4, w + 4, generator=g), 5, 1).clamp(0, 1)
    x = gt + 0.15 * torch.randn(n, 1, h, w, generator=g)
    return x.contiguous(), gt.contiguous()


def test_g9_reference_ssim(golden_dir):
    """calculate_ssim (the drop-in, numpy in / numpy out, no clamp) against the reference's own outputs."""
    from dt4image_restoration_amd.transformations import calculate_ssim
    z = np.load(os.path.join(golden_dir, "g9_ssim.npz"))
    worst_s = worst_m = 0.0
    for name in PAIRS:
        x, gt = z[f"{name}_x"].astype(np.float32), z[f"{name}_gt"].astype(np.float32)
        for j, (win, L) in enumerate(PARAMS):
            smap, score = calculate_ssim(x, gt, win_size=win, L=L)
            assert isinstance(smap, np.ndarray) and smap.shape == x.shape and np.ndim(score) == 0
            worst_s = max(worst_s, abs(float(score) - float(z[f"{name}_score{j}"])))
            if f"{name}_map{j}" in z.files:
                worst_m = max(worst_m, float(np.abs(smap - z[f"{name}_map{j}"]).max()))
    print(f"G9: max |dscore| = {worst_s:.3e}, max |dmap| = {worst_m:.3e}")
    assert worst_s <= 1e-5 and worst_m <= 2e-3


@pytest.mark.parametrize("n,h,w", [(1, 16, 16), (3, 48, 80), (2, 128, 128), (64, 256, 256), (4, 512, 512), (2, 208, 32)])
def test_shape_sweep_against_float64(n, h, w):
    x, gt = _pair(n, h, w, seed=h * 1000 + w + n)
    e = _engine(n, h, w)
    got, smap = e.ssim(x.cuda(), gt.cuda(), return_map=True)
    torch.cuda.synchronize()
    ref_map, ref = ssim_ref(x.clamp(0, 1).double().numpy()[:, 0], gt.double().numpy()[:, 0], L=1.0)
    d = np.abs(got.cpu().double().numpy() - ref).max()
    dm = np.abs(smap.cpu().double().numpy()[:, 0] - ref_map).max()
    print(f"{n}x{h}x{w}: max |dscore| = {d:.3e}, max |dmap| = {dm:.3e}")
    assert got.shape == (n,) and smap.shape == (n, 1, h, w)
    assert d <= 1e-5 and dm <= 2e-3


def test_identical_images_score_one_and_calls_are_bit_identical():
    x, gt = _pair(5, 128, 96, seed=11)
    x, gt = x.cuda(), gt.cuda()
    e = _engine(5, 128, 96)
    one = e.ssim(gt, gt)
    assert float((one - 1).abs().max()) <= 1e-6
    a, am = e.ssim(x, gt, return_map=True)
    b, bm = e.ssim(x, gt, return_map=True)
    c = e.ssim(x, gt)                                              # no map store: same score
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(am, bm) and torch.equal(a, c)


def test_clamp_flag_matches_clamping_on_the_host():
    x, gt = _pair(3, 64, 64, seed=12)
    assert float(x.min()) < 0 and float(x.max()) > 1
    e = _engine(3, 64, 64)
    on = e.ssim(x.cuda(), gt.cuda(), clamp=True)
    host = e.ssim(x.clamp(0, 1).cuda(), gt.cuda(), clamp=False)
    off = e.ssim(x.cuda(), gt.cuda(), clamp=False)
    assert torch.equal(on, host) and not torch.equal(on, off)


def test_every_handle_kind_and_argument_errors():
    x, gt = _pair(2, 64, 64, seed=13)
    x, gt = x.cuda(), gt.cuda()
    want = _engine(2, 64, 64).ssim(x, gt)                          # PNP_FLAG_NO_DENOISER
    bf16 = _engine(2, 64, 64, denoiser=True, bf16_convs=True)
    bf16.load_weights(weights.generate_unet_weights(0, "unit_gain"))
    f32 = _engine(2, 64, 64, denoiser=True)
    assert torch.equal(bf16.ssim(x, gt), want) and torch.equal(f32.ssim(x, gt), want)
    before = bf16.workspace_bytes
    for kw in ({"radius": 0}, {"radius": 17}, {"data_range": 0.0}, {"data_range": -1.0}):
        with pytest.raises(_lib.PnPError):
            bf16.ssim(x, gt, **kw)
    with pytest.raises(ValueError):
        bf16.ssim(x[:1], gt)
    assert bf16.workspace_bytes == before
    r1 = _engine(2, 64, 64).ssim(x, gt, radius=1)
    r16, m16 = _engine(2, 64, 64).ssim(x, gt, radius=16, return_map=True)    # largest window: LDS above 64 KiB
    torch.cuda.synchronize()
    assert m16.shape == (2, 1, 64, 64)
    # the smallest and the largest radius against the restatement's filter with that many taps
    import test_ssim_host as H
    xs, gs = x.clamp(0, 1).double().cpu().numpy()[:, 0], gt.double().cpu().numpy()[:, 0]
    for r, got in ((1, r1), (16, r16)):
        w = np.exp(-0.5 / 2.25 * np.arange(-r, r + 1) ** 2)
        w /= w.sum()
        mx, my = H.gfilter(xs, w), H.gfilter(gs, w)
        vx, vy, cxy = H.gfilter(xs * xs, w) - mx * mx, H.gfilter(gs * gs, w) - my * my, H.gfilter(xs * gs, w) - mx * my
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        ref = ((2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))).mean(axis=(-2, -1))
        assert np.abs(got.cpu().double().numpy() - ref).max() <= 1e-5, r


def test_calculate_ssim_tensor_and_batched_inputs():
    from dt4image_restoration_amd.transformations import calculate_ssim
    x, gt = _pair(3, 32, 48, seed=14)
    smap, score = calculate_ssim(x[:, 0].cuda(), gt[:, 0].cuda(), L=1)
    assert smap.is_cuda and smap.shape == (3, 32, 48) and score.shape == (3,)
    ref = ssim_ref(x.double().numpy()[:, 0], gt.double().numpy()[:, 0], L=1.0)[1]     # no clamp in calculate_ssim
    assert np.abs(score.cpu().double().numpy() - ref).max() <= 1e-5
    with pytest.raises(ValueError):
        calculate_ssim(np.zeros((24, 32), np.float32), np.zeros((24, 32), np.float32))


def _evaluator(steps, ssim):
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    m = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    m.load_state_dict(weights.generate_policy_weights(m, 7, t_bias=-1.0, head_gain=8.0))
    env = PnPEnv(steps, UNetDenoiser2D.seeded(0, "unit_gain"), "cuda")
    return GreedyEvaluator(m, env, max_timesteps=steps, device_type="cuda", sync_every=4, ssim=ssim), env


def test_greedy_evaluator_scores_ssim():
    n, steps = 5, 8
    p = synthetic.make_problem(n, 128, 128, accel=4.0, sigma_n=10.0 / 255.0, seed=505)
    mat = {k: torch.from_numpy(np.asarray(v)) for k, v in p.items()}
    rtg, task = torch.full((n,), D.normalised_rtg(10.0)), torch.full((n,), 4)
    ev, env = _evaluator(steps, True)
    r = ev.run(mat, rtg, task)
    gt = torch.from_numpy(p["gt"]).cuda()
    assert r.ssim.shape == (n, 1) and r.initial_ssim.shape == (n, 1) and not r.ssim.is_cuda
    assert torch.equal(r.ssim, env.compute_ssim(r.x, gt))
    assert bool(((r.ssim > 0) & (r.ssim <= 1)).all()) and bool(((r.initial_ssim > 0) & (r.initial_ssim <= 1)).all())
    want_init = ssim_ref(np.clip(p["x0"][..., 0].reshape(n, 128, 128), 0, 1), p["gt"].reshape(n, 128, 128), L=1.0)[1]
    assert np.abs(r.initial_ssim.numpy()[:, 0] - want_init).max() <= 1e-5
    piped = ev.run_pipelined(mat, rtg, task, parts=2)
    torch.cuda.synchronize()
    assert piped.stop_time.tolist() == r.stop_time.tolist()
    # FLOAT TOLERANCE: f32 summation order of another tile plan (sub-batches of 2 and 3), carried through the policy-driven steps
    assert float((piped.ssim - r.ssim).abs().max()) < 1e-4
    assert float((piped.initial_ssim - r.initial_ssim).abs().max()) < 1e-6
    off, _ = _evaluator(steps, False)
    r0 = off.run(mat, rtg, task)
    assert r0.ssim is None and r0.initial_ssim is None
    assert torch.equal(r0.reward, r.reward) and torch.equal(r0.stop_time, r.stop_time)


def test_cli_eval_prints_ssim(capsys):
    from dt4image_restoration_amd import cli
    ev = cli.main(["--block_size", "18", "--n_embeds", "9", "--limit", "2", "eval", "--rtg", "10", "--max_timesteps", "4"])
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().split("\n") if s.startswith("{")]
    assert len(ev) == 2 and len(lines) == 2
    for e in lines:
        assert {"psnr", "psnr_increment", "mean_stop_iteration", "ssim", "ssim_increment"} <= set(e)
        assert 0.0 < e["ssim"] <= 1.0 and -1.0 < e["ssim_increment"] < 1.0
