"""The k-space stage at sides of 2^a * 5^b (80, 160, 320, 400, 640, 800; fft_mixed_kernels.hip) on the GPU: the centred transforms and
the fused data-fidelity stage against the CPU oracle, ADMM trajectories against the reference's own runs at 320 x 320 and 640 x 320
(g10_radix5.npz), determinism, the bf16 handle, the drivers, and the sizes that stay refused."""
import os

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import synthetic
from oracle import pnp_oracle as O

pytestmark = pytest.mark.gpu

PSNR_TOL_DB = 0.01     # north_star: restored images within +-0.01 dB PSNR of the reference CPU path


@pytest.fixture(scope="module")
def denoiser():
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    return UNetDenoiser2D.seeded(0, "unit_gain")


def _env(denoiser):
    from dt4image_restoration_amd.env import PnPEnv
    return PnPEnv(max_episode_step=30, denoiser=denoiser, device_type="cuda")


def _mat(data):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in data.items()}


def _kspace_engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, denoiser=False, **kw)


def _rand_complex(seed, b, h, w):
    v = synthetic.hash_uniform(seed, h * 1000 + w, 2 * b * h * w).reshape(b, 1, h, w, 2)
    return torch.view_as_complex(torch.from_numpy(v.copy()))


@pytest.mark.parametrize("h,w,b", [(80, 80, 2), (320, 320, 1), (640, 320, 2), (320, 640, 1), (160, 64, 3), (400, 400, 2),
                                   (800, 160, 1)])
def test_fft2c_matches_oracle_round_trips_and_keeps_energy(h, w, b):
    e = _kspace_engine(b, h, w)
    c = _rand_complex(3, b, h, w)
    cg = c.cuda()
    for inverse, ref in ((False, O.fft2c(c)), (True, O.ifft2c(c))):
        got = e.fft2c(cg, inverse=inverse).cpu()
        # FLOAT TOLERANCE: f32 FFT, |values| ~ 1 after ortho scaling (as the power-of-two test)
        np.testing.assert_allclose(torch.view_as_real(got).numpy(), torch.view_as_real(ref).numpy(), rtol=0, atol=3e-6)
    f = e.fft2c(cg)
    back = e.fft2c(f, inverse=True).cpu()
    np.testing.assert_allclose(torch.view_as_real(back).numpy(), torch.view_as_real(c).numpy(), rtol=0, atol=3e-6)
    # Parseval (ortho): energy preserved
    assert abs(float((f.abs() ** 2).sum()) / float((cg.abs() ** 2).sum()) - 1) < 1e-5


def _prox_inputs(n, h, w, seed):
    xs = torch.from_numpy(synthetic.hash_uniform(seed, 1, n * h * w).reshape(n, 1, h, w))
    u0 = 0.1 * torch.view_as_complex(torch.from_numpy(synthetic.hash_uniform(seed, 2, 2 * n * h * w).reshape(n, 1, h, w, 2).copy()))
    return xs, u0


@pytest.mark.parametrize("h,w", [(320, 320), (640, 320)])
@pytest.mark.parametrize("per_slice_masks", [False, True])
def test_prox_dual_matches_oracle_and_skips_stopped_slices(h, w, per_slice_masks):
    n = 3
    if per_slice_masks:                                        # mask_n == N: every slice its own sampling pattern
        datas = [synthetic.make_problem(1, h, w, accel=acc, seed=70 + i) for i, acc in enumerate((2.0, 4.0, 8.0))]
        masks = torch.stack([torch.from_numpy(np.asarray(d["mask"])).reshape(h, w).bool() for d in datas])
        assert not torch.equal(masks[0], masks[2])
        y0 = torch.cat([torch.view_as_complex(torch.from_numpy(d["y0"])) for d in datas])
        x0 = torch.cat([torch.view_as_complex(torch.from_numpy(d["x0"])) for d in datas])
    else:
        data = synthetic.make_problem(n, h, w, accel=4.0, seed=99)
        masks = torch.from_numpy(np.asarray(data["mask"])).reshape(1, h, w).bool().expand(n, h, w)
        y0 = torch.view_as_complex(torch.from_numpy(data["y0"]))
        x0 = torch.view_as_complex(torch.from_numpy(data["x0"]))
    e = _kspace_engine(n, h, w)
    x, z, u = e.reset(x0.cuda(), y0.cuda(), masks.cuda() if per_slice_masks else masks[0].cuda())
    np.testing.assert_array_equal(x.cpu().numpy(), x0.real.numpy())
    assert float(u.abs().max()) == 0.0
    xs, u0 = _prox_inputs(n, h, w, 8)
    xd = torch.clamp(x0.real + 0.05 * xs, 0, 1)
    mu = torch.tensor([0.07, 0.3, 0.55])
    xg, ug = xd.cuda(), u0.cuda().clone()
    zg = torch.empty_like(ug)
    e.prox_dual(xg, zg, ug, mu.cuda())
    for i in range(n):
        zf = O.fft2c(xd[i:i + 1] + u0[i:i + 1])
        temp = (mu[i] * zf + y0[i:i + 1]) / (1 + mu[i])
        zn = O.ifft2c(torch.where(masks[i].reshape(1, 1, h, w), temp, zf))
        # FLOAT TOLERANCE: two f32 FFTs + pointwise, data O(1)
        np.testing.assert_allclose(torch.view_as_real(zg[i:i + 1].cpu()).numpy(), torch.view_as_real(zn).numpy(), rtol=0, atol=5e-6)
        np.testing.assert_allclose(torch.view_as_real(ug[i:i + 1].cpu()).numpy(),
                                   torch.view_as_real(u0[i:i + 1] + xd[i:i + 1] - zn).numpy(), rtol=0, atol=5e-6)
    # a slice whose t_action > 0.5 keeps x, z, u bit for bit; the others move
    before = [t.clone() for t in (xg, zg, ug)]
    tact = torch.tensor([0.0, 0.9, 0.2]).cuda()
    e.prox_dual(xg, zg, ug, mu.cuda(), t_action=tact)
    for b, a in zip(before, (xg, zg, ug)):
        assert torch.equal(b[1], a[1])
    assert not torch.equal(before[2][0], ug[0]) and not torch.equal(before[2][2], ug[2])


def test_trajectories_match_reference_runs_at_320_and_640x320(denoiser, golden_dir):
    """2 slices of 320 x 320 stepped as ONE batch, and 1 slice of 640 x 320, with per-slice (mu, sigma) tables == the reference's
    own single-slice runs (g10_radix5.npz), every iteration within the PSNR tolerance."""
    g = np.load(os.path.join(golden_dir, "g10_radix5.npz"))
    iters = int(g["iters"])
    for tag, n, h, w in (("320", 2, 320, 320), ("640x320", 1, 640, 320)):
        env = _env(denoiser)
        st = env.reset(_mat(synthetic.make_problem(n, h, w, accel=4.0, sigma_n=10.0 / 255.0, seed=1234)), "cuda")
        mu, sg = torch.from_numpy(g[f"mu_tab_{tag}"]).cuda(), torch.from_numpy(g[f"sig_tab_{tag}"]).cuda()
        ps = np.zeros((n, iters))
        for t in range(iters):
            st, done = env.step(st, {"T": torch.zeros(n), "mu": mu[:, t], "sigma_d": sg[:, t]})
            assert not bool(torch.as_tensor(done).any())      # (a bool for one slice, as the reference's)
            ps[:, t] = env.compute_reward(st["x"], st["gt"])[:, 0].numpy()
        assert np.abs(ps - g[f"psnr_{tag}"]).max() < PSNR_TOL_DB, tag
        xf = st["x"].cpu().numpy()[:, 0].astype(np.float64)
        if tag == "320":
            # FLOAT TOLERANCE: 20 iterations of f32 U-Net + FFTs against the reference's f32 torch run (as G4 at 256)
            np.testing.assert_allclose(xf, g["x_final_320"], rtol=0, atol=1e-4)
        else:
            s, l2 = xf.reshape(n, -1).sum(axis=1), np.sqrt((xf.reshape(n, -1) ** 2).sum(axis=1))
            np.testing.assert_allclose(s, g[f"x_sum_{tag}"], rtol=1e-4, atol=0)
            np.testing.assert_allclose(l2, g[f"x_l2_{tag}"], rtol=1e-4, atol=0)


def test_ten_steps_at_320_are_bitwise_repeatable(denoiser):
    data = synthetic.make_problem(2, 320, 320, accel=4.0, seed=31)
    mu_tab, sig_tab = synthetic.param_table(2, 10, seed=77)
    runs = []
    for _ in range(2):
        env = _env(denoiser)
        st = env.reset(_mat(data), "cuda")
        for t in range(10):
            st, _ = env.step(st, {"T": torch.zeros(2), "mu": torch.from_numpy(mu_tab[:, t]), "sigma_d": torch.from_numpy(sig_tab[:, t])})
        torch.cuda.synchronize()
        runs.append({k: st[k].clone() for k in ("x", "z", "u")})
    for k in ("x", "z", "u"):
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_bf16_handle_steps_at_320_and_its_kspace_stage_is_the_f32_one(denoiser):
    from dt4image_restoration_amd import weights
    from dt4image_restoration_amd.engine import PnPEngine
    n, h, w = 2, 320, 320
    data = synthetic.make_problem(n, h, w, accel=4.0, seed=41)
    x0 = torch.view_as_complex(torch.from_numpy(data["x0"])).cuda()
    y0 = torch.view_as_complex(torch.from_numpy(data["y0"])).cuda()
    mask = torch.from_numpy(np.asarray(data["mask"])).reshape(h, w).cuda()
    sd = weights.generate_unet_weights(0, "unit_gain")
    outs = []
    for bf16 in (False, True):
        e = PnPEngine(n, h, w, bf16_convs=bf16)
        e.load_weights(sd)
        assert (e.bf16_weight_terms() > 0) == bf16
        e.reset(x0, y0, mask)
        xs, u0 = _prox_inputs(n, h, w, 12)
        xg, ug = torch.clamp(x0.real.cpu() + 0.05 * xs, 0, 1).cuda(), u0.cuda()
        zg = torch.empty_like(ug)
        e.prox_dual(xg, zg, ug, torch.tensor([0.1, 0.4]).cuda())
        torch.cuda.synchronize()
        outs.append((zg.clone(), ug.clone()))
        if bf16:                                               # and the whole step runs: finite iterates, a sane PSNR
            x, z, u = e.reset(x0, y0, mask)
            for _ in range(3):
                e.step(x, z, u, torch.tensor([0.1, 0.3]).cuda(), torch.tensor([15 / 255.0, 25 / 255.0]).cuda())
            gt = torch.from_numpy(data["gt"]).cuda()
            assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(torch.view_as_real(u)).all())
            assert bool(((e.psnr(x, gt) > 20) & (e.psnr(x, gt) < 50)).all())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_greedy_rollout_and_cli_eval_at_320():
    from dt4image_restoration_amd import cli, data as D, weights
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.drivers.greedy import GreedyEvaluator
    from dt4image_restoration_amd.env import PnPEnv
    from dt4image_restoration_amd.policy import DecisionTransformer, DecisionTransformerConfig
    m = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    m.load_state_dict(weights.generate_policy_weights(m, 7, t_bias=-1.0, head_gain=8.0))
    mat = _mat(synthetic.make_problem(2, 320, 320, accel=4.0, seed=19))
    ev = GreedyEvaluator(m, PnPEnv(30, UNetDenoiser2D.seeded(0), "cuda"), max_timesteps=4, device_type="cuda", ssim=True)
    r = ev.run(mat, torch.full((2,), D.normalised_rtg(10.0)), torch.tensor([4, 4]))
    assert bool(torch.isfinite(r.reward).all()) and bool(((r.reward > 15) & (r.reward < 50)).all())
    assert bool(torch.isfinite(r.ssim).all()) and bool(((r.ssim > 0) & (r.ssim <= 1)).all())
    out = cli.main(["--block_size", "18", "--n_embeds", "9", "--size", "320", "--limit", "2", "eval", "--rtg", "10", "--max_timesteps", "3"])
    assert len(out) == 2
    for o in out:
        assert o["n"] == 2 and np.isfinite(o["psnr"]) and 15 < o["psnr"] < 50 and np.isfinite(o["ssim"]) and 0 < o["ssim"] <= 1


@pytest.mark.parametrize("h,w", [(368, 320), (96, 96)])
def test_other_sizes_are_still_refused_with_the_supported_list(h, w):
    from dt4image_restoration_amd._lib import PnPError
    e = _kspace_engine(1, h, w)
    data = synthetic.make_problem(1, h, w, accel=4.0, seed=3)
    x0 = torch.view_as_complex(torch.from_numpy(data["x0"])).cuda()
    y0 = torch.view_as_complex(torch.from_numpy(data["y0"])).cuda()
    with pytest.raises(PnPError) as ei:
        e.reset(x0, y0, torch.from_numpy(np.asarray(data["mask"])).reshape(h, w).cuda())
    msg = str(ei.value)
    assert "320" in msg and "800" in msg and "1024" in msg and f"{h}x{w}" in msg
    with pytest.raises(PnPError):
        e.fft2c(x0)
