"""ADMM residuals on the MI355X (pnp_residuals) against the float64 restatement of tests/residual_ref.py, the exact cases (zero change,
reproducibility, position in the batch, columns not asked for, error paths), the pinned trajectory against the CPU oracle, the
fixed-schedule solver's stop, and the layers above: CLI `fixed`, `eval --residuals`, `mcts --scorer neg_dc`.

Bounds (include/pnpadmm.h; each figure is printed before it is asserted):
  * columns 0-3: relative 5e-7 - the difference is one float32 rounding (2^-24), the sums are float64, the root and the cast add two
    more: three rounding units of 6e-8, and one is allowed for the library's sqrt;
  * column 4 against (c1 + c2 + c3) / sqrt(HW) in float64 from the returned columns: relative 5e-7 (the same three roundings);
  * column 5: |dc_gpu - dc_64| <= 1e-6 ||x|| + 5e-7 dc_64 - the project's asserted bound on pnp_fft2c (1e-6 relative RMS) carried
    through the triangle inequality, plus the roundings above."""
import json

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import _lib
import residual_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64, 64), (2, 128, 128), (64, 256, 256), (2, 320, 320), (1, 640, 320), (2, 16, 1024), (5, 16, 16), (2, 80, 400)]
REL = 5e-7


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def _state(n, h, w, seed, per_slice_mask=False):
    """Random iterate and previous iterate, random y0, a random mask (shared [h,w] or one per slice)."""
    g = torch.Generator().manual_seed(seed)
    rc = lambda: torch.complex(torch.randn(n, 1, h, w, generator=g), torch.randn(n, 1, h, w, generator=g))
    x, z, u = torch.rand(n, 1, h, w, generator=g), rc(), 0.3 * rc()
    xp = x + 0.05 * torch.randn(n, 1, h, w, generator=g)
    zp, up = z + 0.05 * rc(), u + 0.02 * rc()
    y0 = rc()
    mask = torch.rand((n, h, w) if per_slice_mask else (h, w), generator=g) < 0.3
    return x, z, u, xp, zp, up, y0, mask


def _install(e, y0, mask):
    e.set_kspace(y0.cuda().contiguous(), mask.cuda())


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


@pytest.mark.parametrize("per_slice_mask", [False, True])
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_all_columns_against_float64(n, h, w, per_slice_mask):
    x, z, u, xp, zp, up, y0, mask = _state(n, h, w, seed=h * 131 + w + n, per_slice_mask=per_slice_mask)
    e = _engine(n, h, w)
    _install(e, y0, mask)
    xc, zc, uc = x.cuda(), z.cuda(), u.cuda()
    prev = e.snapshot(xp.cuda(), zp.cuda(), up.cuda())                  # a real pnp_snapshot
    got = e.residuals(xc, zc, uc, prev=prev, dc=True).cpu().double().numpy()
    ref = R.residuals_ref(x, z, u, (xp, zp, up), y0, mask)
    assert got.shape == (n, 6)
    r03 = _rel(got[:, :4], ref[:, :4])
    c4 = (got[:, 1] + got[:, 2] + got[:, 3]) / np.sqrt(float(h * w))
    r4 = _rel(got[:, 4], c4)
    xn = np.sqrt((x.double().numpy().reshape(n, -1) ** 2).sum(1))
    ddc = np.abs(got[:, 5] - ref[:, 5])
    bound = 1e-6 * xn + REL * ref[:, 5]
    print(f"{n}x{h}x{w} mask_n={'N' if per_slice_mask else 1}: rel err cols 0-3 = {r03:.3e}, col 4 = {r4:.3e}, "
          f"|ddc| / bound = {float((ddc / bound).max()):.3e} (|ddc| max {float(ddc.max()):.3e})")
    assert r03 <= REL
    assert r4 <= REL
    assert (ddc <= bound).all()


@pytest.mark.parametrize("n,h,w", [(3, 64, 64), (2, 320, 320)])
def test_x_close_to_z_and_consistent_data(n, h, w):
    """x within a few float32 units of z: the bound holds against the float64 norm of the float32 difference.  And y0 = mask * fft_c(x):
    the misfit comes out below 1e-6 ||x||."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, 1, h, w, generator=g)
    z = torch.complex(x * (1 + 3e-7 * torch.randn(n, 1, h, w, generator=g)), 1e-7 * torch.randn(n, 1, h, w, generator=g))
    u = torch.zeros_like(z)
    mask = torch.rand(h, w, generator=g) < 0.3
    y0 = torch.from_numpy(np.where(mask.numpy(), R.fft2c64(x.double().numpy()), 0)).to(torch.complex64)
    e = _engine(n, h, w)
    _install(e, y0, mask)
    got = e.residuals(x.cuda(), z.cuda(), u.cuda(), dc=True).cpu().double().numpy()
    d32 = torch.complex(x - z.real, -z.imag)                          # the float32 difference, as the kernel forms it
    ref = np.sqrt((d32.abs().double().numpy().reshape(n, -1) ** 2).sum(1))
    xn = np.sqrt((x.double().numpy().reshape(n, -1) ** 2).sum(1))
    print(f"{n}x{h}x{w}: primal {got[:, 0]} rel err {_rel(got[:, 0], ref):.3e}; dc / ||x|| = {float((got[:, 5] / xn).max()):.3e}")
    assert (ref > 0).all() and _rel(got[:, 0], ref) <= REL
    assert (got[:, 5] < 1e-6 * xn).all()
    assert (got[:, 1:5] == 0).all()


def test_exact_cases():
    n, h, w = 3, 128, 80
    x, z, u, xp, zp, up, y0, mask = _state(n, h, w, seed=9)
    e = _engine(n, h, w)
    _install(e, y0, mask)
    xc, zc, uc = x.cuda(), z.cuda(), u.cuda()
    same = e.snapshot(xc, zc, uc)
    r = e.residuals(xc, zc, uc, prev=same, dc=True)
    assert bool((r[:, 1:5] == 0).all()) and bool((r[:, 0] > 0).all()) and bool((r[:, 5] > 0).all())
    prev = e.snapshot(xp.cuda(), zp.cuda(), up.cuda())
    a = e.residuals(xc, zc, uc, prev=prev, dc=True)
    b = e.residuals(xc, zc, uc, prev=prev, dc=True)
    assert torch.equal(a, b)                                           # two calls: the same bits
    # columns that were not asked for are 0, the others keep their bits
    only_delta = e.residuals(xc, zc, uc, prev=prev)
    only_dc = e.residuals(xc, zc, uc, dc=True)
    plain = e.residuals(xc, zc, uc)
    assert torch.equal(only_delta[:, :5], a[:, :5]) and bool((only_delta[:, 5] == 0).all())
    assert torch.equal(only_dc[:, 5], a[:, 5]) and torch.equal(only_dc[:, 0], a[:, 0]) and bool((only_dc[:, 1:5] == 0).all())
    assert torch.equal(plain[:, 0], a[:, 0]) and bool((plain[:, 1:] == 0).all())


@pytest.mark.parametrize("h,w", [(64, 64), (320, 320)])
def test_position_in_the_batch_does_not_change_the_bits(h, w):
    x, z, u, xp, zp, up, y0, mask = _state(3, h, w, seed=21, per_slice_mask=True)
    e3 = _engine(3, h, w)
    _install(e3, y0, mask)
    a = e3.residuals(x.cuda(), z.cuda(), u.cuda(), prev=e3.snapshot(xp.cuda(), zp.cuda(), up.cuda()), dc=True).cpu()
    g = torch.Generator().manual_seed(22)
    pad = lambda t: torch.cat([(torch.randn(5, *t.shape[1:], generator=g).to(t.dtype) if not t.is_complex() else
                                torch.complex(torch.randn(5, *t.shape[1:], generator=g), torch.randn(5, *t.shape[1:], generator=g))), t])
    e8 = _engine(8, h, w)
    mask8 = torch.cat([torch.rand(5, h, w, generator=g) < 0.5, mask])
    _install(e8, pad(y0), mask8)
    b = e8.residuals(pad(x).cuda(), pad(z).cuda(), pad(u).cuda(), prev=e8.snapshot(pad(xp).cuda(), pad(zp).cuda(), pad(up).cuda()),
                     dc=True).cpu()[5:]
    assert torch.equal(a[:, :5], b[:, :5])
    ref = R.residuals_ref(x, z, u, None, y0, mask)[:, 5]
    xn = np.sqrt((x.double().numpy().reshape(3, -1) ** 2).sum(1))
    assert (np.abs(b[:, 5].double().numpy() - ref) <= 1e-6 * xn + REL * ref).all()


def test_error_paths_leave_out_untouched():
    n, h, w = 2, 64, 64
    x, z, u, xp, zp, up, y0, mask = _state(n, h, w, seed=3)
    e = _engine(n, h, w)                                              # no reset yet
    xc, zc, uc = x.cuda(), z.cuda(), u.cuda()
    out = torch.full((n, 6), 7.0, device="cuda")
    with pytest.raises(_lib.PnPError, match=r"\(-3\).*pnp_reset"):   # PNP_ERR_STATE
        e.residuals(xc, zc, uc, dc=True, out=out)
    lib, hnd, st = e.lib, e._h, e._stream()
    prev = e.snapshot(xp.cuda(), zp.cuda(), up.cuda())
    cases = [((hnd, None, zc.data_ptr(), uc.data_ptr(), None, 0, out.data_ptr(), st), b"null x"),
             ((hnd, xc.data_ptr(), zc.data_ptr(), uc.data_ptr(), None, 1, out.data_ptr(), st), b"prev"),
             ((hnd, xc.data_ptr(), zc.data_ptr(), uc.data_ptr(), prev.data_ptr(), 8, out.data_ptr(), st), b"flag"),
             ((hnd, xc.data_ptr() + 4, zc.data_ptr(), uc.data_ptr(), None, 0, out.data_ptr(), st), b"aligned")]
    for args, what in cases:
        assert lib.pnp_residuals(*args) == -1 and what in lib.pnp_last_error(), lib.pnp_last_error()
    with pytest.raises(ValueError, match="snapshot"):
        e.residuals(xc, zc, uc, prev=prev[:-4])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ok = e.residuals(xc, zc, uc, prev=prev, out=out)                   # works before a reset without PNP_RES_DC, into `out`
    assert ok.data_ptr() == out.data_ptr() and bool((out[:, 0] > 0).all())


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_denoiser_handles_and_a_side_stream(kind):
    """Any handle kind, on the caller's stream."""
    n, h, w = 2, 64, 64
    x, z, u, xp, zp, up, y0, mask = _state(n, h, w, seed=4)
    e = _engine(n, h, w, denoiser=True, bf16_convs=(kind == "bf16"))
    _install(e, y0, mask)
    ref = R.residuals_ref(x, z, u, (xp, zp, up), y0, mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xc, zc, uc = x.cuda(), z.cuda(), u.cuda()
        got = e.residuals(xc, zc, uc, prev=e.snapshot(xp.cuda(), zp.cuda(), up.cuda()), dc=True)
    side.synchronize()
    got = got.cpu().double().numpy()
    assert _rel(got[:, :4], ref[:, :4]) <= REL


# ---- PnPEnv.residuals, the trajectory, the solver ---------------------------------------------------------------------------
def _env():
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    return PnPEnv(max_episode_step=30, denoiser=UNetDenoiser2D.seeded(0, "unit_gain"), device_type="cuda")


def _mat():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in R.trajectory_problem().items()}


def test_env_residuals_packed_and_per_tensor_snapshots_agree():
    env = _env()
    st = env.reset(_mat(), "cuda")
    n = st["z"].shape[0]
    act = {"T": torch.zeros(n), "mu": torch.full((n,), R.TRAJ_MU), "sigma_d": torch.full((n,), R.TRAJ_SIGMA)}
    packed = env.snapshot(st)
    loose = {k: st[k].clone() for k in ("x", "z", "u", "T")}          # the per-tensor form: packed by the shim first
    assert "packed" in packed
    st, _ = env.step(st, act)
    a = env.residuals(st, prev=packed, dc=True)
    b = env.residuals(st, prev=loose, dc=True)
    assert torch.equal(a, b) and a.shape == (n, 6) and bool((a > 0).all())
    with pytest.raises(ValueError, match="elements"):
        env.residuals(st, prev={k: v[:1] for k, v in loose.items()})
    ref = R.residuals_ref(st["x"], st["z"], st["u"], (loose["x"], loose["z"], loose["u"]), st["y0"], st["mask"])
    assert _rel(a.cpu().double().numpy()[:, :4], ref[:, :4]) <= REL


def test_trajectory_against_the_oracle():
    """GPU delta within 2e-4 of the oracle's at every iteration: the project bounds the pointwise iterate error against the oracle
    by 2e-5 over 30 iterations; two consecutive iterates of x, z and u then move delta by at most
    2 (1 + 2 sqrt 2) 2e-5 = 1.5e-4."""
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    want = R.oracle_trajectory()
    r = FixedScheduleSolver(_env(), max_iter=R.TRAJ_ITERS, dc=True).run(
        _mat(), np.full((R.TRAJ_N, R.TRAJ_ITERS), R.TRAJ_MU, np.float32), np.full((R.TRAJ_N, R.TRAJ_ITERS), R.TRAJ_SIGMA, np.float32))
    d = r.delta.double().numpy().T
    err = np.abs(d - want[:, :, 4])
    print("GPU delta:", " ".join(f"{v:.6f}" for v in d[:, 0]), "|", " ".join(f"{v:.6f}" for v in d[:, 1]))
    print(f"max |delta_gpu - delta_oracle| = {err.max():.3e}; max |primal diff| = {np.abs(r.primal.double().numpy().T - want[:, :, 0]).max():.3e}; "
          f"|dc diff| = {np.abs(r.dc.double().numpy() - want[-1, :, 5]).max():.3e}")
    assert err.max() <= 2e-4
    assert r.iterations.tolist() == [R.TRAJ_ITERS] * R.TRAJ_N and r.steps == R.TRAJ_ITERS


def _solve(tol, mu=(R.TRAJ_MU, R.TRAJ_MU), max_iter=R.TRAJ_ITERS, sync_every=1):
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    mu_tab = np.tile(np.asarray(mu, np.float32)[:, None], (1, max_iter))
    return FixedScheduleSolver(_env(), max_iter=max_iter, tol=tol, sync_every=sync_every).run(
        _mat(), mu_tab, np.full((R.TRAJ_N, max_iter), R.TRAJ_SIGMA, np.float32))


@pytest.mark.parametrize("sync_every", [1, 5])
def test_both_slices_stop_at_iteration_8(sync_every):
    r = _solve(R.STOP_TOL, sync_every=sync_every)
    d = r.delta.numpy()
    print("delta at 7, 8:", d[:, R.STOP_ITER - 2], d[:, R.STOP_ITER - 1], "iterations", r.iterations.tolist(), "steps", r.steps)
    assert r.iterations.tolist() == [R.STOP_ITER] * R.TRAJ_N
    assert r.steps == -(-R.STOP_ITER // sync_every) * sync_every
    assert (d[:, R.STOP_ITER:] == d[:, R.STOP_ITER - 1:R.STOP_ITER]).all()
    assert (r.primal.numpy()[:, R.STOP_ITER:] == r.primal.numpy()[:, R.STOP_ITER - 1:R.STOP_ITER]).all()
    short = _solve(None, max_iter=R.STOP_ITER)                        # bit-identical from the stop on: the iterate of iteration 8
    torch.cuda.synchronize()
    assert torch.equal(r.x, short.x) and torch.equal(r.z, short.z) and torch.equal(r.u, short.u)


def test_slices_stop_at_different_iterations():
    r = _solve(R.SPLIT_TOL, mu=R.SPLIT_MU)
    free = _solve(None, mu=R.SPLIT_MU)
    a, b = R.SPLIT_ITERS
    d, f = r.delta.numpy(), free.delta.numpy()
    print("iterations", r.iterations.tolist(), "delta slice 0:", d[0, a - 2:a], "slice 1:", d[1, b - 2:b])
    assert tuple(r.iterations.tolist()) == R.SPLIT_ITERS
    assert (d[0, a:] == d[0, a - 1]).all() and (d[1, b:] == d[1, b - 1]).all()
    # the stopped slice is bit-identical from its stop on ...
    early = _solve(None, mu=R.SPLIT_MU, max_iter=a)
    torch.cuda.synchronize()
    assert torch.equal(r.x[0], early.x[0]) and torch.equal(r.z[0], early.z[0]) and torch.equal(r.u[0], early.u[0])
    # ... and the other slice matches the run without the stop (the engine's slices are independent: the same bits), up to its own stop
    assert (d[1, :b] == f[1, :b]).all() and (r.primal.numpy()[1, :b] == free.primal.numpy()[1, :b]).all()
    until_b = _solve(None, mu=R.SPLIT_MU, max_iter=b)
    assert torch.equal(r.x[1], until_b.x[1]) and torch.equal(r.z[1], until_b.z[1]) and torch.equal(r.u[1], until_b.u[1])


# ---- drivers and CLI --------------------------------------------------------------------------------------------------------
def _cli(capsys, argv):
    from dt4image_restoration_amd import cli
    out = cli.main(argv)
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if l.startswith("{")]
    assert [json.loads(l) for l in lines] == out
    return lines, out


def test_cli_fixed(capsys):
    base = ["--block_size", "18", "--n_embeds", "9", "--size", "64", "--limit", "2"]
    lines, out = _cli(capsys, base + ["fixed", "--mu", "0.3", "--sigma-start", "15", "--sigma-end", "15", "--tol", "0.02",
                                      "--max_iter", "16", "--dc"])
    assert len(out) == 2
    for o in out:
        for k in ("set", "n", "psnr", "psnr_increment", "mean_stop_iteration", "ranks", "iterations", "delta", "primal", "dc"):
            assert k in o, k
        assert o["n"] == 2 and len(o["iterations"]) == 2 and all(1 <= i <= 16 for i in o["iterations"])
        assert o["delta"] > 0 and o["primal"] > 0 and o["dc"] > 0 and o["psnr_increment"] > 0
    print(lines)
    assert all(i < 16 for i in out[0]["iterations"])                  # the tolerance stops the 4x set before max_iter (delta starts near 0.05)
    _, full = _cli(capsys, base + ["fixed", "--tol", "0", "--max_iter", "5"])
    assert all(o["iterations"] == [5, 5] and "dc" not in o for o in full)   # --tol 0 runs max_iter steps


def test_cli_eval_residuals_adds_two_fields_and_nothing_else(capsys):
    base = ["--block_size", "18", "--n_embeds", "9", "--limit", "2", "eval", "--max_timesteps", "4"]
    plain, _ = _cli(capsys, base)
    with_res, out = _cli(capsys, base + ["--residuals"])
    assert len(plain) == len(with_res) == 2
    for p, w, o in zip(plain, with_res, out):
        assert w.startswith(p[:-1] + ", ")                           # no other byte of the line changes
        assert list(o)[-2:] == ["primal", "dc"] and o["primal"] > 0 and o["dc"] > 0
        assert json.loads(p) == {k: v for k, v in o.items() if k not in ("primal", "dc")}


def test_cli_mcts_neg_dc_scorer_runs(capsys):
    _, out = _cli(capsys, ["--block_size", "18", "--n_embeds", "9", "--limit", "2", "mcts", "--max_timesteps", "4", "--rollouts", "3",
                           "--scorer", "neg_dc"])
    assert len(out) == 2 and all(np.isfinite(o["mcts_psnr"]) and o["mcts_psnr"] > 0 for o in out)
