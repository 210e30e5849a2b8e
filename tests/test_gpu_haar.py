"""The Haar wavelet prior (pnp_haar_denoise, pnp_set_prior_haar / pnp_get_prior_haar, pnp_step under PNP_PRIOR_HAAR) on the MI355X, through
the C ABI (PnPEngine is the ctypes binding), against the float64 restatement of tests/haar_ref.py computed from the float32 input the device
is handed.  Every figure is printed and attached with record_property before it is asserted.

CASES (haar_ref.CASES; phantoms plus seeded noise of sigma 0.04, slice 0 of every case stretched to [-0.15, 1.15]; thresholds per slice):

      N  H    W    lam per slice      covers
      2  16   16   0.2, 0             at J = 4 the whole image is one block and every halo pixel is a wrap
      1  16   48   0.05               thin in one axis
      1  48   16   1e-6               the same the other way
      3  64   80   0.05, 1e-6, 10     a 2^a 5^b side, non-square
      1  112  128  0.2                tile seams: at J = 4 (tile 98) the second row of tiles is 14 pixels high, less than the halo of 15; the
                                      128 side crosses the seam at every J (tiles 126, 122, 114, 98)
      2  208  144  10, 0.05           ragged on both axes

levels in 1..4, both modes.

BOUNDS.  max |out - ref| is within TEN TIMES the error of the float32 restatement (haar_ref.haar(f32=True), the header's expression order)
against the float64 one, measured on the CPU by tests/test_haar_host.py (haar_ref.F32_ERR), per mode, case and level count:

      ti     J = 1       2           3           4              ortho  J = 1       2           3           4
      0      3.725e-08   4.459e-08   5.147e-08   5.185e-08      0      3.725e-08   6.286e-08   8.708e-08   5.532e-08
      1      3.353e-08   3.702e-08   3.469e-08   3.944e-08      1      2.980e-08   5.588e-08   4.889e-08   5.427e-08
      2      2.486e-08   2.895e-08   2.964e-08   2.873e-08      2      2.316e-08   2.486e-08   2.895e-08   2.945e-08
      3      5.215e-08   6.566e-08   7.210e-08   9.400e-08      3      5.960e-08   9.686e-08   1.127e-07   1.705e-07
      4      5.588e-08   7.043e-08   7.854e-08   7.124e-08      4      5.960e-08   1.006e-07   1.029e-07   1.313e-07
      5      5.960e-08   8.265e-08   9.692e-08   1.276e-07      5      6.706e-08   1.267e-07   1.974e-07   2.205e-07

Haar-ADMM (haar_ref.FIXTURE: TV's fixture - 1 x 64 x 80, 4x, sigma 5/255, seed 1234, mu 0.3, sigma_d 50/255 -> 5/255 geometric over 30
iterations - with haar_scale 1, 3 levels, TI) through FixedScheduleSolver with HaarDenoiser2D: the first 10 iterations against the float64
loop within ten times the float32 restatement's |dPSNR| = 2.824e-07 dB and max |dx| = 2.303e-07 (haar_ref.ADMM_F32); the 30 iterations
end at least 3 dB above x0 (the reference: 28.256 -> 34.824 dB).

Multi-coil step (2 x 64 x 64, 4 coils, sense_ref.solve_case, mu 0.3, K = 8, defaults): x against haar_ref within ten times the float32
restatement's error on that input (measured in the test, on the CPU), z against sense_ref.prox_dual fed the reference's x under
test_gpu_sense.py's bound for (0.3, 8): ten times (1.040e-06, 3.780e-07).

Everything else is bit for bit.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as GB  # noqa: E402
import haar_ref as R  # noqa: E402
import sense_ref as SR  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic, weights  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0
SENSE_F32 = (1.040e-06, 3.780e-07)                         # test_gpu_sense.py, F32[(0.3, 8)]: err_max, err_rms
DEV = "cuda"
C64, F32T, U8 = torch.complex64, torch.float32, torch.uint8
NAIVE_PLANES = 5                                           # a_1 .. a_3 and two residual planes: 20 n H W bytes


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def _naive_engine(monkeypatch, n, h, w):
    monkeypatch.setenv("PNP_HAAR_NAIVE", "1")              # read at pnp_create
    e = _engine(n, h, w)
    monkeypatch.delenv("PNP_HAAR_NAIVE")
    return e


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def c64(a):
    return torch.from_numpy(np.array(a, dtype=np.complex64)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _case(i):
    v, lam = R.case_input(i)
    n, h, w = R.CASES[i]
    return f32(v).reshape(n, 1, h, w), f32(lam)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("levels", R.CASE_LEVELS)
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_haar_denoise_against_float64(i, levels, mode, record_property):
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    out = _engine(n, h, w).haar_denoise(v, lam, levels, mode)
    assert out.shape == (n, 1, h, w) and out.dtype == F32T
    err = float(np.abs(_np(out)[:, 0] - R.case_ref(i, levels, mode)).max())
    own = R.F32_ERR[mode][i][R.CASE_LEVELS.index(levels)]
    bound = MARGIN * own
    print(f"case {i} {n}x{h}x{w} lam {lam.tolist()} {mode} J {levels}: max |out - ref| {err:.3e} (float32 restatement {own:.3e}) / {bound:.2e}")
    record_property("max_abs_err", err); record_property("bound", bound)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert err <= bound


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_fused_and_naive_give_the_same_bits(i, monkeypatch):
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    fused, naive = _engine(n, h, w), _naive_engine(monkeypatch, n, h, w)
    for levels in R.CASE_LEVELS:
        assert _same(fused.haar_denoise(v, lam, levels), naive.haar_denoise(v, lam, levels)), levels
    for e in (fused, naive):                                                       # out aliasing x_in == not aliasing, in both forms and modes
        for levels in (1, 4):
            for mode in R.MODES:
                want = e.haar_denoise(v, lam, levels, mode)
                buf = v.clone()
                assert e.haar_denoise(buf, lam, levels, mode, out=buf) is buf
                assert _same(buf, want), (levels, mode)


def test_a_slice_gives_the_same_bits_alone_at_every_place_of_a_batch_on_a_side_stream_twice_and_on_every_handle_kind():
    i = 3
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    e3 = _engine(n, h, w)
    for levels, mode in ((3, "ti"), (4, "ti"), (3, "ortho")):
        base = e3.haar_denoise(v, lam, levels, mode)
        assert _same(e3.haar_denoise(v, lam, levels, mode), base)                  # two calls in a row
        assert not _same(base[0], base[1]) and not _same(base[1], base[2])
        e1 = _engine(1, h, w)
        for j in range(n):                                                         # alone
            assert _same(e1.haar_denoise(v[j:j + 1].clone(), lam[j:j + 1].clone(), levels, mode)[0], base[j]), j
        for shift in (1, 2):                                                       # at the two other places
            perm = [(j + shift) % n for j in range(n)]
            got = e3.haar_denoise(v[perm].contiguous(), lam[perm].contiguous(), levels, mode)
            for k, j in enumerate(perm):
                assert _same(got[k], base[j]), (shift, k)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = e3.haar_denoise(v, lam, levels, mode)
        side.synchronize()
        assert _same(got, base)
        unet, bf16 = _engine(n, h, w, denoiser=True), _engine(n, h, w, denoiser=True, bf16_convs=True)   # no weights are needed
        assert _same(unet.haar_denoise(v, lam, levels, mode), base) and _same(bf16.haar_denoise(v, lam, levels, mode), base)
        mc = _engine(n, h, w)                                                      # a handle in multi-coil mode
        sens = c64(synthetic.coil_maps(2, h, w))
        mc.set_kspace(torch.zeros((n, 2, h, w), dtype=C64, device=DEV), torch.ones((h, w), dtype=U8, device=DEV), sens=sens, cg_iters=2)
        assert _same(mc.haar_denoise(v, lam, levels, mode), base) and mc.coils == 2


@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 112, 128), (1, 208, 144)])
def test_a_constant_image_returns_itself_and_lam_zero_is_the_clamp(shape):
    n, h, w = shape
    e = _engine(n, h, w)
    lam = torch.tensor([0.2, 1e-6][:n], device=DEV)
    for mode in R.MODES:
        for c in (0.0, 0.3, 1.0):
            v = torch.full((n, 1, h, w), c, dtype=F32T, device=DEV)
            for levels in R.CASE_LEVELS:
                assert _same(e.haar_denoise(v, lam, levels, mode), v), (c, levels, mode)
        assert _same(e.haar_denoise(torch.full((n, 1, h, w), 1.5, device=DEV), lam, 3, mode), torch.ones((n, 1, h, w), device=DEV))
        g = torch.Generator().manual_seed(3)
        v = (torch.randn((n, 1, h, w), generator=g) * 0.8 + 0.5).to(DEV)
        for levels in (1, 4):
            assert _same(e.haar_denoise(v, torch.zeros(n, device=DEV), levels, mode), torch.clamp(v, 0, 1))


@pytest.mark.parametrize("i", [0, 4, 5])
def test_ti_commutes_with_every_circular_shift_and_ortho_with_shifts_by_block_multiples(i):
    """The test of the tile seams and of the periodic wrap: a shifted image meets the seams elsewhere, and must give the shifted result."""
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    e = _engine(n, h, w)
    big = (R.tile(4) + 32, R.tile(1) - 25)                                         # larger than a tile where the image is; wraps where it is not
    for levels in R.CASE_LEVELS:
        base = e.haar_denoise(v, lam, levels, "ti")
        for s in ((1, 0), (0, 7), (15, 15), big):
            got = e.haar_denoise(torch.roll(v, s, dims=(2, 3)).contiguous(), lam, levels, "ti")
            assert _same(got, torch.roll(base, s, dims=(2, 3))), (levels, s)
        base = e.haar_denoise(v, lam, levels, "ortho")
        b = 1 << levels
        for s in ((b, 0), (0, 3 * b), (5 * b, 2 * b)):
            got = e.haar_denoise(torch.roll(v, s, dims=(2, 3)).contiguous(), lam, levels, "ortho")
            assert _same(got, torch.roll(base, s, dims=(2, 3))), (levels, s)


# ---- pnp_step under the Haar prior ----------------------------------------------------------------------------------------------------

def _problem(n, h, w, seed=9):
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=seed)
    return (c64(R.cplx(d["x0"])), c64(R.cplx(d["y0"])), torch.from_numpy(d["mask"]).to(DEV), d)


@pytest.mark.parametrize("mode", R.MODES)
def test_a_haar_step_is_haar_denoise_on_re_z_minus_u_then_prox_dual_bit_for_bit_and_stopped_slices_keep_their_bits(mode, monkeypatch):
    n, h, w = 2, 64, 80
    x0, y0, mask, _ = _problem(n, h, w)
    mu = torch.tensor([0.1, 0.4], device=DEV)
    sig = torch.tensor([40.0 / 255.0, 15.0 / 255.0], device=DEV)
    scale, levels = 0.7, 4
    for e in (_engine(n, h, w), _naive_engine(monkeypatch, n, h, w)):
        e.set_haar_prior(scale, levels, mode)
        assert e.haar_settings() == (0.7, 4, mode) and e.prior == "haar" and e.prior_settings() == ("haar", 1.0, 20)
        x, z, u = e.reset(x0, y0, mask)
        xm, zm, um = x.clone(), z.clone(), u.clone()
        t_state, done = torch.zeros(n, device=DEV), torch.full((n,), 7, dtype=U8, device=DEV)
        lam = (torch.tensor(scale, dtype=F32T, device=DEV) * sig).contiguous()
        for _ in range(3):                                                         # (u is zero in the first step only)
            e.step(x, z, u, mu, sig, t_state=t_state, done=done)
            xm = e.haar_denoise((zm.real - um.real).contiguous(), lam, levels, mode)
            e.prox_dual(xm, zm, um, mu)
            assert _same(x, xm) and _same(z, zm) and _same(u, um)
        assert done.tolist() == [0, 0] and torch.allclose(t_state, torch.full((n,), 3.0 / 30.0, device=DEV))
        # slice 0 stopped: all four tensors keep their bits, slice 1 moves as it would alone in the same place
        keep = [t.clone() for t in (x, z, u, t_state)]
        act = torch.tensor([1.0, 0.0], device=DEV)
        e.step(x, z, u, mu, sig, t_action=act, t_state=t_state, done=done)
        assert done.tolist() == [1, 0]
        for t, k in zip((x, z, u, t_state), keep):
            assert _same(t[0], k[0])
        assert not _same(x[1], keep[0][1]) and not _same(z[1], keep[1][1])
        xm = e.haar_denoise((zm.real - um.real).contiguous(), lam, levels, mode)
        e.prox_dual(xm, zm, um, mu)
        assert _same(x[1], xm[1]) and _same(z[1], zm[1]) and _same(u[1], um[1])


def _mat(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def test_haar_admm_through_the_fixed_schedule_solver_against_the_float64_loop(record_property):
    from dt4image_restoration_amd.denoiser import HaarDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    t = R.FIXTURE
    d = R.fixture_problem()
    den = HaarDenoiser2D(scale=t["haar_scale"], levels=t["levels"], mode=t["mode"])
    k = t["compare_iters"]
    mu, sig = R.fixture_schedules(k)
    x64, p0, p64 = R.admm_haar(d, mu, sig)
    env = PnPEnv(max_episode_step=k, denoiser=den, device_type="cuda")
    r = FixedScheduleSolver(env, max_iter=k).run(_mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    dx = float(np.abs(_np(r.x)[:, 0] - x64).max())
    gt = d["gt"][:, 0].astype(np.float64)
    dp = float(np.abs(R.psnr(_np(r.x)[:, 0], gt) - p64).max())                      # both in float64 from the iterate, as the restatement's figure
    bp, bx = (MARGIN * v for v in R.ADMM_F32)
    print(f"{k} Haar-ADMM iterations: PSNR {r.psnr.reshape(-1).tolist()} ref {p64}  |dPSNR| {dp:.3e} / {bp:.2e} dB  max |dx| {dx:.3e} / {bx:.2e}")
    record_property("dpsnr", dp); record_property("max_abs_dx", dx)
    assert env._engine.prior == "haar" and not env._engine.coils
    assert dx <= bx and dp <= bp
    assert abs(float(r.psnr.reshape(-1)[0]) - float(p64[0])) <= 1e-4               # what the engine itself reports (float32)
    mu, sig = R.fixture_schedules()
    env = PnPEnv(max_episode_step=t["iters"], denoiser=den, device_type="cuda")
    r = FixedScheduleSolver(env, max_iter=t["iters"]).run(_mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    gain = float((r.psnr - r.initial_psnr).min())
    print(f"{t['iters']} iterations: PSNR of x0 {r.initial_psnr.reshape(-1).tolist()}, final {r.psnr.reshape(-1).tolist()} (reference {p0} -> 34.824)")
    record_property("psnr_gain", gain)
    assert gain >= 3.0
    out = den(r.x, torch.full((t["n"],), 0.1, device=DEV))                          # the reference's denoiser(x, sigma) call shape
    assert out.shape == r.x.shape and _same(out, env._engine.haar_denoise(r.x, torch.full((t["n"],), 0.1, device=DEV), t["levels"], t["mode"]))


def test_one_multi_coil_haar_step_against_haar_ref_and_sense_ref(record_property):
    n, h, w, coils, K, mu_v = 2, 64, 64, 4, 8, 0.3
    cs = SR.solve_case(h, w, coils, False, "radial", 4)
    e = _engine(n, h, w)
    e.set_haar_prior()
    mask = torch.from_numpy(cs["mask"]).to(DEV)
    x0 = c64(cs["z0"]).reshape(n, 1, h, w)
    x, z, u = e.reset(x0, c64(cs["y"]), mask, sens=c64(cs["sens"]), cg_iters=K)
    u.copy_(c64(cs["u"]).reshape(n, 1, h, w))
    assert e.coils == coils
    mu = torch.full((n,), mu_v, device=DEV)
    sig = torch.tensor([30.0 / 255.0, 12.0 / 255.0], device=DEV)
    z0n, un = _np(z)[:, 0], _np(u)[:, 0]
    vin = (z.real - u.real)[:, 0].cpu().numpy()                                     # float32, as the kernel forms it
    lam = sig.cpu().numpy()
    e.step(x, z, u, mu, sig)
    xr = R.haar(vin, lam, R.LEVELS, R.MODE)
    x_f32 = float(np.abs(R.haar(vin, lam, R.LEVELS, R.MODE, f32=True) - xr).max())
    zr, ur, _ = SR.prox_dual(xr, z0n, un, cs["y"], cs["sens"], cs["mask"], np.full(n, float(np.float32(mu_v))), K, cs["aty"])
    ex = float(np.abs(_np(x)[:, 0] - xr).max())
    emax, erms = SR.solve_errors(_np(z)[:, 0], zr)
    umax = float(np.abs(_np(u)[:, 0] - ur).max() / np.abs(zr).max())
    bmax, brms = (MARGIN * v for v in SENSE_F32)
    print(f"multi-coil Haar step: x {ex:.3e} / {MARGIN * x_f32:.2e}; z err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}; "
          f"cg_res {e.cg_residual().cpu().numpy()}")
    record_property("x_err", ex); record_property("err_max", emax); record_property("err_rms", erms); record_property("u_max", umax)
    assert ex <= MARGIN * x_f32
    assert emax <= bmax and erms <= brms and umax <= 2 * bmax


def test_cli_prior_haar_fixed_runs():
    from dt4image_restoration_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = cli.main(["--block_size", "6", "--n_embeds", "9", "--size", "64", "--limit", "2", "--prior", "haar", "--haar-levels", "2", "--seed", "3",
                        "fixed", "--max_iter", "2"])
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
    assert lines and [l["psnr"] for l in lines] == [o["psnr"] for o in out] and all(np.isfinite(l["psnr"]) for l in lines)


# ---- prior switching -------------------------------------------------------------------------------------------------------------------

def test_a_unet_handle_that_visited_the_haar_prior_steps_bit_for_bit_like_a_fresh_one():
    n, h, w = 2, 32, 32
    x0, y0, mask, _ = _problem(n, h, w, seed=5)
    sd = weights.generate_unet_weights(0, "unit_gain")
    mu, sig = torch.tensor([0.1, 0.4], device=DEV), torch.tensor([0.15, 0.05], device=DEV)
    out = []
    for visit in (True, False):
        e = _engine(n, h, w, denoiser=True)
        e.load_weights(sd)
        assert e.prior_settings() == ("unet", 1.0, 20) and e.haar_settings() == (1.0, 3, "ti")
        x, z, u = e.reset(x0, y0, mask)
        e.step(x, z, u, mu, sig)
        if visit:
            e.set_haar_prior(0.5, 2, "ortho")
            xs, zs, us = x.clone(), z.clone(), u.clone()
            e.step(xs, zs, us, mu, sig)
            e.haar_denoise(xs, sig, 4)
            e.set_prior("unet")
            assert e.prior_settings() == ("unet", 1.0, 20) and e.haar_settings() == (0.5, 2, "ortho")
        e.step(x, z, u, mu, sig)
        out.append((x, z, u))
    for a, b in zip(*out):
        assert _same(a, b)


def test_tv_to_haar_to_tv_and_back_to_the_unet_steps_bit_for_bit_like_handles_that_never_visited():
    n, h, w = 2, 32, 32
    x0, y0, mask, _ = _problem(n, h, w, seed=5)
    sd = weights.generate_unet_weights(0, "unit_gain")
    mu, sig = torch.tensor([0.1, 0.4], device=DEV), torch.tensor([0.15, 0.05], device=DEV)
    tv_out, unet_out = [], []
    for visit in (True, False):
        e = _engine(n, h, w, denoiser=True)
        e.load_weights(sd)
        e.set_prior("tv", 0.6, 9)
        x, z, u = e.reset(x0, y0, mask)
        e.step(x, z, u, mu, sig)
        if visit:
            e.set_haar_prior(2.0, 4, "ti")
            assert e.prior == "haar" and e.prior_settings() == ("haar", 0.6, 9)       # the TV pair is untouched
            xs, zs, us = x.clone(), z.clone(), u.clone()
            e.step(xs, zs, us, mu, sig)
            assert not _same(xs, x)
            e.set_prior("tv", 0.6, 9)
        assert e.prior_settings() == ("tv", 0.6, 9)
        e.step(x, z, u, mu, sig)
        tv_out.append((x.clone(), z.clone(), u.clone()))
        e.set_prior("unet")
        e.step(x, z, u, mu, sig)
        unet_out.append((x, z, u))
    for pair in (tv_out, unet_out):
        for a, b in zip(*pair):
            assert _same(a, b)


def test_a_kspace_only_handle_steps_once_the_haar_prior_is_set_and_a_refused_setter_changes_nothing():
    n, h, w = 1, 32, 32
    x0, y0, mask, _ = _problem(n, h, w, seed=6)
    e = _engine(n, h, w)
    x, z, u = e.reset(x0, y0, mask)
    keep = [t.clone() for t in (x, z, u)]
    mu, sig = torch.tensor([0.3], device=DEV), torch.tensor([0.1], device=DEV)
    args = (e._h, mu.data_ptr(), sig.data_ptr(), None, x.data_ptr(), z.data_ptr(), u.data_ptr(), None, None, None)
    assert e.lib.pnp_step(*args) == -3                                              # PNP_ERR_STATE
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip((x, z, u), keep))
    assert e.haar_settings() == (1.0, 3, "ti") and e.prior == "unet"               # the fresh-handle defaults
    e.set_haar_prior(1.5, 2, "ortho")
    assert e.haar_settings() == (1.5, 2, "ortho") and e.prior == "haar"
    assert e.lib.pnp_step(*args) == 0, e.lib.pnp_last_error()
    assert not _same(x, keep[0])
    for bad, what in (((-1.0, 3, 0), b"haar_scale"), ((float("nan"), 3, 0), b"haar_scale"), ((float("inf"), 3, 0), b"haar_scale"),
                      ((1.0, 0, 0), b"levels"), ((1.0, 5, 0), b"levels"), ((1.0, 3, 2), b"mode"), ((1.0, 3, -1), b"mode")):
        assert e.lib.pnp_set_prior_haar(e._h, *bad) == -1 and what in e.lib.pnp_last_error(), bad
    assert e.lib.pnp_set_prior(e._h, _lib.PNP_PRIOR_HAAR, 1.0, 20) == -1 and b"prior must be" in e.lib.pnp_last_error()
    assert e.haar_settings() == (1.5, 2, "ortho") and e.prior == "haar"
    assert e.lib.pnp_set_prior(e._h, _lib.PNP_PRIOR_UNET, 1.0, 20) == -3            # still a k-space-only handle
    assert e.prior == "haar"
    with pytest.raises(ValueError, match="mode"):
        e.set_haar_prior(mode="db4")


# ---- memory ----------------------------------------------------------------------------------------------------------------------------

def test_the_shipped_forms_need_no_workspace_and_the_naive_form_grows_it_on_its_first_ti_call_only(monkeypatch):
    n, h, w = 2, 64, 80
    v, lam = torch.rand((n, 1, h, w), device=DEV), torch.tensor([0.1, 0.2], device=DEV)
    x0, y0, mask, _ = _problem(n, h, w)
    e = _engine(n, h, w)
    ws0 = e.workspace_bytes
    for mode in R.MODES:
        e.haar_denoise(v, lam, 4, mode)
        e.haar_denoise(v.clone(), lam, 3, mode, out=None)
        buf = v.clone()
        e.haar_denoise(buf, lam, 2, mode, out=buf)
    x, z, u = e.reset(x0, y0, mask)
    ws1 = e.workspace_bytes
    e.set_haar_prior()
    e.step(x, z, u, lam, lam)
    assert e.workspace_bytes == ws1 and ws1 >= ws0
    e2 = _engine(n, h, w)
    e2.haar_denoise(v, lam, 4)
    assert e2.workspace_bytes == ws0
    nv = _naive_engine(monkeypatch, n, h, w)
    assert nv.workspace_bytes == ws0                                               # its planes are allocated only when it runs
    nv.haar_denoise(v, lam, 3, "ortho")
    assert nv.workspace_bytes == ws0
    nv.haar_denoise(v, lam, 1)                                                     # a single level allocates all planes as well
    assert nv.workspace_bytes - ws0 == 4 * NAIVE_PLANES * n * h * w
    nv.haar_denoise(v, lam, 4)
    nv.haar_denoise(buf, lam, 4, out=buf)
    assert nv.workspace_bytes - ws0 == 4 * NAIVE_PLANES * n * h * w
    nv = _naive_engine(monkeypatch, n, h, w)                                       # the first use may be a step
    x, z, u = nv.reset(x0, y0, mask)
    nv.set_haar_prior()
    ws1 = nv.workspace_bytes
    nv.step(x, z, u, lam, lam)
    assert nv.workspace_bytes - ws1 == 4 * NAIVE_PLANES * n * h * w
    nv.step(x, z, u, lam, lam)
    assert nv.workspace_bytes - ws1 == 4 * NAIVE_PLANES * n * h * w


@pytest.mark.parametrize("naive", [False, True], ids=["fused", "naive"])
@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 16, 16), (1, 208, 144), (1, 112, 128)], ids=["2x64x80", "1x16x16", "1x208x144", "1x112x128"])
def test_guard_bands_around_every_caller_buffer_of_haar_denoise(shape, naive, monkeypatch):
    n, h, w = shape
    e = _naive_engine(monkeypatch, n, h, w) if naive else _engine(n, h, w)
    g = torch.Generator().manual_seed(5)
    x_in = GB.guarded((n, 1, h, w), F32T, DEV, fill=torch.rand((n, 1, h, w), generator=g), name="x_in")
    lam = GB.guarded((n,), F32T, DEV, fill=torch.tensor([0.2, 0.05][:n]), name="lam")
    out = GB.guarded((n, 1, h, w), F32T, DEV, name="out")
    for levels, mode in ((1, _lib.PNP_HAAR_TI), (4, _lib.PNP_HAAR_TI), (4, _lib.PNP_HAAR_ORTHO)):
        with GB.watch(outputs={"out": out}, inputs={"x_in": x_in, "lam": lam}):
            rc = e.lib.pnp_haar_denoise(e._h, x_in.data_ptr(), lam.data_ptr(), levels, mode, out.data_ptr(), None)
            assert rc == 0, e.lib.pnp_last_error()
        assert bool(torch.isfinite(out).all())
        both = GB.guarded((n, 1, h, w), F32T, DEV, fill=x_in, name="in-place")
        with GB.watch(outputs={"in-place": both}, inputs={"lam": lam}):
            assert e.lib.pnp_haar_denoise(e._h, both.data_ptr(), lam.data_ptr(), levels, mode, both.data_ptr(), None) == 0
        assert _same(both, out)


@pytest.mark.parametrize("naive", [False, True], ids=["fused", "naive"])
@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 16, 16)], ids=["2x64x80", "1x16x16"])
def test_guard_bands_around_every_caller_buffer_of_a_haar_step(shape, naive, monkeypatch):
    n, h, w = shape
    e = _naive_engine(monkeypatch, n, h, w) if naive else _engine(n, h, w)
    x0, y0, mask, _ = _problem(n, h, w)
    xr, zr, ur = e.reset(x0, y0, mask)
    e.set_haar_prior(1.0, 4, "ti")
    x = GB.guarded((n, 1, h, w), F32T, DEV, fill=xr, name="x")
    z = GB.guarded((n, 1, h, w), C64, DEV, fill=zr, name="z")
    u = GB.guarded((n, 1, h, w), C64, DEV, fill=ur, name="u")
    mu = GB.guarded((n,), F32T, DEV, fill=torch.tensor([0.3, 0.1][:n]), name="mu")
    sig = GB.guarded((n,), F32T, DEV, fill=torch.tensor([0.1, 0.05][:n]), name="sigma_d")
    act = GB.guarded((n,), F32T, DEV, fill=torch.zeros(n), name="t_action")
    t_state = GB.guarded((n,), F32T, DEV, fill=torch.zeros(n), name="t_state")
    done = GB.guarded((n,), U8, DEV, fill=torch.zeros(n, dtype=U8), name="done")
    for stop in (False, True):
        if stop:
            act[0] = 1.0
        with GB.watch(outputs={"x": x, "z": z, "u": u, "t_state": t_state, "done": done}, inputs={"mu": mu, "sigma_d": sig, "t_action": act}):
            rc = e.lib.pnp_step(e._h, mu.data_ptr(), sig.data_ptr(), act.data_ptr(), x.data_ptr(), z.data_ptr(), u.data_ptr(), t_state.data_ptr(),
                                done.data_ptr(), None)
            assert rc == 0, e.lib.pnp_last_error()
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(torch.view_as_real(z)).all())


def test_every_argument_error_is_invalid_and_leaves_the_outputs_untouched():
    n, h, w = 1, 32, 48
    e = _engine(n, h, w)
    v, lam = torch.rand((n, 1, h, w), device=DEV), torch.tensor([0.1], device=DEV)
    out = torch.full((n, 1, h, w), 7.0, device=DEV)
    ws0 = e.workspace_bytes
    vp, lp, op = v.data_ptr(), lam.data_ptr(), out.data_ptr()
    bad = [((None, vp, lp, 3, 0, op), b"null handle"), ((e._h, None, lp, 3, 0, op), b"null x_in"), ((e._h, vp, None, 3, 0, op), b"null lam"),
           ((e._h, vp, lp, 3, 0, None), b"null out"), ((e._h, vp, lp, 0, 0, op), b"levels"), ((e._h, vp, lp, 5, 0, op), b"levels"),
           ((e._h, vp, lp, 3, 2, op), b"mode"), ((e._h, vp, lp, 3, -1, op), b"mode")]
    for args, what in bad:
        assert e.lib.pnp_haar_denoise(*args, None) == -1 and what in e.lib.pnp_last_error(), (args, e.lib.pnp_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and e.workspace_bytes == ws0                    # nothing ran, nothing was allocated
    with pytest.raises(ValueError, match="levels"):
        e.haar_denoise(v, lam, 5)
    with pytest.raises(ValueError, match="mode"):
        e.haar_denoise(v, lam, 3, "db4")
    assert e.lib.pnp_haar_denoise(e._h, vp, lp, 4, 1, op, None) == 0
