"""The total-variation prior (pnp_tv_denoise, pnp_set_prior / pnp_get_prior, pnp_step under PNP_PRIOR_TV) on the MI355X, through the C ABI
(PnPEngine is the ctypes binding), against the float64 restatement of tests/tv_ref.py computed from the float32 input the device is handed.
Every figure is printed and attached with record_property before it is asserted.

CASES (tv_ref.CASES; phantoms plus seeded noise of sigma 0.04, slice 0 of every case stretched to [-0.15, 1.15]; weights per slice):

      N  H    W    lam per slice      covers
      2  16   16   0.2, 0             an image smaller than any halo
      3  80   64   0.05, 1e-6, 10     a 2^a 5^b side, non-square
      1  16   272  0.2                ragged tiles, a one-tile-thin image
      1  272  16   0.05               the same the other way
      2  128  128  10, 0.05           several tiles both ways
      1  208  144  0.2                sides that are no k-space size

iters in {1, 7, 10, 11, 20, 64}: below, at and above the fused kernel's depth of 10 iterations per launch, so the hand-over between launches
runs with one, two and seven launches.

BOUNDS.  max |out - ref| is within TEN TIMES the error of the float32 restatement (tv_ref.tv(f32=True), the header's expression order) against
the float64 one, measured on the CPU by tests/test_tv_host.py (tv_ref.F32_ERR), per case and iteration count:

      case   K = 1       7           10          11          20          64
      0      3.943e-08   5.146e-08   7.026e-08   6.450e-08   7.101e-08   1.031e-07
      1      5.511e-08   6.849e-08   8.086e-08   7.966e-08   1.120e-07   1.551e-07
      2      5.631e-08   9.262e-08   9.971e-08   9.125e-08   8.961e-08   1.202e-07
      3      4.403e-08   6.773e-08   7.845e-08   7.105e-08   7.724e-08   9.344e-08
      4      6.156e-08   1.004e-07   9.170e-08   1.163e-07   1.524e-07   2.224e-07
      5      5.245e-08   8.541e-08   9.329e-08   8.825e-08   9.405e-08   1.183e-07

TV-ADMM (tv_ref.FIXTURE: 1 x 64 x 80, 4x, sigma 5/255, seed 1234, mu 0.3, sigma_d 50/255 -> 5/255 geometric over 30 iterations, tv_scale 1,
tv_iters 20) through FixedScheduleSolver with TVDenoiser2D: the first 10 iterations against the float64 loop within ten times the float32
restatement's |dPSNR| = 3.374e-07 dB and max |dx| = 2.041e-07 (tv_ref.ADMM_F32); the 30 iterations end at least 3 dB above x0 (the
reference: 28.256 -> 35.884 dB).

Multi-coil step (2 x 64 x 64, 4 coils, sense_ref.solve_case, mu 0.3, K = 8, tv_iters 20): x against tv_ref within ten times the float32
restatement's error on that input (measured in the test, on the CPU), z against sense_ref.prox_dual fed the reference's x under
test_gpu_sense.py's bound for (0.3, 8): ten times (1.040e-06, 3.780e-07).

Everything else is bit for bit.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as GB  # noqa: E402
import sense_ref as SR  # noqa: E402
import tv_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic, weights  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0
SENSE_F32 = (1.040e-06, 3.780e-07)                         # test_gpu_sense.py, F32[(0.3, 8)]: err_max, err_rms
DEV = "cuda"
C64, F32T, U8 = torch.complex64, torch.float32, torch.uint8


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def _naive_engine(monkeypatch, n, h, w):
    monkeypatch.setenv("PNP_TV_NAIVE", "1")                # read at pnp_create
    e = _engine(n, h, w)
    monkeypatch.delenv("PNP_TV_NAIVE")
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


@pytest.mark.parametrize("iters", R.CASE_ITERS)
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_tv_denoise_against_float64(i, iters, record_property):
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    out = _engine(n, h, w).tv_denoise(v, lam, iters)
    assert out.shape == (n, 1, h, w) and out.dtype == F32T
    err = float(np.abs(_np(out)[:, 0] - R.case_ref(i, iters)).max())
    bound = MARGIN * R.F32_ERR[i][R.CASE_ITERS.index(iters)]
    print(f"case {i} {n}x{h}x{w} lam {lam.tolist()} iters {iters}: max |out - ref| {err:.3e} / {bound:.2e}")
    record_property("max_abs_err", err); record_property("bound", bound)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert err <= bound


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_fused_and_naive_give_the_same_bits(i, monkeypatch):
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    fused, naive = _engine(n, h, w), _naive_engine(monkeypatch, n, h, w)
    for iters in R.CASE_ITERS:
        a, b = fused.tv_denoise(v, lam, iters), naive.tv_denoise(v, lam, iters)
        assert _same(a, b), iters
    for e in (fused, naive):                                                       # out aliasing x_in == not aliasing, in both forms
        for iters in (1, R.FUSE_T, 20):
            want = e.tv_denoise(v, lam, iters)
            buf = v.clone()
            assert e.tv_denoise(buf, lam, iters, out=buf) is buf
            assert _same(buf, want), iters


def test_a_slice_gives_the_same_bits_alone_at_every_place_of_a_batch_on_a_side_stream_twice_and_on_every_handle_kind():
    i = 1
    n, h, w = R.CASES[i]
    v, lam = _case(i)
    e3 = _engine(n, h, w)
    for iters in (7, 20):
        base = e3.tv_denoise(v, lam, iters)
        assert _same(e3.tv_denoise(v, lam, iters), base)                           # two calls in a row
        assert not _same(base[0], base[1]) and not _same(base[1], base[2])
        e1 = _engine(1, h, w)
        for j in range(n):                                                         # alone
            assert _same(e1.tv_denoise(v[j:j + 1].clone(), lam[j:j + 1].clone(), iters)[0], base[j]), j
        for shift in (1, 2):                                                       # at the two other places
            perm = [(j + shift) % n for j in range(n)]
            got = e3.tv_denoise(v[perm].contiguous(), lam[perm].contiguous(), iters)
            for k, j in enumerate(perm):
                assert _same(got[k], base[j]), (shift, k)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got = e3.tv_denoise(v, lam, iters)
        side.synchronize()
        assert _same(got, base)
        unet, bf16 = _engine(n, h, w, denoiser=True), _engine(n, h, w, denoiser=True, bf16_convs=True)   # no weights are needed
        assert _same(unet.tv_denoise(v, lam, iters), base) and _same(bf16.tv_denoise(v, lam, iters), base)
        mc = _engine(n, h, w)                                                      # a handle in multi-coil mode
        sens = c64(synthetic.coil_maps(2, h, w))
        mc.set_kspace(torch.zeros((n, 2, h, w), dtype=C64, device=DEV), torch.ones((h, w), dtype=U8, device=DEV), sens=sens, cg_iters=2)
        assert _same(mc.tv_denoise(v, lam, iters), base) and mc.coils == 2


@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 128, 224), (1, 208, 144)])
def test_a_constant_image_returns_itself_and_lam_zero_is_the_clamp(shape):
    n, h, w = shape
    e = _engine(n, h, w)
    lam = torch.tensor([0.2, 1e-6][:n], device=DEV)
    for c in (0.0, 0.3, 1.0):
        v = torch.full((n, 1, h, w), c, dtype=F32T, device=DEV)
        for iters in (1, 11, 64):
            assert _same(e.tv_denoise(v, lam, iters), v), (c, iters)
    assert _same(e.tv_denoise(torch.full((n, 1, h, w), 1.5, device=DEV), lam, 20), torch.ones((n, 1, h, w), device=DEV))
    g = torch.Generator().manual_seed(3)
    v = (torch.randn((n, 1, h, w), generator=g) * 0.8 + 0.5).to(DEV)
    for iters in (1, 20):
        assert _same(e.tv_denoise(v, torch.zeros(n, device=DEV), iters), torch.clamp(v, 0, 1))


# ---- pnp_step under the TV prior -------------------------------------------------------------------------------------------------------

def _problem(n, h, w, seed=9):
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=seed)
    return (c64(R.cplx(d["x0"])), c64(R.cplx(d["y0"])), torch.from_numpy(d["mask"]).to(DEV), d)


def test_a_tv_step_is_tv_denoise_on_re_z_minus_u_then_prox_dual_bit_for_bit_and_stopped_slices_keep_their_bits(monkeypatch):
    n, h, w = 2, 64, 80
    x0, y0, mask, _ = _problem(n, h, w)
    mu = torch.tensor([0.1, 0.4], device=DEV)
    sig = torch.tensor([40.0 / 255.0, 15.0 / 255.0], device=DEV)
    scale, iters = 0.7, 13
    for e in (_engine(n, h, w), _naive_engine(monkeypatch, n, h, w)):
        e.set_prior("tv", scale, iters)
        assert e.prior_settings() == ("tv", 0.7, 13) and e.prior == "tv"
        x, z, u = e.reset(x0, y0, mask)
        xm, zm, um = x.clone(), z.clone(), u.clone()
        t_state, done = torch.zeros(n, device=DEV), torch.full((n,), 7, dtype=U8, device=DEV)
        lam = (torch.tensor(scale, dtype=F32T, device=DEV) * sig).contiguous()
        for _ in range(3):                                                         # (u is zero in the first step only)
            e.step(x, z, u, mu, sig, t_state=t_state, done=done)
            xm = e.tv_denoise((zm.real - um.real).contiguous(), lam, iters)
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
        xm = e.tv_denoise((zm.real - um.real).contiguous(), lam, iters)
        e.prox_dual(xm, zm, um, mu)
        assert _same(x[1], xm[1]) and _same(z[1], zm[1]) and _same(u[1], um[1])


def _mat(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def test_tv_admm_through_the_fixed_schedule_solver_against_the_float64_loop(record_property):
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    t = R.FIXTURE
    d = R.fixture_problem()
    den = TVDenoiser2D(scale=t["tv_scale"], iters=t["tv_iters"])
    k = t["compare_iters"]
    mu, sig = R.fixture_schedules(k)
    x64, p0, p64 = R.admm_tv(d, mu, sig)
    env = PnPEnv(max_episode_step=k, denoiser=den, device_type="cuda")
    r = FixedScheduleSolver(env, max_iter=k).run(_mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    dx = float(np.abs(_np(r.x)[:, 0] - x64).max())
    gt = d["gt"][:, 0].astype(np.float64)
    dp = float(np.abs(R.psnr(_np(r.x)[:, 0], gt) - p64).max())                      # both in float64 from the iterate, as the restatement's figure
    bp, bx = (MARGIN * v for v in R.ADMM_F32)
    print(f"{k} TV-ADMM iterations: PSNR {r.psnr.reshape(-1).tolist()} ref {p64}  |dPSNR| {dp:.3e} / {bp:.2e} dB  max |dx| {dx:.3e} / {bx:.2e}")
    record_property("dpsnr", dp); record_property("max_abs_dx", dx)
    assert env._engine.prior == "tv" and not env._engine.coils
    assert dx <= bx and dp <= bp
    assert abs(float(r.psnr.reshape(-1)[0]) - float(p64[0])) <= 1e-4               # what the engine itself reports (float32)
    mu, sig = R.fixture_schedules()
    env = PnPEnv(max_episode_step=t["iters"], denoiser=den, device_type="cuda")
    r = FixedScheduleSolver(env, max_iter=t["iters"]).run(_mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    gain = float((r.psnr - r.initial_psnr).min())
    print(f"{t['iters']} iterations: PSNR of x0 {r.initial_psnr.reshape(-1).tolist()}, final {r.psnr.reshape(-1).tolist()} (reference {p0} -> 35.884)")
    record_property("psnr_gain", gain)
    assert gain >= 3.0
    out = den(r.x, torch.full((t["n"],), 0.1, device=DEV))                          # the reference's denoiser(x, sigma) call shape
    assert out.shape == r.x.shape and _same(out, env._engine.tv_denoise(r.x, torch.full((t["n"],), 0.1, device=DEV), t["tv_iters"]))


def test_one_multi_coil_tv_step_against_tv_ref_and_sense_ref(record_property):
    n, h, w, coils, K, mu_v, iters = 2, 64, 64, 4, 8, 0.3, 20
    cs = SR.solve_case(h, w, coils, False, "radial", 4)
    e = _engine(n, h, w)
    e.set_prior("tv", 1.0, iters)
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
    xr = R.tv(vin, lam, iters)
    x_f32 = float(np.abs(R.tv(vin, lam, iters, f32=True) - xr).max())
    zr, ur, _ = SR.prox_dual(xr, z0n, un, cs["y"], cs["sens"], cs["mask"], np.full(n, float(np.float32(mu_v))), K, cs["aty"])
    ex = float(np.abs(_np(x)[:, 0] - xr).max())
    emax, erms = SR.solve_errors(_np(z)[:, 0], zr)
    umax = float(np.abs(_np(u)[:, 0] - ur).max() / np.abs(zr).max())
    bmax, brms = (MARGIN * v for v in SENSE_F32)
    print(f"multi-coil TV step: x {ex:.3e} / {MARGIN * x_f32:.2e}; z err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}; "
          f"cg_res {e.cg_residual().cpu().numpy()}")
    record_property("x_err", ex); record_property("err_max", emax); record_property("err_rms", erms); record_property("u_max", umax)
    assert ex <= MARGIN * x_f32
    assert emax <= bmax and erms <= brms and umax <= 2 * bmax


# ---- prior switching -------------------------------------------------------------------------------------------------------------------

def test_a_unet_handle_that_visited_the_tv_prior_steps_bit_for_bit_like_a_fresh_one():
    n, h, w = 2, 32, 32
    x0, y0, mask, _ = _problem(n, h, w, seed=5)
    sd = weights.generate_unet_weights(0, "unit_gain")
    mu, sig = torch.tensor([0.1, 0.4], device=DEV), torch.tensor([0.15, 0.05], device=DEV)
    out = []
    for visit in (True, False):
        e = _engine(n, h, w, denoiser=True)
        e.load_weights(sd)
        assert e.prior_settings() == ("unet", 1.0, 20)
        x, z, u = e.reset(x0, y0, mask)
        e.step(x, z, u, mu, sig)
        if visit:
            e.set_prior("tv", 0.5, 12)
            xs, zs, us = x.clone(), z.clone(), u.clone()
            e.step(xs, zs, us, mu, sig)
            e.tv_denoise(xs, sig, 25)
            e.set_prior("unet")
            assert e.prior_settings() == ("unet", 0.5, 12)
        e.step(x, z, u, mu, sig)
        out.append((x, z, u))
    for a, b in zip(*out):
        assert _same(a, b)


def test_a_kspace_only_handle_cannot_step_until_the_tv_prior_is_set_and_refuses_the_unet_prior():
    n, h, w = 1, 32, 32
    x0, y0, mask, _ = _problem(n, h, w, seed=6)
    e = _engine(n, h, w)
    x, z, u = e.reset(x0, y0, mask)
    keep = [t.clone() for t in (x, z, u)]
    mu, sig = torch.tensor([0.3], device=DEV), torch.tensor([0.1], device=DEV)
    args = (e._h, mu.data_ptr(), sig.data_ptr(), None, x.data_ptr(), z.data_ptr(), u.data_ptr(), None, None, None)
    assert e.lib.pnp_step(*args) == -3                                              # PNP_ERR_STATE
    assert e.lib.pnp_set_prior(e._h, _lib.PNP_PRIOR_UNET, 1.0, 20) == -3 and b"PNP_FLAG_NO_DENOISER" in e.lib.pnp_last_error()
    assert e.lib.pnp_step(*args) == -3
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip((x, z, u), keep))
    e.set_prior("tv")
    assert e.prior_settings() == ("tv", 1.0, 20)
    assert e.lib.pnp_step(*args) == 0, e.lib.pnp_last_error()
    assert not _same(x, keep[0])
    for bad in ((2, 1.0, 20), (1, -1.0, 20), (1, float("nan"), 20), (1, 1.0, 0), (1, 1.0, 65)):     # a refused setter changes nothing
        assert e.lib.pnp_set_prior(e._h, *bad) == -1
    assert e.prior_settings() == ("tv", 1.0, 20)
    with pytest.raises(ValueError, match="prior"):
        e.set_prior("wavelet")


# ---- memory ----------------------------------------------------------------------------------------------------------------------------

def test_workspace_grows_by_the_documented_bytes_on_the_first_call_only():
    n, h, w = 2, 64, 80
    v, lam = torch.rand((n, 1, h, w), device=DEV), torch.tensor([0.1, 0.2], device=DEV)
    e = _engine(n, h, w)
    ws0 = e.workspace_bytes
    e.tv_denoise(v, lam, 1)                                                        # a single launch allocates the plane as well
    assert e.workspace_bytes - ws0 == 8 * n * h * w
    e.tv_denoise(v, lam, 64)
    e.tv_denoise(v, lam, 20, out=v)
    assert e.workspace_bytes - ws0 == 8 * n * h * w
    e = _engine(n, h, w)                                                           # the first use may be a step
    x0, y0, mask, _ = _problem(n, h, w)
    x, z, u = e.reset(x0, y0, mask)
    e.set_prior("tv")
    ws0 = e.workspace_bytes
    e.step(x, z, u, lam, lam)
    assert e.workspace_bytes - ws0 == 8 * n * h * w
    e.step(x, z, u, lam, lam)
    e.tv_denoise(v, lam, 20)
    assert e.workspace_bytes - ws0 == 8 * n * h * w


@pytest.mark.parametrize("naive", [False, True], ids=["fused", "naive"])
@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 16, 16), (1, 208, 144), (1, 16, 272)], ids=["2x64x80", "1x16x16", "1x208x144", "1x16x272"])
def test_guard_bands_around_every_caller_buffer_of_tv_denoise(shape, naive, monkeypatch):
    n, h, w = shape
    e = _naive_engine(monkeypatch, n, h, w) if naive else _engine(n, h, w)
    g = torch.Generator().manual_seed(5)
    x_in = GB.guarded((n, 1, h, w), F32T, DEV, fill=torch.rand((n, 1, h, w), generator=g), name="x_in")
    lam = GB.guarded((n,), F32T, DEV, fill=torch.tensor([0.2, 0.05][:n]), name="lam")
    out = GB.guarded((n, 1, h, w), F32T, DEV, name="out")
    for iters in (1, 11, 20):
        with GB.watch(outputs={"out": out}, inputs={"x_in": x_in, "lam": lam}):
            rc = e.lib.pnp_tv_denoise(e._h, x_in.data_ptr(), lam.data_ptr(), iters, out.data_ptr(), None)
            assert rc == 0, e.lib.pnp_last_error()
        assert bool(torch.isfinite(out).all())
        both = GB.guarded((n, 1, h, w), F32T, DEV, fill=x_in, name="in-place")
        with GB.watch(outputs={"in-place": both}, inputs={"lam": lam}):
            assert e.lib.pnp_tv_denoise(e._h, both.data_ptr(), lam.data_ptr(), iters, both.data_ptr(), None) == 0
        assert _same(both, out)


@pytest.mark.parametrize("naive", [False, True], ids=["fused", "naive"])
@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 16, 16)], ids=["2x64x80", "1x16x16"])
def test_guard_bands_around_every_caller_buffer_of_a_tv_step(shape, naive, monkeypatch):
    n, h, w = shape
    e = _naive_engine(monkeypatch, n, h, w) if naive else _engine(n, h, w)
    x0, y0, mask, _ = _problem(n, h, w)
    xr, zr, ur = e.reset(x0, y0, mask)
    e.set_prior("tv", 1.0, 13)
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
    bad = [((None, v.data_ptr(), lam.data_ptr(), 20, out.data_ptr()), b"null handle"), ((e._h, None, lam.data_ptr(), 20, out.data_ptr()), b"null x_in"),
           ((e._h, v.data_ptr(), None, 20, out.data_ptr()), b"null lam"), ((e._h, v.data_ptr(), lam.data_ptr(), 20, None), b"null out"),
           ((e._h, v.data_ptr(), lam.data_ptr(), 0, out.data_ptr()), b"iters"), ((e._h, v.data_ptr(), lam.data_ptr(), 65, out.data_ptr()), b"iters")]
    for args, what in bad:
        assert e.lib.pnp_tv_denoise(*args, None) == -1 and what in e.lib.pnp_last_error(), (args, e.lib.pnp_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and e.workspace_bytes == ws0                    # nothing ran, nothing was allocated
    with pytest.raises(ValueError, match="iters"):
        e.tv_denoise(v, lam, 65)
    assert e.lib.pnp_tv_denoise(e._h, v.data_ptr(), lam.data_ptr(), 64, out.data_ptr(), None) == 0
