"""Non-Cartesian sampling on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against the float64 restatement of
tests/nufft_ref.py: the model built from the plan's float32-rounded weights and factors, evaluated in float64.  Every buffer handed to the
new entry points comes from tests/guard_bands.py.  Every figure is printed before it is asserted.  No bound here is measured on the device.

BOUNDS (u = 2^-24, gamma_n = n u / (1 - n u)).
  Grid transform.  The suite asserts max |err| <= 3e-6 for pnp_fft2c on data whose complex elements have rms sqrt(2/3) (hash_uniform
  components; tests/test_gpu_kernels.py, tests/test_gpu_kspace_radix5.py), at every grid size used here; relative to the grid's norm that
  is E(X) = 3e-6 / sqrt(2/3) * ||X|| / sqrt(gh gw) per grid point.
  Forward, per sample m:  sum |wy wx| * E(X) + gamma_{2 J^2} sum |wy wx| |X|   (the transform's error gathered through the footprint,
  plus the rounding of the J^2-term double fma chain in the form of the GRAPPA apply bound: each term passes at most 2 J roundings).
  Adjoint, per pixel q:  |cy cx| * ( E(G) + gamma_{2 k} sum_g S[g] / sqrt(gh gw) ),  G = the float64 spread grid, S = the spread of
  |v| |wy| |wx| and k the case's largest chain length (taken from the plan; a term passes three roundings before its fma and at most k
  after, k + 3 <= 2 k); an error dG on the grid reaches a pixel of the orthonormal inverse transform with at most ||dG||_1 / sqrt(gh gw).
  Adjointness.  The float64 model is exactly adjoint, so <A x, y> - <x, A^H y> on the device outputs is <df, y> - <x, da>, at most
  ||Bf|| ||y|| + ||x|| ||Ba|| = (e_f + e_a) ||x|| ||y|| s with e_f = ||Bf|| / (s ||x||), e_a = ||Ba|| / (s ||y||), s = the model's norm.
  Stage.  The CG is the multi-coil text on another operator: the tolerances of tests/test_gpu_sense.py for mu = 0.3, K = 4 (ten times its
  float32 restatement: err_max 9.992e-07, err_rms 3.740e-07, d_res 2.784e-07), and its C = 1 cross-check bound 3e-6 + 10 x 9.44e-07 at
  mu = 0.3 (the float32 rounding), to which the model error of the host test is added: tests/test_nufft_host.py measures
  max |dz| / max |z| = 1.418e-07 for two float64 CG iterations on the Cartesian-bin trajectory against the closed form and asserts twice that.
  End to end (nufft_ref.FIXTURE: one 64 x 64 phantom, 24 golden-angle spokes of 128 samples, density-compensated, noise 5/255, mu 0.3,
  sigma_d 50/255 -> 5/255 geometric over 20 iterations, K = 8, TV with tv_scale 1, tv_iters 20) through FixedScheduleSolver: the float64
  restatement on the CPU goes from 16.572 dB (x0) to 36.812 dB, a gain of 20.24 dB (the condition on the input is >= 1 dB; checked by
  tests/test_nufft_host.py); the device's PSNR is asserted within 0.01 dB of the restatement's, the project's north-star bound.
  DC column: the bound of tests/test_gpu_residuals.py, |ddc| <= 1e-6 ||x|| + 5e-7 dc, with ||x|| scaled by the model's norm s.
  Acquisition: against the float64 exact NDFT, rms(err) / rms(ref) <= 1e-6 (tests/test_gpu_acquire.py) + twice the host test's model
  error of the case (J = 6 on 64 -> 80: 5.938e-04 relative, dominated by the kernel's aliasing, not by rounding)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as GB  # noqa: E402
import nufft_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
FFT_REL = 3e-6 / math.sqrt(2.0 / 3.0)
MARGIN = 10.0
F32_MU03_K4 = (9.992e-07, 3.740e-07, 2.784e-07)
C1K2_BOUND = 3e-6 + MARGIN * 9.44e-07
CLOSED_FORM_ERR = 1.418e-07                                # tests/test_nufft_host.py: the model's two CG iterations against the closed form
MODEL_J6_64 = 5.938e-04


def gamma(n):
    return n * U / (1.0 - n * U)


def _engine(n, h, w):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=False)


def g_c64(a, shape=None):
    a = np.ascontiguousarray(a)
    return GB.guarded(shape or a.shape, torch.complex64, DEV, fill=torch.from_numpy(a).to(torch.complex64))


def g_f32(a, shape=None):
    a = np.ascontiguousarray(a)
    return GB.guarded(shape or a.shape, torch.float32, DEV, fill=torch.from_numpy(a).to(torch.float32))


def _np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _rt(a):
    """a complex128 array rounded to complex64 and back: what the device is handed"""
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


_CASE = {}


def case(i):
    """(plan of the restatement, traj, image, samples) of CASES[i], computed once"""
    if i not in _CASE:
        n, h, w, gh, gw, J = R.CASES[i]
        traj = R.case_traj(i)
        P = R.plan(h, w, gh, gw, J, traj)
        _CASE[i] = (P, traj, _rt(R.case_image(i)), _rt(R.case_samples(i, P["m"])))
    return _CASE[i]


def planned(i, n=None):
    P, traj = case(i)[:2]
    e = _engine(n or R.CASES[i][0], P["h"], P["w"])
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=P["J"])
    return e


def raw_forward(e, img, out):
    with GB.watch(outputs={"samples": out}, inputs={"img": img}):
        _lib.check(e.lib.pnp_nufft_forward(e._h, img.data_ptr(), img.shape[0], out.data_ptr(), e._stream()), "pnp_nufft_forward")
    return out


def raw_adjoint(e, smp, wgt, out):
    with GB.watch(outputs={"img": out}, inputs={"samples": smp, "weights": wgt}):
        _lib.check(e.lib.pnp_nufft_adjoint(e._h, smp.data_ptr(), wgt.data_ptr() if wgt is not None else None, smp.shape[0], out.data_ptr(),
                                           e._stream()), "pnp_nufft_adjoint")
    return out


def forward_bound(P, x):
    X = R.grid_of(P, x)
    G = P["gh"] * P["gw"]
    e_fft = FFT_REL * np.sqrt((np.abs(X) ** 2).sum(axis=(1, 2))) / math.sqrt(G)              # [N]
    ones = np.ones((1, P["gh"], P["gw"]))
    return R.gather(P, ones, absolute=True) * e_fft[:, None] + gamma(2 * P["J"] ** 2) * R.gather(P, X, absolute=True)


def adjoint_bound(P, y, wgt=None):
    Gd = R.spread(P, y, wgt)
    S = R.spread(P, y, wgt, absolute=True)
    G = P["gh"] * P["gw"]
    k = int(R.chain_lengths(P).max())
    per = FFT_REL * np.sqrt((np.abs(Gd) ** 2).sum(axis=(1, 2))) / math.sqrt(G) + gamma(2 * k) * S.sum(axis=(1, 2)) / math.sqrt(G)
    f = np.abs(P["cy"][:, None].astype(np.float64) * P["cx"][None, :].astype(np.float64))
    return per[:, None, None] * f[None], k


# ---- forward, adjoint, adjointness ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_forward_and_adjoint_against_the_float64_model_and_adjointness(i):
    P, traj, x, y = case(i)
    n, h, w = R.CASES[i][:3]
    e = planned(i)
    assert e.nufft_samples == P["m"] and e.nufft_grid == (P["gh"], P["gw"])
    wgt = (0.25 + np.abs(R.case_samples(i, P["m"], seed=3)[0].real)).astype(np.float32)
    got_f = _np(raw_forward(e, g_c64(x), GB.guarded((n, P["m"]), torch.complex64, DEV)))
    ref_f, bf = R.forward(P, x), forward_bound(P, x)
    rf = float((np.abs(got_f - ref_f) / bf).max())
    print(f"case {i} {R.CASES[i]}: forward max |err| {np.abs(got_f - ref_f).max():.3e}, worst err / bound {rf:.3f}, rel l2 "
          f"{np.linalg.norm(got_f - ref_f) / np.linalg.norm(ref_f):.3e}")
    assert rf <= 1.0
    worst = 0.0
    for wv in (None, wgt):
        got_a = _np(raw_adjoint(e, g_c64(y), None if wv is None else g_f32(wv), GB.guarded((n, h, w), torch.complex64, DEV)))
        ref_a = R.adjoint(P, y, wv)
        ba, k = adjoint_bound(P, y, wv)
        ra = float((np.abs(got_a - ref_a) / ba).max())
        print(f"case {i}: adjoint ({'weights' if wv is not None else 'no weights'}) max |err| {np.abs(got_a - ref_a).max():.3e}, worst err / bound "
              f"{ra:.3f}, chain k = {k}, rel l2 {np.linalg.norm(got_a - ref_a) / np.linalg.norm(ref_a):.3e}")
        worst = max(worst, ra)
        if wv is None:
            got_a0, ba0 = got_a, ba
    assert worst <= 1.0
    s = R.op_norm(P)
    nx, ny = np.linalg.norm(x.reshape(n, -1), axis=1), np.linalg.norm(y, axis=1)
    lhs = np.array([np.vdot(y[j], got_f[j]) - np.vdot(got_a0[j], x[j]) for j in range(n)])          # <y, A x> - <A^H y, x>
    e_f = np.linalg.norm(bf, axis=1) / (s * nx)
    e_a = np.linalg.norm(ba0.reshape(n, -1), axis=1) / (s * ny)
    bound = (e_f + e_a) * nx * ny * s
    print(f"case {i}: adjointness |<Ax,y> - <x,A^H y>| {np.abs(lhs)} bound {bound} (e_f {e_f}, e_a {e_a}, s {s:.4f})")
    assert (np.abs(lhs) <= bound).all()


# ---- bits -------------------------------------------------------------------------------------------------------------------------------------

def _stage_inputs(i, seed=0):
    P, traj, x, y = case(i)
    n, h, w = R.CASES[i][:3]
    rng = np.random.default_rng(77 + seed)
    xr = rng.random((n, h, w)).astype(np.float32).astype(np.float64)
    z0 = _rt(xr + 0.05 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    u0 = _rt(0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    wgt = (0.5 + rng.random(P["m"])).astype(np.float32)
    ys = _rt(R.forward(P, xr.astype(np.complex128)) + 0.02 * R.case_samples(i, P["m"], seed=9))
    return xr, z0, u0, wgt, ys


def _iterate(xr, z0, u0):
    n, h, w = xr.shape
    return g_f32(xr, (n, 1, h, w)), g_c64(z0, (n, 1, h, w)), g_c64(u0, (n, 1, h, w))


def test_two_runs_and_a_slice_alone_give_the_same_bits():
    i = 4
    P, traj, x, y = case(i)
    n, h, w = R.CASES[i][:3]
    xr, z0, u0, wgt, ys = _stage_inputs(i)
    mu = np.array([0.3, 0.05, 0.6], dtype=np.float32)
    e = planned(i)

    def run(eng, sl):
        k = sl.stop - sl.start
        f = eng.nufft_forward(g_c64(x[sl]))
        a = eng.nufft_adjoint(g_c64(y[sl]), g_f32(wgt))
        eng.set_kspace_nc(g_c64(ys[sl]), g_f32(wgt), cg_iters=3)
        q = eng.nc_normal(g_c64(u0[sl], (k, 1, h, w)), g_f32(mu[sl]))
        xs, zs, us = _iterate(xr[sl], z0[sl], u0[sl])
        eng.set_prior("tv", tv_scale=1.0, tv_iters=5)
        eng.step(xs, zs, us, g_f32(mu[sl]), g_f32(np.full(k, 0.05, dtype=np.float32)))
        dc = eng.residuals(xs, zs, us, dc=True)
        return f, a, q, xs, zs, us, dc, eng.nc_cg_residual()

    full = run(e, slice(0, n))
    again = run(e, slice(0, n))
    for name, a, b in zip("forward adjoint normal x z u residuals cg_res".split(), full, again):
        assert _same(a, b), name
    e1 = planned(i, n=1)
    for j in range(n):
        alone = run(e1, slice(j, j + 1))
        for name, a, b in zip("forward adjoint normal x z u residuals cg_res".split(), full, alone):
            assert _same(a[j:j + 1], b), (name, j)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run(e, slice(0, n))
    side.synchronize()
    for name, a, b in zip("forward adjoint normal x z u residuals cg_res".split(), full, other):
        assert _same(a, b), name


def test_swapping_two_samples_with_disjoint_footprints_keeps_the_adjoint_bits():
    i = 4
    P, traj, x, y = case(i)
    n, h, w = R.CASES[i][:3]
    # two NEIGHBOURS in the sample order that share no tile (a fortiori no grid point): no grid point's chain holds both, and no sample
    # lies between them, so every grid point's ascending order is unchanged by their swap
    a = next(a for a in range(P["m"] - 1) if not (R.tiles_of(P, a) & R.tiles_of(P, a + 1)))
    b = a + 1
    perm = np.arange(P["m"])
    perm[[a, b]] = perm[[b, a]]
    e = planned(i)
    base = e.nufft_adjoint(g_c64(y))
    e.nufft_plan(traj[perm], grid=(P["gh"], P["gw"]), width=P["J"])
    swapped = e.nufft_adjoint(g_c64(y[:, perm]))
    print(f"swapped samples {a} and {b}: tiles {sorted(R.tiles_of(P, a))} and {sorted(R.tiles_of(P, b))}")
    assert _same(base, swapped)


# ---- the stage -----------------------------------------------------------------------------------------------------------------------------

def test_normal_operator_prox_dual_steps_and_residuals_against_float64():
    i = 4
    P, traj, x, y = case(i)
    n, h, w = R.CASES[i][:3]
    xr, z0, u0, wgt, ys = _stage_inputs(i)
    K, mu = 4, np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    e = planned(i)
    with pytest.raises(_lib.PnPError, match="non-Cartesian mode"):
        e.nc_cg_residual()
    e.set_kspace_nc(g_c64(ys), g_f32(wgt), cg_iters=K)
    assert e.coils == 0
    assert not e.nc_cg_residual().any()                                             # 0 before the first solve
    # the normal operator: both operator bounds chained, A^H W (A p): the forward's error bound spread by the adjoint model's absolute
    # weights (through adjoint_bound on |Bf|), plus the adjoint's own bound on the float64 samples, plus mu p's rounding
    p = u0
    q = _np(e.nc_normal(g_c64(p, (n, 1, h, w)), g_f32(mu)))[:, 0]
    qr = R.normal(P, p, mu64, wgt)
    bf = forward_bound(P, p)
    f = np.abs(P["cy"][:, None].astype(np.float64) * P["cx"][None, :].astype(np.float64))
    ba, k = adjoint_bound(P, R.forward(P, p), wgt)
    G = P["gh"] * P["gw"]
    carry = f[None] * (R.spread(P, bf, wgt, absolute=True).sum(axis=(1, 2)) / math.sqrt(G))[:, None, None]
    bq = carry + ba + 2 * U * np.abs(qr)
    rq = float((np.abs(q - qr) / bq).max())
    print(f"nc_normal: max |err| {np.abs(q - qr).max():.3e}, worst err / bound {rq:.3f}")
    assert rq <= 1.0
    # one prox_dual
    aty = R.adjoint(P, ys, wgt)
    xs, zs, us = _iterate(xr, z0, u0)
    with GB.watch(outputs={"z": zs, "u": us}, inputs={"x": xs}):
        e.prox_dual(xs, zs, us, g_f32(mu))
    zr, ur, rr = R.prox_dual(P, xr, z0, u0, aty, mu64, K, wgt)
    res = e.nc_cg_residual().cpu().numpy().astype(np.float64)
    bmax, brms, bres = (MARGIN * v for v in F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"prox_dual K={K}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    # the DC column
    dc = e.residuals(xs, zs, us, dc=True).cpu().numpy().astype(np.float64)[:, 5]
    dcr = R.dc_misfit(P, xr, ys, wgt)
    s = R.op_norm(P)
    bdc = 1e-6 * s * math.sqrt(float(wgt.max())) * np.linalg.norm(xr.reshape(n, -1), axis=1) + 5e-7 * dcr
    print(f"dc column {dc} ref {dcr} |d| {np.abs(dc - dcr)} bound {bdc}")
    assert (np.abs(dc - dcr) <= bdc).all()
    # three steps under the TV prior: the float64 stage on the device's own x (the check is of the new stage alone); slice 1 stopped in step 2
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = g_f32(np.full(n, 0.05, dtype=np.float32))
    t_state = GB.guarded((n,), torch.float32, DEV, fill=0.0)
    for step in range(3):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [t.clone() for t in (xs, zs, us, t_state)]
        tact = g_f32(np.array([0.0, 1.0 if step == 1 else 0.0, 0.0], dtype=np.float32))
        with GB.watch(outputs={"x": xs, "z": zs, "u": us, "t": t_state}, inputs={"mu": sig}):
            e.step(xs, zs, us, g_f32(mu), sig, t_action=tact, t_state=t_state)
        xd = _np(xs)[:, 0]
        zr, ur, rr = R.prox_dual(P, xd, zin, uin, aty, mu64, K, wgt)
        live = [0, 2] if step == 1 else [0, 1, 2]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {e.nc_cg_residual().cpu().numpy()}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:                                                               # the stopped slice keeps x, z, u and t bit for bit
            for name, t, kp in zip("xzut", (xs, zs, us, t_state), keep):
                assert _same(t[1], kp[1]), name
    # the frozen case: y = 0, x0 = 0 never produces NaN
    zero = np.zeros((n, P["m"]), dtype=np.complex64)
    x, z, u = e.reset_nc(g_c64(np.zeros((n, 1, h, w), dtype=np.complex64)), g_c64(zero), None, cg_iters=K)
    e.prox_dual(x, z, u, g_f32(mu))
    assert not _bits(z).any() and not _bits(u).any() and not e.nc_cg_residual().any()
    e.step(x, z, u, g_f32(mu), sig)
    assert torch.isfinite(torch.view_as_real(z)).all() and torch.isfinite(x).all() and torch.isfinite(torch.view_as_real(u)).all()


def test_cartesian_bin_trajectory_equals_the_closed_form_and_leaves_no_trace():
    n, h, w, J = 2, 16, 16, 8
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=5)
    mask = np.asarray(d["mask"]).astype(bool).reshape(h, w)
    traj, (jj, ll) = R.mask_traj(mask)
    y0 = np.ascontiguousarray(d["y0"]).view(np.float32).reshape(n, h, w, 2)
    y0c = (y0[..., 0] + 1j * y0[..., 1]).astype(np.complex64)
    rng = np.random.default_rng(3)
    xr = rng.random((n, h, w)).astype(np.float32)
    u0 = (0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w)))).astype(np.complex64)
    mu = g_f32(np.full(n, 0.3, dtype=np.float32))
    mk = torch.from_numpy(mask).to(DEV)

    def closed(eng):
        eng.set_kspace(torch.from_numpy(y0c).reshape(n, 1, h, w).to(DEV), mk)
        xs, zs, us = _iterate(xr, np.zeros_like(u0), u0)
        eng.prox_dual(xs, zs, us, mu)
        return zs, us

    fresh = closed(_engine(n, h, w))
    e = _engine(n, h, w)
    e.nufft_plan(traj, grid=(32, 32), width=J)
    e.set_kspace_nc(g_c64(y0c[:, jj, ll]), None, cg_iters=2)
    xs, zs, us = _iterate(xr, xr.astype(np.complex64) + u0, u0)                     # warm start anywhere: two iterations are exact
    e.prox_dual(xs, zs, us, mu)
    dz, du = float((zs - fresh[0]).abs().max()), float((us - fresh[1]).abs().max())
    # the host test's model error (twice the measured figure, relative to max |z|) plus the float32 rounding of the C = 1 cross-check
    bound = C1K2_BOUND + 2 * CLOSED_FORM_ERR * float(fresh[0].abs().max())
    print(f"Cartesian-bin trajectory, K = 2: max |z_nc - z_closed| {dz:.3e}, |du| {du:.3e} (bound {bound:.2e}); cg_res {e.nc_cg_residual().cpu().numpy()}")
    assert dz <= bound and du <= bound
    after = closed(e)                                                               # back in the single-coil stage: a fresh handle's bits
    assert _same(after[0], fresh[0]) and _same(after[1], fresh[1])
    with pytest.raises(_lib.PnPError, match="non-Cartesian mode"):
        e.nc_normal(zs, mu)


# ---- mode, state, workspace ------------------------------------------------------------------------------------------------------------------

def test_state_errors_replanning_and_workspace_accounting():
    i = 0
    P, traj, x, y = case(i)
    n, h, w, gh, gw, J = R.CASES[i]
    e = _engine(n, h, w)
    m = P["m"]
    img, smp = g_c64(x), GB.guarded((n, m), torch.complex64, DEV, fill=0.0)
    assert e.nufft_samples == 0
    for call in (lambda: raw_forward(e, img, smp), lambda: raw_adjoint(e, smp, None, GB.guarded((n, h, w), torch.complex64, DEV)),
                 lambda: e.set_kspace_nc(smp), lambda: e.acquire_nc(g_f32(np.zeros((n, 1, h, w))), 0.0, 1)):
        with pytest.raises(_lib.PnPError, match="no NUFFT plan"):
            call()
    ws0 = e.workspace_bytes
    # refused plans change nothing: the grid rule, a side that is no k-space side, a coordinate out of range, a bad width
    bad = traj.copy()
    bad[5, 1] = 0.51
    for kw, tj in ((dict(grid=(16, 32)), traj), (dict(grid=(48, 32)), traj), (dict(), bad), (dict(width=5), traj)):
        with pytest.raises(_lib.PnPError, match="pnp_nufft_plan"):
            e.nufft_plan(tj, **kw)
    assert e.workspace_bytes == ws0 and e.nufft_samples == 0
    e.nufft_plan(traj, grid=(gh, gw), width=J)
    bins = sum(len(R.tiles_of(P, s)) for s in range(m))
    want = 8 * n * gh * gw + 8 * n * m + 8 * m + 8 * J * m + 4 * (h + w) + 8 * (gh + gw) + 4 * (gh * gw // 256 + 1) + 4 * bins
    print(f"pnp_nufft_plan grew the workspace by {e.workspace_bytes - ws0} bytes, documented {want} ({bins} bin entries)")
    assert e.workspace_bytes - ws0 == want
    with pytest.raises(_lib.PnPError, match="batch"):
        _lib.check(e.lib.pnp_nufft_forward(e._h, img.data_ptr(), n + 1, smp.data_ptr(), e._stream()), "pnp_nufft_forward")
    with pytest.raises(_lib.PnPError, match="alias"):
        _lib.check(e.lib.pnp_nufft_forward(e._h, img.data_ptr(), n, img.data_ptr(), e._stream()), "pnp_nufft_forward")
    GB.check({"img": img, "samples": smp})
    big = _engine(1, 1024, 16)
    with pytest.raises(_lib.PnPError, match="1024"):
        big.nufft_plan(traj)
    # constants: installing grows by the documented amounts, a second install by nothing
    ws1 = e.workspace_bytes
    wgt = g_f32(np.ones(m, dtype=np.float32))
    e.set_kspace_nc(g_c64(y), wgt, cg_iters=2)
    chunks = (h * w + 2047) // 2048
    want = 8 * n * m + 4 * m + 8 * n * ((m + 2047) // 2048) + 4 * 8 * n * h * w + 16 * n * chunks + 64 * n
    print(f"pnp_set_kspace_nc grew the workspace by {e.workspace_bytes - ws1} bytes, documented {want}")
    assert e.workspace_bytes - ws1 == want
    e.set_kspace_nc(g_c64(y), wgt, cg_iters=2)
    assert e.workspace_bytes == ws1 + want
    # re-planning drops the non-Cartesian constants: no episode constants are left; Cartesian ones are not touched by a plan
    xs, zs, us = _iterate(np.zeros((n, h, w)), np.zeros((n, h, w)), np.zeros((n, h, w)))
    mu = g_f32(np.full(n, 0.3))
    e.prox_dual(xs, zs, us, mu)
    e.nufft_plan(traj, grid=(gh, gw), width=J)
    with pytest.raises(_lib.PnPError, match="pnp_reset"):
        e.prox_dual(xs, zs, us, mu)
    with pytest.raises(_lib.PnPError, match="non-Cartesian mode"):
        e.nc_cg_residual()
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=5)
    y0 = np.ascontiguousarray(d["y0"]).view(np.float32).reshape(n, 1, h, w, 2)
    e.set_kspace(torch.view_as_complex(torch.from_numpy(y0.copy())).to(DEV), torch.from_numpy(np.asarray(d["mask"]).reshape(h, w)).to(DEV))
    xs, zs, us = _iterate(np.zeros((n, h, w)), np.zeros((n, h, w)), np.zeros((n, h, w)))
    e.prox_dual(xs, zs, us, mu)
    ref = (zs.clone(), us.clone())
    xs, zs, us = _iterate(np.zeros((n, h, w)), np.zeros((n, h, w)), np.zeros((n, h, w)))
    e.nufft_plan(traj, grid=(gh, gw), width=4)                                      # a plan while Cartesian constants are live: they stay
    e.prox_dual(xs, zs, us, mu)
    assert _same(zs, ref[0]) and _same(us, ref[1])


# ---- acquisition -------------------------------------------------------------------------------------------------------------------------------

def test_acquire_nc_is_the_forward_without_noise_and_matches_the_float64_ndft_with_it():
    i = 1
    P, traj = case(i)[:2]
    n, h, w = R.CASES[i][:3]
    gt = np.stack([synthetic.phantom(h, w, 40 + j) for j in range(n)]).astype(np.float32)
    e = planned(i)
    dcf = (0.2 + np.abs(traj).sum(axis=1)).astype(np.float32)
    y, aty, x0 = e.acquire_nc(g_f32(gt, (n, 1, h, w)), 0.0, 7, dcf=g_f32(dcf))
    f = e.nufft_forward(g_c64(gt.astype(np.complex64)))
    assert _same(y, f)
    assert _same(aty.reshape(n, h, w), e.nufft_adjoint(y, g_f32(dcf)))
    assert torch.equal(torch.view_as_real(x0), torch.view_as_real(aty).clamp_min(0))
    sigma, seed = 5.0 / 255.0, 99
    yn = _np(e.acquire_nc(g_f32(gt, (n, 1, h, w)), sigma, seed)[0])
    ref = R.ndft(traj, gt.astype(np.float64))
    for j in range(n):
        ref[j] += sigma * (synthetic._gauss(seed + j, 9001, P["m"]) + 1j * synthetic._gauss(seed + j, 9003, P["m"]))
    rel = float(np.linalg.norm(yn - ref) / np.linalg.norm(ref))
    bound = 1e-6 + 2 * MODEL_J6_64
    print(f"acquire_nc with noise against the float64 NDFT: rel l2 {rel:.3e} (bound {bound:.2e})")
    assert rel <= bound
    noise = yn - _np(f)
    rn = float(np.linalg.norm(noise - (ref - R.ndft(traj, gt.astype(np.float64)))) / np.linalg.norm(noise))
    print(f"the noise alone against synthetic._gauss: rel l2 {rn:.3e}")
    bn = 2 * U * float(np.linalg.norm(yn) / np.linalg.norm(noise))                  # one float32 rounding of each component of transform + noise
    print(f"(bound {bn:.2e})")
    assert rn <= bn


def test_simulate_with_a_trajectory_matches_make_problem_nc():
    """acquisition.simulate(traj=, dcf=) (pnp_nufft_plan + pnp_acquire_nc) against synthetic.make_problem_nc, the exact NDFT in float64 with
    the same counter-hash noise: y0 to the acquisition bound of the module docstring; ATy0 and x0 are the device's own adjoint of its y0."""
    from dt4image_restoration_amd import acquisition
    n, h, w, spokes = 2, 64, 64, 13
    traj = acquisition.radial_trajectory(h, w, spokes)
    assert np.array_equal(traj, R.radial(h, w, spokes))
    dcf = acquisition.radial_dcf(traj, h, w)
    ref = synthetic.make_problem_nc(n, h, w, traj, dcf=dcf, sigma_n=5.0 / 255.0, seed=40)
    e = _engine(n, h, w)
    d = acquisition.simulate(e, ref["gt"], None, 5.0 / 255.0, 40, traj=traj, dcf=dcf)
    assert d["y0"].shape == (n, 1, traj.shape[0], 2) and d["ATy0"].shape == (n, 1, h, w, 2) and e.nufft_grid == (80, 80)
    y = _np(torch.view_as_complex(d["y0"]))
    yr = ref["y0"][..., 0].astype(np.float64) + 1j * ref["y0"][..., 1].astype(np.float64)
    rel = float(np.linalg.norm(y - yr) / np.linalg.norm(yr))
    bound = 1e-6 + 2 * MODEL_J6_64
    a = _np(torch.view_as_complex(d["ATy0"]))
    ar = ref["ATy0"][..., 0].astype(np.float64) + 1j * ref["ATy0"][..., 1].astype(np.float64)
    print(f"simulate(traj=): y0 rel l2 {rel:.3e} (bound {bound:.2e}); ATy0 rel l2 against the exact adjoint {np.linalg.norm(a - ar) / np.linalg.norm(ar):.3e} "
          f"(recorded, not asserted: the adjoint's model error has no bound from the host test)")
    assert rel <= bound
    assert _same(torch.view_as_complex(d["ATy0"]).reshape(n, h, w), e.nufft_adjoint(torch.view_as_complex(d["y0"]).reshape(n, -1).contiguous(), d["dcf"]))
    assert torch.equal(d["x0"], d["ATy0"].clamp_min(0))


def test_env_reset_and_step_with_a_trajectory_and_rebinding_across_episodes():
    """PnPEnv.reset / step with data["traj"] (TV prior set on the env's engine): the same bits as the engine driven directly; a second
    episode on ANOTHER trajectory re-plans, and stepping the first episode again re-plans back and re-installs its constants."""
    from dt4image_restoration_amd import acquisition
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    n, h, w = 2, 64, 64
    env = PnPEnv(30, UNetDenoiser2D.seeded(0), "cuda", cg_iters=4)
    data = []
    for spokes in (13, 8):
        traj = acquisition.radial_trajectory(h, w, spokes)
        gt = np.stack([synthetic.phantom(h, w, 60 + j) for j in range(n)]).astype(np.float32)
        data.append(acquisition.simulate(env, gt, None, 5.0 / 255.0, 11, traj=traj, dcf=acquisition.radial_dcf(traj, h, w)))
    act = {"mu": torch.full((n,), 0.3), "sigma_d": torch.full((n,), 0.05), "T": torch.zeros(n)}
    st = [env.reset(d, "cuda") for d in data]
    eng = env._engine
    eng.set_prior("tv", tv_scale=1.0, tv_iters=5)
    assert eng.nufft_samples == 8 * 128 and eng.coils == 0
    env.step(st[0], act)                                                            # re-plans for the first trajectory, re-installs
    assert eng.nufft_samples == 13 * 128
    env.step(st[1], act)
    env.step(st[0], act)
    direct = _engine(n, h, w)
    direct.set_prior("tv", tv_scale=1.0, tv_iters=5)
    direct.nufft_plan(data[0]["traj"])
    x0 = torch.view_as_complex(data[0]["x0"].contiguous())
    x, z, u = direct.reset_nc(x0, torch.view_as_complex(data[0]["y0"].contiguous()).reshape(n, -1).contiguous(), data[0]["dcf"], cg_iters=4)
    mu, sg = torch.full((n,), 0.3, device=DEV), torch.full((n,), 0.05, device=DEV)
    for _ in range(2):
        direct.step(x, z, u, mu, sg)
    assert _same(st[0]["x"], x) and _same(st[0]["z"], z) and _same(st[0]["u"], u)
    p0 = env.compute_reward(torch.view_as_complex(data[0]["x0"].contiguous()).real, st[0]["gt"])
    p2 = env.compute_reward(st[0]["x"], st[0]["gt"])
    print(f"PSNR of x0 {p0.reshape(-1).tolist()} dB, after two TV steps {p2.reshape(-1).tolist()} dB")
    assert torch.isfinite(p2).all()


def _mat(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items() if v is not None}


def test_end_to_end_tv_admm_through_the_fixed_schedule_solver(record_property):
    """The fixture of the module docstring: the float64 restatement first (its gain over x0 is the condition on the input), then the
    device through PnPEnv.reset(data with traj, dcf) and FixedScheduleSolver."""
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    t = R.FIXTURE
    d, P = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    x64, p0, p64 = R.admm_tv_nc(d, P, mu, sig, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"float64 restatement: PSNR of x0 {p0}, final {p64} dB (recorded {R.FIXTURE_PSNR})")
    assert (p64 - p0 >= 1.0).all()
    env = PnPEnv(max_episode_step=t["iters"], denoiser=TVDenoiser2D(scale=t["tv_scale"], iters=t["tv_iters"]), device_type="cuda",
                 cg_iters=t["cg_iters"], nufft_width=t["width"])
    r = FixedScheduleSolver(env, max_iter=t["iters"], dc=True).run(_mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    gt = d["gt"][:, 0].astype(np.float64)
    import tv_ref
    pdev = tv_ref.psnr(_np(r.x)[:, 0], gt)                                         # float64 from the device's iterate, as the restatement's figure
    dp, dx = float(np.abs(pdev - p64).max()), float(np.abs(_np(r.x)[:, 0] - x64).max())
    print(f"device: PSNR of x0 {r.initial_psnr.reshape(-1).tolist()}, final {pdev} (engine's own {r.psnr.reshape(-1).tolist()}), |dPSNR| {dp:.3e} dB, "
          f"max |dx| {dx:.3e}, dc {r.dc.tolist()}, cg_res {env._engine.nc_cg_residual().cpu().tolist()}")
    record_property("max_abs_dpsnr_db", dp)
    record_property("max_abs_dx", dx)
    assert dp <= 0.01
    assert abs(float(r.psnr.reshape(-1)[0]) - float(p64[0])) <= 0.01              # what the engine itself reports (float32)


def test_cli_traj_radial_fixed_on_a_ground_truth_folder(tmp_path):
    import contextlib
    import io
    import json
    from dt4image_restoration_amd import cli
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5), synthetic.phantom(64, 64, 6)]).astype(np.float32))
    base = ["--block_size", "6", "--n_embeds", "9", "--gt", str(gtd), "--tasks", "4x_5", "--prior", "tv", "--seed", "3"]
    with pytest.raises(SystemExit, match="--traj with --coils"):
        cli.main(base + ["--traj", "radial", "--coils", "4", "fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit, match="need --traj radial"):
        cli.main(base + ["--spokes", "8", "fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit, match="--traj radial: task 4x_5"):               # a 64 x 64 grid for a 64 x 64 slice breaks the grid rule
        cli.main(base + ["--traj", "radial", "--nufft-grid", "64", "64", "fixed", "--max_iter", "2"])

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = cli.main(base + ["--traj", "radial"] + extra + ["fixed", "--max_iter", "10", "--dc"])
        lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
        assert lines == out and len(out) == 1 and out[0]["n"] == 2 and "radial-nc" in out[0]["set"]
        return out[0]

    a = run([])                                                                     # spokes from the task: ceil(64 / 4) = 16
    b = run(["--spokes", "32", "--nufft-width", "8", "--nufft-grid", "128", "80", "--cg-iters", "4"])
    c = run(["--nc-weights", "none"])
    print(f"cli --traj radial fixed: 16 spokes {a['psnr']:.3f} dB (+{a['psnr_increment']:.3f}), 32 spokes J=8 {b['psnr']:.3f} dB "
          f"(+{b['psnr_increment']:.3f}), unweighted {c['psnr']:.3f} dB (+{c['psnr_increment']:.3f}); dc {a['dc']:.4f} {b['dc']:.4f} {c['dc']:.4f}")
    for r in (a, b, c):
        assert np.isfinite(r["psnr"]) and r["psnr_increment"] > 1.0 and r["dc"] > 0.0
    assert b["psnr"] > a["psnr"]                                                    # twice the spokes restore more
