"""The least-squares temporal interpolator of the off-resonance operator on the MI355X (include/pnpadmm_offres_ls.h), through the C ABI,
against tests/offres_ls_ref.py.  The shapes, the data and the helpers are those of tests/test_gpu_offres.py (imported read-only).  Every model
here is built from the DEVICE's own coefficient table (pnp_offres_ls_coeffs) and the device's maps.  Every figure is printed before it is
asserted.  No bound here is measured on the device.

BOUNDS.
  L = 1, dense against naive, plan switching, invariance under the block size: torch.equal (numbers) or the bits.
  Rounding level, against the float64 model on the NUFFT plan: tests/test_gpu_offres.py's `forward_err_norm` / `adjoint_err` with the
  coefficient table in the place of b0, b1.  Forward: per plane the forward bound of tests/test_gpu_nufft.py weighted by |b_l|; the rounding
  of the segment image (three roundings through an operator of norm s_nu) enters plane l with at most max_m |b_l| - the linear case's
  b0^2 + b1^2 <= 1 is not available, the sum over l of max_m |b_l| stands in; the blend is a chain of L terms, gamma(L + 1) on
  sum_l |b_l| |v_l|.  Adjoint: the same expression as the linear case's, over all L planes (|b_l| is inside the samples b_l . q).
  Against the dense segmented restatement: model_tol(h, w, J) max_m sum_l |b_l| relative l2 - a per-plane NUFFT error enters with |b_l|.
  Against the exact operator, per sample: that tolerance times ||ref|| plus eps ||p||_1 / sqrt(H W), eps = acquisition.offres_ls_error at
  the map's own values with the device's coefficients.  Adjointness: tests/test_gpu_offres.py's bound.
  Stage: that file's tolerances (ten times the float32 restatement of the CG at mu = 0.3, K = 4), scaled by kappa(least squares) /
  kappa(linear) = (||A^H W A|| + mu) of the two float64 models, never below 1; the DC column's bound with s_nu max sum |b| for the operator
  norm.
  Fixture: within 0.01 dB of offres_ls_ref.CORRECTS_LS (float64, CPU) and not below the linear L = 32 run of the same test.

MEASURED on one MI355X: forward against the float64 model ||err|| 2.6e-06 .. 2.2e-05 (bounds 3.4e-04 .. 9.6e-03), adjoint at most 0.006 of its
bound, adjointness 2.3e-09 .. 1.1e-08 of ||p|| ||q||; against the dense segmented restatement 1.1e-05 (32 x 32, J = 6) .. 1.0e-02 (80 x 64,
J = 4), 0.11 to 0.47 of the tolerance; against the exact operator 5.1e-05 of a bound 4.4e-03 at L = 10 (eps 3.8e-05) and 3.2 of 21.7 at L = 2
(eps 1.1: two segments do not fit 2 pi); CG stage err_max 2.0e-06 .. 3.1e-06 of 1.06e-05 (||A^H W A|| 5.82 against the linear stage's 5.45:
tolerances times 1.065), DC column 1.5e-07 of 7.6e-04; the fixture 50.573 dB with a misfit at x = gt of 4.38e-03, the linear L = 32 run
50.549 dB and 2.33e-02, through PnPEnv and FixedScheduleSolver 50.573 dB."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcf_ref as D  # noqa: E402
import guard_bands as GB  # noqa: E402
import nufft_ref as NR  # noqa: E402
import offres_ls_ref as LS  # noqa: E402
import offres_ref as OR  # noqa: E402
import test_gpu_nufft as TN  # noqa: E402
import test_gpu_offres as TO  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = TO.DEV
U = TO.U
c64, f32, _np, _same, _bits, gamma = TO.c64, TO.f32, TO._np, TO._same, TO._bits, TO.gamma
GRIDS = dict(TO.GRIDS)


def setup(h, w, kind, J):
    if J in (4, 6):
        return TO.setup(h, w, kind, J)
    key = (h, w, kind, J)                                                           # J = 8: the same trajectory, times and maps on a plan of that width
    if key not in TO._SETUP:
        traj, t, _, om = TO.setup(h, w, kind, 6)
        gh, gw = GRIDS[(h, w)]
        TO._SETUP[key] = (traj, t, NR.plan(h, w, gh, gw, J, traj), om)
    return TO._SETUP[key]


def band_of(om):
    return float(np.abs(om).max()) * (1.0 + 1e-6)


def _engine(n, h, w, monkeypatch=None, naive=None, block=None, noskip=None):
    from dt4image_restoration_amd.engine import PnPEngine
    if monkeypatch is not None:
        for name, v in (("PNP_OFFRES_LS_NAIVE", naive), ("PNP_OFFRES_SEG_BLOCK", block), ("PNP_OFFRES_LS_NOSKIP", noskip)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(int(v)))
    return PnPEngine(n, h, w, device=0, denoiser=False)


def planned(n, h, w, kind, J, L, interp="ls", **env):
    traj, t, P, om = setup(h, w, kind, J)
    e = _engine(n, h, w, **env)
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=J)
    if interp == "ls":
        e.offres_plan_ls(t, L, band_of(om))
    else:
        e.offres_plan(t, L)
    return e


# ---- exact anchors ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,J,n", ((16, 16, "radial", 6, 2), (80, 64, "spiral", 4, 3)))
def test_one_segment_has_the_bits_of_the_linear_plan(h, w, kind, J, n):
    traj, t, P, om = setup(h, w, kind, J)
    e, lin = planned(n, h, w, kind, J, 1), planned(n, h, w, kind, J, 1, interp="linear")
    assert e.offres_segments == 1 and e.offres_interpolator() == "ls" and lin.offres_interpolator() == "linear"
    assert (e.offres_ls_coeffs() == 1.0).all()
    x, y, wgt = TO._data(n, h, w, P["m"])
    for omega in (om[0], om[:n]):
        maps = e.offres_maps(f32(omega))
        assert _same(maps, lin.offres_maps(f32(omega)))
        assert _same(e.offres_forward(c64(x), maps), lin.offres_forward(c64(x), maps))
        for wd in (None, f32(wgt)):
            assert _same(e.offres_adjoint(c64(y), maps, wd), lin.offres_adjoint(c64(y), maps, wd))


def _three(e, h, w, J, n, om, P):
    """forward, adjoint (weighted) and the normal operator of the installed stage"""
    x, y, wgt = TO._data(n, h, w, P["m"], seed=3)
    od = f32(om[:n])
    maps = e.offres_maps(od)
    f = e.offres_forward(c64(x), maps)
    a = e.offres_adjoint(c64(y), maps, f32(wgt))
    a0 = e.offres_adjoint(c64(y), maps, None)
    e.set_kspace_offres(c64(y), od, f32(wgt), cg_iters=2)
    q = e.offres_normal(c64(x, (n, 1, h, w)), f32(TO.MU3[:n]))
    return f, a, a0, q


@pytest.mark.parametrize("h,w,kind,J,L", ((16, 16, "radial", 6, 2), (32, 32, "spiral", 6, 10), (80, 64, "radial", 4, 3), (128, 128, "spiral", 8, 8),
                                          (16, 16, "spiral", 6, 32)))
def test_the_dense_form_equals_the_naive_form_for_every_segment_block(h, w, kind, J, L, monkeypatch):
    """L = 10 at block 8 is the case where a partial crosses a block; J = 8 with 8 segments in a block is the register-heaviest instantiation"""
    n = 2
    traj, t, P, om = setup(h, w, kind, J)
    outs = {}
    for naive in (1, 0):
        for block in (1, 3, 8):
            e = planned(n, h, w, kind, J, L, monkeypatch=monkeypatch, naive=naive, block=block)
            outs[(naive, block)] = _three(e, h, w, J, n, om, P)
    outs[(0, "noskip")] = _three(planned(n, h, w, kind, J, L, monkeypatch=monkeypatch, naive=0, block=8, noskip=1), h, w, J, n, om, P)
    outs[("shipped", None)] = _three(planned(n, h, w, kind, J, L, monkeypatch=monkeypatch), h, w, J, n, om, P)
    ref = outs[(1, 8)]
    names = ("forward", "adjoint", "adjoint (no weights)", "normal")
    assert all(torch.isfinite(torch.view_as_real(v)).all() and bool(v.abs().max() > 0) for v in ref)
    for key, got in outs.items():
        for name, a, b in zip(names, ref, got):
            assert torch.equal(a, b), (name, key)
    for form in (0, 1):                                                             # within one form the block size changes no bit
        for block in (1, 3):
            for name, a, b in zip(names, outs[(form, 8)], outs[(form, block)]):
                assert _same(a, b), (name, form, block)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------

def forward_err_norm(P, B, E, x, ref_planes):
    n, L = x.shape[0], B.shape[0]
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    aB = np.abs(B)
    per = sum(aB[l] * TN.forward_bound(P, E4[:, l] * x) for l in range(L))
    img = float(aB.max(axis=1).sum()) * np.linalg.norm(x.reshape(n, -1), axis=1)
    chain = sum(aB[l] * np.abs(ref_planes[l]) for l in range(L))
    return np.linalg.norm(per, axis=1) + NR.op_norm(P) * gamma(3) * img + gamma(L + 1) * np.linalg.norm(chain, axis=1)


def adjoint_err(P, B, E, y, wgt):
    n, L = y.shape[0], B.shape[0]
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    out = np.zeros((n, P["h"], P["w"]))
    for l in range(L):
        yl = B[l] * y
        out += np.abs(E4[:, l]) * (TN.adjoint_bound(P, yl, wgt)[0] + gamma(4 * L) * np.abs(NR.adjoint(P, yl, wgt)))
    return out


@pytest.mark.parametrize("h,w,kind,J,L,n", ((16, 16, "radial", 6, 2, 1), (32, 32, "spiral", 6, 10, 2), (80, 64, "radial", 4, 3, 2),
                                            (128, 128, "spiral", 6, 8, 1), (16, 16, "spiral", 6, 32, 1)))
def test_forward_and_adjoint_against_the_model_the_segmented_and_the_exact_restatement(h, w, kind, J, L, n):
    traj, t, P, om = setup(h, w, kind, J)
    m = P["m"]
    e = planned(n, h, w, kind, J, L)
    B = e.offres_ls_coeffs().astype(np.float64)
    assert B.shape == (L, m)
    tau = LS.centres(t, L)
    ref_b = acquisition.offres_ls_coeffs(t, L, band_of(om))
    sab = float(np.abs(B).sum(axis=0).max())
    print(f"{h}x{w} {kind} J={J} L={L}: device coefficients: max sum |b| {sab:.2f}, max |b| {np.abs(B).max():.2f}, max |b - numpy| {np.abs(B - ref_b).max():.3e}")
    assert np.abs(B - ref_b).max() <= 1e-3 * np.abs(ref_b).max()
    x, y, wgt = TO._data(n, h, w, m, seed=L)
    omega = om[:n].astype(np.float64)
    maps = e.offres_maps(f32(om[:n]))
    got_f, got_a = _np(e.offres_forward(c64(x), maps)), _np(e.offres_adjoint(c64(y), maps, f32(wgt)))
    # at rounding level, against the float64 model on the plan with the device's own maps and coefficients
    E = _np(maps)
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    planes = [NR.forward(P, E4[:, l] * x) for l in range(L)]
    mod_f, mod_a = sum(B[l] * planes[l] for l in range(L)), LS.model_adjoint(P, B, E, y, wgt)
    bf, ba = forward_err_norm(P, B, E, x, planes), adjoint_err(P, B, E, y, wgt)
    ef = np.linalg.norm(got_f - mod_f, axis=1)
    ra = float((np.abs(got_a - mod_a) / ba).max())
    print(f"        against the float64 model: forward ||err|| {ef.tolist()} bound {bf.tolist()}; adjoint worst err / bound {ra:.3f}")
    assert (ef <= bf).all() and ra <= 1.0
    # against the dense segmented restatement: the NUFFT's own error, per plane with weight |b_l|
    ref_f, ref_a = LS.segmented_forward(traj, tau, B, omega, x), LS.segmented_adjoint(traj, tau, B, omega, y, h, w, wgt)
    tol = TO.model_tol(h, w, J) * sab
    rf = float(np.linalg.norm(got_f - ref_f) / np.linalg.norm(ref_f))
    rr = float(np.linalg.norm(got_a - ref_a) / np.linalg.norm(ref_a))
    print(f"        against the dense segmented restatement: forward rel l2 {rf:.3e}, adjoint rel l2 {rr:.3e} (tolerance {tol:.3e})")
    assert rf <= tol and rr <= tol
    # against the exact operator
    if L > 1:
        ex = OR.exact_forward(traj, t, omega, x)
        eps = acquisition.offres_ls_error(t, L, band_of(om), omega=omega, coef=B)
        l1 = np.abs(x).reshape(n, -1).sum(axis=1) / math.sqrt(h * w)
        bnd = tol * np.linalg.norm(ref_f.reshape(n, -1), axis=1) + eps * l1
        err = np.abs(got_f - ex).max(axis=1)
        print(f"        against the exact operator: max |err| {err.tolist()} bound {bnd.tolist()} (eps {eps:.3e}, of the bound eps ||p||_1: {(eps * l1).tolist()})")
        assert (err <= bnd).all()
    # adjointness on the device outputs
    nx, ny = np.linalg.norm(x.reshape(n, -1), axis=1), np.linalg.norm(y, axis=1)
    yw = y * wgt.astype(np.float64)
    lhs = np.array([np.vdot(yw[j], got_f[j]) - np.vdot(got_a[j], x[j]) for j in range(n)])
    lim = bf * np.linalg.norm(yw, axis=1) + np.linalg.norm(ba.reshape(n, -1), axis=1) * nx
    print(f"        adjointness |<A p, W q> - <p, A^H W q>| {np.abs(lhs).tolist()} bound {lim.tolist()} (relative to ||p|| ||q||: {(np.abs(lhs) / (nx * ny)).tolist()})")
    assert (np.abs(lhs) <= lim).all()


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------------

def _norm_of(fwd, adj, h, w, iters=40):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, h, w)) + 1j * rng.standard_normal((1, h, w))
    s = 0.0
    for _ in range(iters):
        x /= np.linalg.norm(x)
        x = adj(fwd(x))
        s = float(np.linalg.norm(x))
    return s


def test_the_stage_step_composition_cg_dc_stopped_slices_and_snapshots():
    h, w, kind, J, L, n, K = 32, 32, "spiral", 6, 8, 3, 4
    traj, t, P, om = setup(h, w, kind, J)
    e = planned(n, h, w, kind, J, L)
    B = e.offres_ls_coeffs().astype(np.float64)
    sab = float(np.abs(B).sum(axis=0).max())
    od = f32(om)
    E = _np(e.offres_maps(od))
    rng = np.random.default_rng(177)
    xr = rng.random((n, h, w)).astype(np.float32).astype(np.float64)
    z0 = TO._rt(xr + 0.05 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    u0 = TO._rt(0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    wgt = D.pipe(P, 30)[0].astype(np.float32)
    ys = TO._rt(LS.model_forward(P, B, E, xr.astype(np.complex128)) + 0.02 * (rng.standard_normal((n, P["m"])) + 1j * rng.standard_normal((n, P["m"]))))
    # the condition-number factor: this operator against the linear stage's of tests/test_gpu_offres.py (L = 3, the same weights), float64 models
    Q3 = OR.plan(t, 3)
    E3 = OR.maps(om[:1].astype(np.float64), Q3)
    s_lin = _norm_of(lambda p: OR.model_forward(P, Q3, E3, p), lambda q: OR.model_adjoint(P, Q3, E3, q, wgt), h, w)
    s_ls = _norm_of(lambda p: LS.model_forward(P, B, E[:1], p), lambda q: LS.model_adjoint(P, B, E[:1], q, wgt), h, w)
    scale = max(1.0, (s_ls + 0.3) / (s_lin + 0.3))
    print(f"||A^H W A||: {s_lin:.3f} linear L = 3, {s_ls:.3f} least squares L = {L}: the CG tolerances are scaled by {scale:.3f}; max sum |b| {sab:.2f}")
    mu = np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    wd = f32(wgt)
    e.set_kspace_offres(c64(ys), od, wd, cg_iters=K)
    assert e.offres_live and e.offres_interpolator() == "ls" and not e.offres_cg_residual().any()
    pd = c64(u0, (n, 1, h, w))
    q = _np(e.offres_normal(pd, f32(mu)))[:, 0]
    comp = _np(e.offres_adjoint(e.offres_forward(pd, e.offres_maps(od)), e.offres_maps(od), wd))
    exact = comp + mu64[:, None, None] * u0
    off = float(max((np.abs(q.real - exact.real) / np.maximum(np.abs(exact.real), 1e-30)).max(),
                    (np.abs(q.imag - exact.imag) / np.maximum(np.abs(exact.imag), 1e-30)).max()))
    print(f"offres_normal against fma(mu, p, adjoint(forward(p))): worst relative distance {off:.3e} (one rounding: {U:.3e})")
    assert off <= U * (1 + 1e-6)
    aty = LS.model_adjoint(P, B, E, ys, wgt)
    xs, zs, us = f32(xr, (n, 1, h, w)), c64(z0, (n, 1, h, w)), c64(u0, (n, 1, h, w))
    e.prox_dual(xs, zs, us, f32(mu))
    zr, ur, rr = LS.prox_dual(P, B, E, xr, z0, u0, aty, mu64, K, wgt)
    res = e.offres_cg_residual().cpu().numpy().astype(np.float64)
    bmax, brms, bres = (scale * TO.MARGIN * v for v in TO.F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"prox_dual K={K}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    dc = e.residuals(xs, zs, us, dc=True).cpu().numpy().astype(np.float64)[:, 5]
    dcr = LS.dc_misfit(P, B, E, xr, ys, wgt)
    bdc = 1e-6 * NR.op_norm(P) * sab * math.sqrt(float(wgt.max())) * np.linalg.norm(xr.reshape(n, -1), axis=1) + 5e-7 * dcr
    print(f"dc column {dc} ref {dcr} |d| {np.abs(dc - dcr)} bound {bdc}")
    assert (np.abs(dc - dcr) <= bdc).all()
    # three steps under the TV prior: each is tv_denoise then prox_dual, bit for bit; slice 1 stopped in step 2
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = f32(np.full(n, 0.05, dtype=np.float32))
    e2 = planned(n, h, w, kind, J, L)
    e2.set_kspace_offres(c64(ys), od, wd, cg_iters=K)
    t_state = torch.zeros(n, dtype=torch.float32, device=DEV)
    for step in range(3):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [v.clone() for v in (xs, zs, us, t_state, e.offres_cg_residual())]
        tact = f32(np.array([0.0, 1.0 if step == 1 else 0.0, 0.0], dtype=np.float32))
        x2, z2, u2 = xs.clone(), zs.clone(), us.clone()
        xp = e2.tv_denoise(z2.real - u2.real, torch.tensor(1.0, dtype=torch.float32, device=DEV) * sig, 5)
        if step == 1:
            xp[1] = x2[1]
        e2.prox_dual(xp, z2, u2, f32(mu), tact)
        e.step(xs, zs, us, f32(mu), sig, t_action=tact, t_state=t_state)
        for name, a, b in zip("xzu", (xs, zs, us), (xp, z2, u2)):
            assert _same(a, b), (f"step {step + 1}: {name} of pnp_step differs from tv_denoise + pnp_prox_dual")
        zr, ur, rr = LS.prox_dual(P, B, E, _np(xs)[:, 0], zin, uin, aty, mu64, K, wgt)
        live = [0, 2] if step == 1 else [0, 1, 2]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:
            for name, a, kp in zip(("x", "z", "u", "t", "cg"), (xs, zs, us, t_state, e.offres_cg_residual()), keep):
                assert _same(a[1], kp[1]), name
    snap = e.snapshot(xs, zs, us, t_state)
    want = [v.clone() for v in (xs, zs, us)]
    e.step(xs, zs, us, f32(mu), sig)
    after = [v.clone() for v in (xs, zs, us)]
    e.restore(snap, xs, zs, us, t_state)
    for a, b in zip((xs, zs, us), want):
        assert _same(a, b)
    e.step(xs, zs, us, f32(mu), sig)
    for a, b in zip((xs, zs, us), after):
        assert _same(a, b)


# ---- the correction corrects ----------------------------------------------------------------------------------------------------------------------

def test_eight_least_squares_segments_correct_as_well_as_thirty_two_linear_on_the_device():
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    c = OR.CORRECTS
    h, w = c["h"], c["w"]
    traj, t, omega, gt, y, L32 = OR.corrects_problem()
    m, L = traj.shape[0], LS.CORRECTS_LS_L
    e = _engine(1, h, w)
    e.nufft_plan(traj, grid=GRIDS[(h, w)], width=c["J"])
    dcf = e.nufft_dcf(iters=30)
    od, yd = f32(omega.astype(np.float32)), c64(y.reshape(1, m))
    mu = f32(np.full(1, c["mu"], dtype=np.float32))
    sig = OR.corrects_schedule()
    e.set_prior("tv", tv_scale=1.0, tv_iters=c["tv_iters"])
    gd, zg = f32(gt.astype(np.float32), (1, 1, h, w)), c64(gt.astype(np.complex64), (1, 1, h, w))
    out = {}
    for name in ("ls", "linear"):
        if name == "ls":
            e.offres_plan_ls(t, L, band_of(omega))
        else:
            e.offres_plan(t, L32)
        x0 = e.offres_adjoint(yd, e.offres_maps(od), dcf).reshape(1, 1, h, w)
        x, z, u = e.reset_offres(x0, yd, od, dcf, cg_iters=c["K"])
        dc_gt = float(e.residuals(gd, zg, torch.zeros_like(zg), dc=True)[0, 5])
        for k in range(c["steps"]):
            e.step(x, z, u, mu, f32(sig[k:k + 1]))
        out[name] = (TO._psnr(_np(x)[0, 0], gt), dc_gt)
    print(f"least squares L = {L}: {out['ls'][0]:.3f} dB, misfit at x = gt {out['ls'][1]:.4e}; linear L = {L32}: {out['linear'][0]:.3f} dB, "
          f"{out['linear'][1]:.4e} (float64: {LS.CORRECTS_LS}, {OR.CORRECTS_PSNR[0]})")
    assert abs(out["ls"][0] - LS.CORRECTS_LS[0]) <= 0.01 and out["ls"][0] >= out["linear"][0] and out["ls"][1] < out["linear"][1]
    # the same through the environment and the fixed-schedule solver: data["b0_interp"]
    env = PnPEnv(max_episode_step=c["steps"], denoiser=TVDenoiser2D(scale=1.0, iters=c["tv_iters"]), device_type="cuda", cg_iters=c["K"],
                 nufft_width=c["J"], nufft_grid=c["grid"])
    eng = env._engine_for(1, h, w, torch.device("cuda", 0))
    dcf = acquisition.pipe_dcf(env, traj, iters=30, width=c["J"], grid=c["grid"])
    eng.offres_plan_ls(t, L, band_of(omega))
    x0 = eng.offres_adjoint(yd, eng.offres_maps(od), dcf).reshape(1, 1, h, w)
    mat = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(c64(y.reshape(1, 1, m))), "ATy0": torch.view_as_real(x0), "gt": gd,
           "traj": torch.from_numpy(traj), "dcf": dcf, "omega": od, "times": torch.from_numpy(t), "segments": L, "b0_interp": "ls"}
    r = FixedScheduleSolver(env, max_iter=c["steps"], dc=True).run(mat, np.full((1, c["steps"]), c["mu"], dtype=np.float32), sig[None])
    assert env._engine.offres_live and env._engine.offres_segments == L and env._engine.offres_interpolator() == "ls"
    p = TO._psnr(_np(r.x)[0, 0], gt)
    print(f"through PnPEnv and FixedScheduleSolver: {p:.3f} dB")
    assert abs(p - LS.CORRECTS_LS[0]) <= 0.01 and p >= out["linear"][0]


# ---- the handle -----------------------------------------------------------------------------------------------------------------------------------

def test_plan_switching_gives_each_plan_its_own_bits_and_drops_what_was_built_on_the_old_one():
    h, w, kind, J, L, n = 32, 32, "spiral", 6, 8, 2
    traj, t, P, om = setup(h, w, kind, J)
    own = {k: _three(planned(n, h, w, kind, J, L, interp=k), h, w, J, n, om, P) for k in ("ls", "linear")}
    assert not torch.equal(own["ls"][0], own["linear"][0])
    e = planned(n, h, w, kind, J, L)
    for k in ("linear", "ls", "linear"):                                            # a linear plan after a least-squares plan, and the reverse
        if k == "ls":
            e.offres_plan_ls(t, L, band_of(om))
        else:
            e.offres_plan(t, L)
        assert e.offres_interpolator() == k and not e.offres_live
        if k == "linear":
            with pytest.raises(_lib.PnPError, match="no least-squares"):
                e.offres_ls_coeffs()
        for a, b in zip(_three(e, h, w, J, n, om, P), own[k]):
            assert _same(a, b), k
        assert e.offres_live
    x, y, wgt = TO._data(n, h, w, P["m"], seed=3)
    e.offres_plan_ls(t, L, band_of(om))                                             # drops the live stage built on the linear plan
    assert not e.offres_live and e.offres_interpolator() == "ls"
    with pytest.raises(_lib.PnPError, match="not in off-resonance mode"):
        e.offres_cg_residual()
    e.set_kspace_offres(c64(y), f32(om[:n]), None, cg_iters=2)
    e.offres_plan_ls(t, L + 1, band_of(om))                                         # ... and one built on a least-squares plan
    assert not e.offres_live and e.offres_segments == L + 1
    bad = t.copy()
    bad[5] = float("inf")
    for call, what in ((lambda: e.offres_plan_ls(bad, 4, 600.0), "not finite"), (lambda: e.offres_plan_ls(np.full_like(t, 1e-3), 2, 600.0), "positive span"),
                       (lambda: e.offres_plan_ls(t, 4, float("nan")), "omega_max")):
        with pytest.raises(_lib.PnPError, match=what):
            call()
    assert e.offres_segments == L + 1 and e.offres_interpolator() == "ls"           # a refused plan call leaves the plan as it was
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=J)                            # a new NUFFT plan drops the plan
    assert e.offres_interpolator() is None and e.offres_segments == 0
    with pytest.raises(_lib.PnPError):
        e.offres_ls_coeffs()
    fresh = _engine(n, h, w)
    rc = fresh.lib.pnp_offres_plan_ls(fresh._h, t.ctypes.data, 4, 600.0, 0)
    assert rc == -3 and b"no NUFFT plan" in fresh.lib.pnp_last_error()


def test_the_new_calls_between_two_steps_of_an_episode_of_another_kind_change_nothing():
    traj, t, P, om = setup(TO.H_H, TO.H_W, "spiral", 6)
    for kind in TO.OTHERS:
        ref = TO._Episode(TO._handle(), kind, TO.H_N, TO.H_H, TO.H_W, 1)
        itr = ref.reset()
        ref.step(itr, 0); ref.step(itr, 1)
        e = TO._handle()
        ep = TO._Episode(e, kind, TO.H_N, TO.H_H, TO.H_W, 1)
        it = ep.reset()
        ep.step(it, 0)
        assert e.offres_interpolator() == "linear"
        e.offres_plan_ls(t, 5, band_of(om))
        assert e.offres_interpolator() == "ls" and e.offres_ls_coeffs().shape == (5, P["m"])
        ep.step(it, 1)
        for name, p, q in zip("xzud", ep.state(it), ref.state(itr)):
            assert _same(p, q), (kind, name)


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,J,L,n,naive", ((80, 64, "spiral", 4, 3, 2, 0), (32, 32, "spiral", 6, 10, 2, 0), (16, 16, "radial", 6, 32, 3, 1)))
def test_every_caller_owned_buffer_keeps_its_guard_bands(h, w, kind, J, L, n, naive, monkeypatch):
    traj, t, P, om = setup(h, w, kind, J)
    m = P["m"]
    e = planned(n, h, w, kind, J, 1, monkeypatch=monkeypatch, naive=naive)
    lib, s = e.lib, e._stream()
    # the two host buffers of the new entry points: the times and the coefficient table, between bands of a sentinel
    pad = 64
    th = np.full(m + 2 * pad, 12345.678)
    th[pad:pad + m] = t
    rc = lib.pnp_offres_plan_ls(e._h, th[pad:].ctypes.data, L, band_of(om), 0)
    assert rc == 0 and (th[:pad] == 12345.678).all() and (th[pad + m:] == 12345.678).all() and np.array_equal(th[pad:pad + m], t)
    ch = np.full(L * m + 2 * pad, -77.0, dtype=np.float32)
    rc = lib.pnp_offres_ls_coeffs(e._h, ch[pad:].ctypes.data)
    assert rc == 0 and (ch[:pad] == -77.0).all() and (ch[pad + L * m:] == -77.0).all() and np.array_equal(ch[pad:pad + L * m].reshape(L, m), e.offres_ls_coeffs())
    assert lib.pnp_offres_interpolator(e._h) == 2
    x, y, wgt = TO._data(n, h, w, m, seed=1)
    for map_n, omega in ((1, om[0]), (n, om[:n])):
        od = TO.g_f32(omega)
        maps = GB.guarded((map_n, L, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"maps": maps}, inputs={"omega": od}):
            _lib.check(lib.pnp_offres_maps(e._h, od.data_ptr(), map_n, maps.data_ptr(), s), "pnp_offres_maps")
        for batch in (1, n):
            img, smp, wd = TO.g_c64(x[:batch]), TO.g_c64(y[:batch]), TO.g_f32(wgt)
            out_s, out_i = GB.guarded((batch, m), torch.complex64, DEV), GB.guarded((batch, h, w), torch.complex64, DEV)
            with GB.watch(outputs={"samples": out_s}, inputs={"img": img, "maps": maps}):
                _lib.check(lib.pnp_offres_forward(e._h, img.data_ptr(), maps.data_ptr(), map_n, batch, out_s.data_ptr(), s), "pnp_offres_forward")
            with GB.watch(outputs={"img": out_i}, inputs={"samples": smp, "weights": wd, "maps": maps}):
                _lib.check(lib.pnp_offres_adjoint(e._h, smp.data_ptr(), wd.data_ptr(), maps.data_ptr(), map_n, batch, out_i.data_ptr(), s),
                           "pnp_offres_adjoint")
            assert torch.isfinite(torch.view_as_real(out_s)).all() and torch.isfinite(torch.view_as_real(out_i)).all()
    assert sorted(_lib.SIGNATURES_OFFRES_LS) == ["pnp_offres_interpolator", "pnp_offres_ls_coeffs", "pnp_offres_plan_ls"]
