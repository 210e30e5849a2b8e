"""The Toeplitz form of the off-resonance normal operator on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against
tests/offres_tz_ref.py.  The shapes are tests/offres_tz_cases.py's: the smallest at which each piece can go wrong.  Every figure is printed
before it is asserted.  No bound here is measured on the device.

BOUNDS.
  Spectra, against the float64 direct Dirichlet sums with the plan's stored coefficients: 2^-24 |K| + M 2^-52 sum_m |u| |D_H| |D_W| / (H W)
  per entry - the one rounding to float32 plus the rounding of an M-term float64 sum, the bound DESIGN.md states for the plain spectrum.
  L = 1: the bits of pnp_toeplitz_spectrum for the same weights.
  Application, each form, against the float64 FFT form on the float64 spectra and the device's own segment maps: relative l2 within ten
  times the float32 restatement's relative l2 error at that case (the rule of tests/test_gpu_toeplitz.py), computed here from
  offres_tz_ref.apply_f32.  Where the dense operator fits (cases A - E) the float64 FFT form is itself held to it at 1e-12 on the host.
  Against the gridding form (pnp_offres_adjoint of pnp_offres_forward): both model the same operator, the gridding pair within the NUFFT
  model error tests/test_gpu_offres.py asserts per operator for that width and grid ratio, 1e-6 + 2 x the host figure, times max sum_l |b_l|
  (tests/test_gpu_offres_mc.py); the normal operator is two of them, so twice that, relative l2.
  Slice blocks, the batch, shared against per-slice maps, coil blocks: the bits, within a form.
  Stage: float64 CG on the Toeplitz operator, relative to max |z|: the tolerances the off-resonance stage tests assert - ten times the
  float32 restatement of the CG at mu = 0.3, K = 4 (1.0e-5 for the maximum), for the multi-coil case scaled by (||A^H W A|| + 0.3) of this
  operator over the single-coil linear stage's, as tests/test_gpu_offres_mc.py scales them; the DC column's bound is that file's.
  End to end: within 0.01 dB of the float64 restatement run the same way."""
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
import offres_mc_ref as MR  # noqa: E402
import offres_ref as OR  # noqa: E402
import offres_tz_cases as ZC  # noqa: E402
import offres_tz_ref as Z  # noqa: E402
import test_gpu_offres as TO  # noqa: E402
import test_gpu_offres_ls as TL  # noqa: E402
import test_gpu_offres_mc as TM  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = TO.DEV
U = TO.U
c64, f32, g_c64, g_f32, _np, _same = TO.c64, TO.f32, TO.g_c64, TO.g_f32, TO._np, TO._same
ENV = ("PNP_OFFRES_TZ_NAIVE", "PNP_OFFRES_TZ_SLICE_BLOCK", "PNP_OFFRES_MC_COIL_BLOCK")
band_of = TM.band_of


def _engine(n, h, w, monkeypatch=None, naive=None, slice_block=None, coil_block=None):
    from dt4image_restoration_amd.engine import PnPEngine
    if monkeypatch is not None:
        for name, v in zip(ENV, (naive, slice_block, coil_block)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(int(v)))
    return PnPEngine(n, h, w, device=0, denoiser=False)


_SETUP = {}


def setup(name):
    """dict(c, traj, t, P, om, S, x, y, wgt), computed once per case"""
    if name not in _SETUP:
        c = ZC.CASES[name]
        traj, t = MR.case_traj(c)
        P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
        x, y, wgt = MR.case_data(c, P["m"], seed=ord(name))
        _SETUP[name] = dict(c=c, traj=traj, t=t, P=P, om=MR.case_omega(c), S=MR.case_sens(c), x=x, y=y, wgt=wgt)
    return _SETUP[name]


def planned(name, n=None, spectra=True, **env):
    s = setup(name)
    c = s["c"]
    e = _engine(c["n"] if n is None else n, c["h"], c["w"], **env)
    e.nufft_plan(s["traj"], grid=c["grid"], width=c["J"])
    if c["plan"] == "ls":
        e.offres_plan_ls(s["t"], c["L"], band_of(s["om"]))
    else:
        e.offres_plan(s["t"], c["L"])
    if spectra:
        e.offres_tz_plan(None if s["wgt"] is None else f32(s["wgt"]))
    return e


def coefficients(e, s):
    """B [L, M] float64: the numbers the device multiplies with"""
    if s["c"]["plan"] == "ls":
        return e.offres_ls_coeffs().astype(np.float64)
    return OR.weights(OR.plan(s["t"], s["c"]["L"]))


def forms(c):
    """(name, PNP_OFFRES_TZ_NAIVE) of the forms the case can run: a mixed-radix padded side has the composed form only"""
    fused = _lib.toeplitz_size_error("f", c["h"], c["w"]) is None and all((2 * v) & (2 * v - 1) == 0 for v in (c["h"], c["w"]))
    return (("fused", None), ("composed", 1)) if fused else (("composed", None),)


_REF = {}


def reference(name, e):
    """the float64 side of a case, once: B, the device's maps E, the float64 spectra and their full matrix"""
    if name not in _REF:
        s = setup(name)
        c = s["c"]
        B = coefficients(e, s)
        E = _np(e.offres_maps(f32(s["om"])))
        K = Z.spectra(s["traj"], c["h"], c["w"], B, c["plan"], s["wgt"])
        _REF[name] = dict(B=B, E=E, K=K, Kf=Z.full_matrix(K, c["plan"], c["L"]))
    return _REF[name]


# ---- 1. the spectra ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ZC.CASES))
def test_the_spectra_against_float64_in_the_headers_pair_order(name):
    s = setup(name)
    c = s["c"]
    h, w, L = c["h"], c["w"], c["L"]
    assert planned(name, spectra=False).offres_tz_spectra == 0
    e = planned(name)
    r = reference(name, e)
    P = len(Z.pairs(c["plan"], L))
    assert e.offres_tz_planned and not e.offres_tz_live and e.offres_tz_spectra == P == _lib.offres_tz_pairs(c["plan"], L)
    got = e.offres_tz_spectrum()
    assert tuple(got.shape) == (P, 2 * h, 2 * w) and got.dtype == torch.float32
    bound = U * np.abs(r["K"]) + Z.spectra_bound(s["traj"], h, w, r["B"], c["plan"], s["wgt"])
    err = np.abs(_np(got) - r["K"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"case {name} ({h} x {w}, L = {L} {c['plan']}, P = {P}, M = {s['P']['m']}): spectra worst |err| / bound {worst:.3f}, max |err| {err.max():.3e}, "
          f"max |K| {np.abs(r['K']).max():.3e}")
    assert worst <= 1.0
    # the bits depend on (trajectory, times plan, weights, H, W) only: another handle, another batch size
    assert _same(planned(name, n=c["n"] + 1).offres_tz_spectrum(), got)
    # a wrong pair order or an H / W swap moves whole planes: every stored spectrum is nearer to its own reference than to any other pair's
    for p in range(P):
        d = [float(np.abs(_np(got[p]) - r["K"][q]).max()) for q in range(P)]
        assert d[p] == min(d), (p, d)


def test_one_segment_has_the_bits_of_the_plain_toeplitz_spectrum():
    s = setup("A")
    m = s["P"]["m"]
    e = planned("A")
    for wgt in (None, f32((0.25 + np.arange(m) % 11 / 8.0).astype(np.float32))):
        e.offres_tz_plan(wgt)
        e.toeplitz_plan(wgt)
        assert e.offres_tz_spectra == 1
        assert torch.equal(e.offres_tz_spectrum()[0], e.toeplitz_spectrum())
        assert _same(e.offres_tz_spectrum()[0], e.toeplitz_spectrum())


# ---- 2. the application, both forms, against float64 ------------------------------------------------------------------------------------------

def model_tol(c):
    return TM.model_tol(c)


@pytest.mark.parametrize("name", sorted(ZC.CASES))
def test_the_application_in_each_form_against_float64_and_the_gridding_form(name, monkeypatch):
    s = setup(name)
    c = s["c"]
    n, h, w, C = c["n"], c["h"], c["w"], c["C"]
    x = s["x"]
    wd = None if s["wgt"] is None else f32(s["wgt"])
    for form, naive in forms(c):
        e = planned(name, monkeypatch=monkeypatch, naive=naive)
        r = reference(name, e)
        maps = e.offres_maps(f32(s["om"]))
        got = _np(e.offres_tz_apply(c64(x), maps))
        want = Z.apply(r["Kf"], r["E"], x)
        f32err = float(np.linalg.norm(Z.apply_f32(r["Kf"], r["E"], x) - want) / np.linalg.norm(want))
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        grid = _np(e.offres_adjoint(e.offres_forward(c64(x), maps), maps, wd))
        sab = float(np.abs(r["B"]).sum(axis=0).max())
        gtol = 2.0 * model_tol(c) * sab
        grel = float(np.linalg.norm(got - grid) / np.linalg.norm(grid))
        print(f"case {name} {form}: rel l2 against float64 {rel:.3e} (float32 restatement {f32err:.3e}, tolerance {10 * f32err:.3e}); against the "
              f"gridding form {grel:.3e} (tolerance {gtol:.3e}, max sum |b| {sab:.2f})")
        assert rel <= 10.0 * f32err
        assert grel <= gtol
        if c["dense"]:
            dense = Z.dense_normal(s["traj"], r["B"], r["E"], x, s["wgt"])
            dr = float(np.linalg.norm(got - dense) / np.linalg.norm(dense))
            print(f"        against the dense A^H W A: {dr:.3e}")
            assert dr <= 10.0 * f32err + 1e-12
        if C > 1:
            sd = c64(s["S"])
            gm = _np(e.offres_tz_apply_mc(c64(x), maps, sd))
            wm = Z.apply_mc(r["Kf"], r["E"], s["S"], x)
            fm = float(np.linalg.norm(Z.apply_mc_f32(r["Kf"], r["E"], s["S"], x) - wm) / np.linalg.norm(wm))
            rm = float(np.linalg.norm(gm - wm) / np.linalg.norm(wm))
            gg = _np(e.offres_adjoint_mc(e.offres_forward_mc(c64(x), maps, sd), maps, sd, wd))
            gr = float(np.linalg.norm(gm - gg) / np.linalg.norm(gg))
            print(f"        {C} coils: rel l2 against float64 {rm:.3e} (float32 restatement {fm:.3e}); against the gridding form {gr:.3e}")
            assert rm <= 10.0 * fm and gr <= gtol
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---- 3. the bits within a form -------------------------------------------------------------------------------------------------------------------

def _run(e, s, sl=None, S=None, om=None, steps=2):
    """the application(s), the normal operator and the iterate after `steps` TV steps for the slices `sl` of the case's data"""
    c = s["c"]
    h, w = c["h"], c["w"]
    sl = slice(0, c["n"]) if sl is None else sl
    cnt = sl.stop - sl.start
    S = s["S"] if S is None else S
    om = s["om"] if om is None else om
    od = f32(om)
    maps = e.offres_maps(od)
    a = e.offres_tz_apply(c64(s["x"][sl]), maps)
    mu = f32(np.array([0.3, 0.05, 0.6], dtype=np.float32)[sl])
    x0 = c64(s["x"][sl], (cnt, 1, h, w))
    wd = None if s["wgt"] is None else f32(s["wgt"])
    if c["C"] > 1:
        sd = c64(S)
        b = e.offres_tz_apply_mc(c64(s["x"][sl]), maps, sd)
        xs, zs, us = e.reset_offres_mc_tz(x0, c64(s["y"][sl]), sd, od, wd, cg_iters=3)
        q = e.offres_mc_normal(x0, mu)
    else:
        b = a
        xs, zs, us = e.reset_offres_tz(x0, c64(s["y"][sl, 0]), od, wd, cg_iters=3)
        q = e.offres_normal(x0, mu)
    assert e.offres_tz_live
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    for _ in range(steps):
        e.step(xs, zs, us, mu, f32(np.full(cnt, 0.05, dtype=np.float32)))
    return a, b, q, xs, zs, us


NAMES = "apply apply_mc normal x z u".split()


@pytest.mark.parametrize("name", ("B", "C", "E"))
def test_slice_blocks_the_batch_shared_maps_and_coil_blocks_change_no_bit(name, monkeypatch):
    s = setup(name)
    c = s["c"]
    n = c["n"]
    for form, naive in forms(c):
        ref = _run(planned(name, monkeypatch=monkeypatch, naive=naive), s)
        assert all(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all() and bool(v.abs().max() > 0) for v in ref)
        envs = [dict(slice_block=k) for k in ZC.SLICE_BLOCKS] + [dict(slice_block=2)]
        if c["C"] > 1:
            envs += [dict(coil_block=k) for k in ZC.COIL_BLOCKS] + [dict(coil_block=2, slice_block=1)]
        for env in envs:
            got = _run(planned(name, monkeypatch=monkeypatch, naive=naive, **env), s)
            for nm, a, b in zip(NAMES, ref, got):
                assert torch.equal(a, b), (form, nm, env)
                assert _same(a, b), (form, nm, env)
        for k in ENV[1:]:
            monkeypatch.delenv(k, raising=False)
        # a slice alone, in a handle of one slice
        e1 = planned(name, n=1, monkeypatch=monkeypatch, naive=naive)
        for j in range(n):
            S = s["S"] if s["S"].ndim == 3 else s["S"][j:j + 1]
            om = s["om"] if s["om"].ndim == 2 else s["om"][j:j + 1]
            alone = _run(e1, s, sl=slice(j, j + 1), S=S, om=om)
            for nm, a, b in zip(NAMES, ref, alone):
                assert _same(a[j:j + 1], b), (form, nm, j)
        # shared maps against the same values given per slice (the multi-coil case then takes its coils one at a time)
        if s["om"].ndim == 2:
            S = np.ascontiguousarray(np.broadcast_to(s["S"], (n,) + s["S"].shape[-3:]))
            om = np.ascontiguousarray(np.broadcast_to(s["om"], (n,) + s["om"].shape[-2:]))
            stacked = _run(planned(name, monkeypatch=monkeypatch, naive=naive), s, S=S, om=om)
            for nm, a, b in zip(NAMES, ref, stacked):
                assert _same(a, b), (form, nm)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---- 4. the stage ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("C", "E"))
def test_the_stage_step_composition_cg_dc_stopped_slices_snapshots_and_workspace(name):
    """pnp_offres_normal / pnp_offres_mc_normal, the CG residual and the stage under pnp_step / pnp_prox_dual / pnp_residuals while a stage
    installed by pnp_set_kspace_offres_tz / pnp_set_kspace_offres_mc_tz is live"""
    s = setup(name)
    c, P = s["c"], s["P"]
    n, h, w, C, L, K = c["n"], c["h"], c["w"], c["C"], c["L"], 4
    mc = C > 1
    e = planned(name, spectra=False)
    B = coefficients(e, s)
    sab = float(np.abs(B).sum(axis=0).max())
    od, sd = f32(s["om"]), c64(s["S"])
    maps = e.offres_maps(od)
    E = _np(maps)
    rng = np.random.default_rng(277)
    xr = rng.random((n, h, w)).astype(np.float32).astype(np.float64)
    z0 = TO._rt(xr + 0.05 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    u0 = TO._rt(0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    wgt = D.pipe(P, 30)[0].astype(np.float32)
    m = P["m"]
    S = s["S"] if mc else np.ones((1, h, w), dtype=np.complex128)
    ys = TO._rt(MR.model_forward(P, B, E, S, xr.astype(np.complex128)) + 0.02 * (rng.standard_normal((n, C, m)) + 1j * rng.standard_normal((n, C, m))))
    scale = 1.0
    if mc:     # the condition-number factor of tests/test_gpu_offres_mc.py: this operator against the single-coil linear stage at L = 3
        Q3 = OR.plan(s["t"], 3)
        om0 = (s["om"] if s["om"].ndim == 2 else s["om"][0]).astype(np.float64)
        E3 = OR.maps(om0[None], Q3)
        s_lin = TL._norm_of(lambda p: OR.model_forward(P, Q3, E3, p), lambda q: OR.model_adjoint(P, Q3, E3, q, wgt), h, w)
        s_mc = MR.op_norm(P, B, E if E.ndim == 3 else E[0], S if S.ndim == 3 else S[0], wgt)
        scale = max(1.0, (s_mc + 0.3) / (s_lin + 0.3))
        print(f"case {name}: ||A^H W A||: {s_lin:.3f} single-coil linear L = 3, {s_mc:.3f} here: the CG tolerances are scaled by {scale:.3f}")
    Kf = Z.full_matrix(Z.spectra(s["traj"], h, w, B, c["plan"], wgt), c["plan"], L)
    mu = np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    wd = f32(wgt)
    yd = c64(ys) if mc else c64(ys[:, 0])

    def install(eng, reset_from=None):
        if mc:
            return eng.set_kspace_offres_mc_tz(yd, sd, od, wd, cg_iters=K)
        return eng.set_kspace_offres_tz(yd, od, wd, cg_iters=K)

    ws0 = e.workspace_bytes
    e.offres_tz_plan(wd)
    ws_plan = e.workspace_bytes
    P_pairs = e.offres_tz_spectra
    assert ws_plan - ws0 >= 16 * P_pairs * h * w + 4 * m + 16 * m                    # the spectra, the weights copy, the trajectory (and more)
    install(e)
    ws1 = e.workspace_bytes
    assert e.offres_tz_live and not e.toeplitz_live and ws1 > ws_plan
    assert (e.offres_mc_coils == C and not e.offres_live) if mc else (e.offres_live and e.offres_mc_coils == 0)
    cgres = e.offres_mc_cg_residual if mc else e.offres_cg_residual
    normal = e.offres_mc_normal if mc else e.offres_normal
    assert not cgres().any()
    install(e)                                                                      # nothing left to grow; the spectra are re-used
    assert e.workspace_bytes == ws1
    pd = c64(u0, (n, 1, h, w))
    q = _np(normal(pd, f32(mu)))[:, 0]
    comp = _np(e.offres_tz_apply_mc(pd, maps, sd) if mc else e.offres_tz_apply(pd, maps))
    exact = comp + mu64[:, None, None] * u0
    off = float(max((np.abs(q.real - exact.real) / np.maximum(np.abs(exact.real), 1e-30)).max(),
                    (np.abs(q.imag - exact.imag) / np.maximum(np.abs(exact.imag), 1e-30)).max()))
    print(f"the stage's normal operator against fma(mu, p, apply(p)): worst relative distance {off:.3e} (one rounding: {U:.3e})")
    assert off <= U * (1 + 1e-6)
    grid = _np(e.offres_adjoint_mc(e.offres_forward_mc(pd, maps, sd), maps, sd, wd) if mc else e.offres_adjoint(e.offres_forward(pd, maps), maps, wd))
    assert float(np.linalg.norm(comp - grid) / np.linalg.norm(grid)) <= 2.0 * model_tol(c) * sab      # the live operator is the Toeplitz one, near the gridding one
    aty = MR.model_adjoint(P, B, E, S, ys, wgt)                                     # aty stays on the gridding pair
    Sref = s["S"] if mc else None
    xs, zs, us = f32(xr, (n, 1, h, w)), c64(z0, (n, 1, h, w)), c64(u0, (n, 1, h, w))
    e.prox_dual(xs, zs, us, f32(mu))
    zr, ur, rr = Z.prox_dual(Kf, E, xr, z0, u0, aty, mu64, K, Sref)
    res = cgres().cpu().numpy().astype(np.float64)
    bmax, brms, bres = (scale * TO.MARGIN * v for v in TO.F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"prox_dual K={K}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    dc = e.residuals(xs, zs, us, dc=True).cpu().numpy().astype(np.float64)[:, 5]
    dcr = MR.dc_misfit(P, B, E, S, xr, ys, wgt)                                     # the DC column stays on the gridding pair
    bdc = 1e-6 * NR.op_norm(P) * sab * math.sqrt(float(wgt.max())) * np.linalg.norm(xr.reshape(n, -1), axis=1) + 5e-7 * dcr
    print(f"dc column {dc} ref {dcr} |d| {np.abs(dc - dcr)} bound {bdc}")
    assert (np.abs(dc - dcr) <= bdc).all()
    # three steps under the TV prior: each is tv_denoise then prox_dual, bit for bit; slice 1 stopped in step 2
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = f32(np.full(n, 0.05, dtype=np.float32))
    e2 = planned(name, spectra=False)
    install(e2)                                                                     # (the binding plans the spectra for these weights)
    t_state = torch.zeros(n, dtype=torch.float32, device=DEV)
    for step in range(3):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [v.clone() for v in (xs, zs, us, t_state, cgres())]
        tact = f32(np.array([0.0, 1.0 if step == 1 else 0.0], dtype=np.float32))
        x2, z2, u2 = xs.clone(), zs.clone(), us.clone()
        xp = e2.tv_denoise(z2.real - u2.real, torch.tensor(1.0, dtype=torch.float32, device=DEV) * sig, 5)
        if step == 1:
            xp[1] = x2[1]
        e2.prox_dual(xp, z2, u2, f32(mu), tact)
        e.step(xs, zs, us, f32(mu), sig, t_action=tact, t_state=t_state)
        for nm, a, b in zip("xzu", (xs, zs, us), (xp, z2, u2)):
            assert _same(a, b), (f"step {step + 1}: {nm} of pnp_step differs from tv_denoise + pnp_prox_dual")
        zr, ur, rr = Z.prox_dual(Kf, E, _np(xs)[:, 0], zin, uin, aty, mu64, K, Sref)
        live = [0] if step == 1 else [0, 1]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:                                                               # the stopped slice keeps z, u and the CG residual bit for bit
            for nm, a, kp in zip(("x", "z", "u", "t", "cg"), (xs, zs, us, t_state, cgres()), keep):
                assert _same(a[1], kp[1]), nm
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
    # a failed install leaves the mode and the iterate untouched
    keep = [v.clone() for v in (xs, zs, us)]
    with pytest.raises(_lib.PnPError, match="cg_iters"):
        if mc:
            e.reset_offres_mc_tz(zs.clone(), yd, sd, od, wd, cg_iters=_lib.PNP_MC_MAX_CG + 1)
        else:
            e.reset_offres_tz(zs.clone(), yd, od, wd, cg_iters=_lib.PNP_MC_MAX_CG + 1)
    assert e.offres_tz_live
    for a, b in zip((xs, zs, us), keep):
        assert _same(a, b)
    e.step(xs, zs, us, f32(mu), sig)
    # the sibling installer leaves the mode; the _tz one enters it again
    if mc:
        e.set_kspace_offres_mc(yd, sd, od, wd, cg_iters=K)
    else:
        e.set_kspace_offres(yd, od, wd, cg_iters=K)
    assert not e.offres_tz_live and e.offres_tz_planned
    install(e)
    assert e.offres_tz_live


# ---- 4b. installed last, the plan calls ---------------------------------------------------------------------------------------------------------------

class _Episode(TM._Episode):
    """tests/test_gpu_offres_mc.py's episode of one stage kind, and the two new kinds "offres_tz" and "offres_mc_tz" (the handle's live plans)"""

    def __init__(self, e, kind, n, h, w, seed):
        base = {"offres_tz": "offres", "offres_mc_tz": "offres_mc"}.get(kind, kind)
        super().__init__(e, base, n, h, w, seed)
        self.kind = kind

    def reset(self):
        if self.kind == "offres_tz":
            return self.e.reset_offres_tz(self.x0, self.y, self.om, self.w, cg_iters=3)
        if self.kind == "offres_mc_tz":
            return self.e.reset_offres_mc_tz(self.x0, self.y, self.sens, self.om, self.w, cg_iters=3)
        return super().reset()

    def set_kspace(self):
        if self.kind == "offres_tz":
            return self.e.set_kspace_offres_tz(self.y, self.om, self.w, cg_iters=3)
        if self.kind == "offres_mc_tz":
            return self.e.set_kspace_offres_mc_tz(self.y, self.sens, self.om, self.w, cg_iters=3)
        return super().set_kspace()


OTHERS = TM.OTHERS + ("offres_mc",)
NEW = ("offres_tz", "offres_mc_tz")
H_N, H_H, H_W, H_L = TO.H_N, TO.H_H, TO.H_W, TO.H_L


def test_installed_last_in_both_orders_and_the_plan_calls():
    """pnp_set_kspace_offres_tz, pnp_reset_offres_tz, pnp_set_kspace_offres_mc_tz, pnp_reset_offres_mc_tz: the stage installed last runs,
    against every other installer in both orders; pnp_nufft_plan, pnp_offres_plan, pnp_offres_plan_ls and pnp_offres_tz_plan drop the stage,
    pnp_toeplitz_plan does not"""
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    for new in NEW:
        for other in OTHERS + tuple(k for k in NEW if k != new):
            for first, second in ((new, other), (other, new)):
                e = TO._handle()
                a = _Episode(e, first, H_N, H_H, H_W, 1)
                it = a.reset()
                a.step(it, 0); a.step(it, 1)
                want = a.state(it)
                e = TO._handle()                                                    # the same episode with the other stage's installers in between
                a, b = _Episode(e, first, H_N, H_H, H_W, 1), _Episode(e, second, H_N, H_H, H_W, 2)
                it = a.reset()
                assert e.offres_tz_live == (first in NEW)
                a.step(it, 0)
                itb = b.reset()
                assert e.offres_tz_live == (second in NEW) and not e.toeplitz_live == (second != "nc_tz")
                b.step(itb, 0)                                                      # the stage installed last runs
                eb = TO._handle()
                b2 = _Episode(eb, second, H_N, H_H, H_W, 2)
                itb2 = b2.reset()
                b2.step(itb2, 0)
                for nm, p, q in zip("xzud", b.state(itb), b2.state(itb2)):
                    assert _same(p, q), (first, second, nm)
                a.set_kspace()
                assert e.offres_tz_live == (first in NEW)
                a.step(it, 1)
                for nm, p, q in zip("xzud", a.state(it), want):
                    assert _same(p, q), (first, second, nm)
    # the Toeplitz stage is not the gridding stage: the same episode through the sibling installer ends elsewhere
    e, eg = TO._handle(), TO._handle()
    a, g = _Episode(e, "offres_tz", H_N, H_H, H_W, 1), _Episode(eg, "offres", H_N, H_H, H_W, 1)
    it, itg = a.reset(), g.reset()
    a.step(it, 0); g.step(itg, 0)
    assert not _same(it[1], itg[1]) and float((it[1] - itg[1]).abs().max()) <= 1e-2 * float(itg[1].abs().max())
    # the plan calls
    for new in NEW:
        e = TO._handle()
        a = _Episode(e, new, H_N, H_H, H_W, 1)
        it = a.reset()
        a.step(it, 0)
        mode = (lambda: e.offres_mc_coils == 3) if new == "offres_mc_tz" else (lambda: e.offres_live)
        assert mode() and e.offres_tz_live
        e.toeplitz_plan(a.w)                                                        # knows nothing of this stage
        assert mode() and e.offres_tz_live and not e.toeplitz_live and e.toeplitz_planned
        a.step(it, 1)
        e2 = TO._handle()
        a2 = _Episode(e2, new, H_N, H_H, H_W, 1)
        it2 = a2.reset()
        a2.step(it2, 0); a2.step(it2, 1)
        for nm, p, q in zip("xzud", a.state(it), a2.state(it2)):
            assert _same(p, q), (new, nm)
        for replan in (lambda: e.offres_tz_plan(a.w), lambda: e.offres_plan(t, H_L + 1), lambda: e.offres_plan_ls(t, H_L, TL.band_of(om)),
                       lambda: e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)):
            if e.offres_segments == 0:
                e.offres_plan(t, H_L)
            a.set_kspace()
            assert mode() and e.offres_tz_live and e.live_episode
            keep = [v.clone() for v in it]
            replan()
            assert not e.offres_tz_live and not mode() and e.live_episode == 0
            with pytest.raises(_lib.PnPError):
                a.step(it, 1)
            for v, k in zip(it, keep):
                assert _same(v, k)
        assert not e.offres_tz_planned
        with pytest.raises(_lib.PnPError, match="no off-resonance plan"):
            a.set_kspace()
        e.offres_plan(t, H_L)
        with pytest.raises(_lib.PnPError, match=r"no Toeplitz off-resonance spectra \(pnp_offres_tz_plan\)"):
            _lib.check(e.lib.pnp_set_kspace_offres_tz(e._h, a.y.data_ptr(), a.om.data_ptr(), H_N, 3, None), "pnp_set_kspace_offres_tz")
        a.set_kspace()                                                              # the binding plans the spectra again
        assert e.offres_tz_planned and e.offres_tz_live


# ---- 5. non-interference ----------------------------------------------------------------------------------------------------------------------------

def test_the_intruders_between_two_steps_of_the_other_kinds_change_nothing():
    """pnp_offres_tz_spectrum, pnp_offres_tz_apply, pnp_offres_tz_apply_mc between two steps of a live episode of every stage kind"""
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    rng = np.random.default_rng(79)
    x = TO._rt(rng.standard_normal((H_N, H_H, H_W)) + 1j * rng.standard_normal((H_N, H_H, H_W)))
    for kind in OTHERS + NEW:
        ref = _Episode(TO._handle(), kind, H_N, H_H, H_W, 1)
        itr = ref.reset()
        ref.step(itr, 0); ref.step(itr, 1)
        e = TO._handle()
        ep = _Episode(e, kind, H_N, H_H, H_W, 1)
        if kind not in NEW:
            e.offres_tz_plan(ep.w)                                                  # spectra for the intruders, before the episode starts
        it = ep.reset()
        ep.step(it, 0)
        live, ws = e.offres_tz_live, e.workspace_bytes
        e.offres_tz_spectrum()
        for C, omega in ((2, f32(om[2])), (9, f32(om[:H_N] * 3.0))):                # shared and per-slice maps, fewer and more coils than the episode's 3
            maps = e.offres_maps(omega)
            e.offres_tz_apply(c64(x), maps)
            e.offres_tz_apply(c64(x[:1]), maps)
            e.offres_tz_apply_mc(c64(x), maps, c64(synthetic.coil_maps(C, H_H, H_W)))
        assert e.offres_tz_live == live and e.workspace_bytes >= ws
        ep.step(it, 1)
        for nm, p, q in zip("xzud", ep.state(it), ref.state(itr)):
            assert _same(p, q), (kind, nm)


def test_the_existing_intruders_between_two_steps_of_the_new_kinds_change_nothing():
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    m = P["m"]
    rng = np.random.default_rng(80)
    x = TO._rt(rng.standard_normal((H_N, H_H, H_W)) + 1j * rng.standard_normal((H_N, H_H, H_W)))
    y = TO._rt(rng.standard_normal((H_N, 9, m)) + 1j * rng.standard_normal((H_N, 9, m)))
    for kind in NEW:
        ref = _Episode(TO._handle(), kind, H_N, H_H, H_W, 1)
        itr = ref.reset()
        ref.step(itr, 0); ref.step(itr, 1)
        e = TO._handle()
        ep = _Episode(e, kind, H_N, H_H, H_W, 1)
        it = ep.reset()
        ep.step(it, 0)
        maps = e.offres_maps(f32(om[:H_N] * 2.0))
        sens = c64(synthetic.coil_maps(9, H_H, H_W))
        e.offres_forward(c64(x), maps)
        e.offres_adjoint(c64(y[:, 0]), maps, None)
        e.offres_forward_mc(c64(x), maps, sens)
        e.offres_adjoint_mc(c64(y), maps, sens, None)
        e.nufft_forward_mc(c64(x), sens)
        e.toeplitz_plan(None)
        e.toeplitz_apply(c64(x))
        e.toeplitz_apply_mc(c64(x), sens)
        e.nufft_dcf(iters=5)
        e.acquire_offres(f32(np.abs(x), (H_N, 1, H_H, H_W)), f32(om[0]), 0.01, 3)
        assert e.offres_tz_live
        ep.step(it, 1)
        for nm, p, q in zip("xzud", ep.state(it), ref.state(itr)):
            assert _same(p, q), (kind, nm)


def test_handle_dependent_argument_errors_leave_the_outputs_untouched():
    h, w, n = H_H, H_W, H_N
    traj, t, P, om = TO.setup(h, w, "spiral", 6)
    e = TO._engine(n, h, w)
    lib = e.lib
    C = 3
    maps = torch.zeros((1, 3, h, w), dtype=torch.complex64, device=DEV)
    sens = c64(synthetic.coil_maps(C, h, w))
    out = torch.full((n, C, P["m"]), 7.0, dtype=torch.complex64, device=DEV)
    img = torch.full((n, h, w), 7.0, dtype=torch.complex64, device=DEV)
    spec = torch.full((5, 2 * h, 2 * w), 7.0, dtype=torch.float32, device=DEV)
    od = f32(om[0])

    def refused(rc, what, code):
        assert rc == code and what in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    plan = lambda: lib.pnp_offres_tz_plan(e._h, None, 0, None)                                                                         # noqa: E731
    app = lambda map_n=1, batch=n: lib.pnp_offres_tz_apply(e._h, out.data_ptr(), maps.data_ptr(), map_n, batch, img.data_ptr(), None)   # noqa: E731
    amc = lambda map_n=1, sens_n=1, batch=n: lib.pnp_offres_tz_apply_mc(e._h, out.data_ptr(), maps.data_ptr(), map_n, sens.data_ptr(), sens_n, C, batch,  # noqa: E731
                                                                        img.data_ptr(), None)
    ins = lambda map_n=1: lib.pnp_set_kspace_offres_tz(e._h, out.data_ptr(), od.data_ptr(), map_n, 4, None)                             # noqa: E731
    imc = lambda map_n=1, sens_n=1: lib.pnp_set_kspace_offres_mc_tz(e._h, out.data_ptr(), sens.data_ptr(), C, sens_n, od.data_ptr(), map_n, 4, None)  # noqa: E731
    spc = lambda: lib.pnp_offres_tz_spectrum(e._h, spec.data_ptr(), None)                                                               # noqa: E731
    for call in (plan, app, amc, ins, imc, spc):
        refused(call(), b"no NUFFT plan", -3)
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)
    for call in (plan, app, amc, ins, imc, spc):
        refused(call(), b"no off-resonance plan", -3)
    e.offres_plan(t, 3)
    for call in (app, amc, ins, imc, spc):
        refused(call(), b"no Toeplitz off-resonance spectra (pnp_offres_tz_plan)", -3)
    assert plan() == 0 and e.offres_tz_spectra == 5
    for call in (app, amc, ins, imc):
        refused(call(map_n=3), b"map_n must be 1 or n=2", -1)
    for call in (amc, imc):
        refused(call(sens_n=3), b"sens_n must be 1 or n=2", -1)
    refused(app(batch=n + 1), b"batch must be 1..n=2", -1)
    refused(amc(batch=n + 1), b"batch must be 1..n=2", -1)
    # P above the limit: 17 segments least squares need 153 spectra; the earlier spectra went with the linear plan
    e.offres_plan_ls(t, 17, TL.band_of(om))
    assert not e.offres_tz_planned
    refused(plan(), b"17 segments under a least-squares plan need 153 spectra, more than the limit of 136", -1)
    assert not e.offres_tz_planned and e.offres_tz_spectra == 0
    e.offres_plan_ls(t, 16, TL.band_of(om))
    assert plan() == 0 and e.offres_tz_spectra == 136
    e.offres_plan(t, 32)
    assert plan() == 0 and e.offres_tz_spectra == 63
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == 7.0).all()) and bool((spec == 7.0).all()) and not e.offres_tz_live
    # a side above 512, in the words of pnp_toeplitz_plan's refusal
    big = TO._engine(1, 16, 640)
    tb = NR.radial(16, 640, 4, readout=16)
    big.nufft_plan(tb, grid=(32, 800), width=4)
    big.offres_plan(np.arange(tb.shape[0]) * 1e-5, 2)
    rc = big.lib.pnp_offres_tz_plan(big._h, None, 0, None)
    assert rc == -1 and _lib.toeplitz_size_error("pnp_offres_tz_plan", 16, 640).encode() == big.lib.pnp_last_error(), big.lib.pnp_last_error()
    assert lib.pnp_offres_tz_planned(None) == 0 and lib.pnp_offres_tz_live(None) == 0 and lib.pnp_offres_tz_spectra(None) == 0


# ---- 6. guard bands -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,naive", (("B", None), ("B", 1), ("D", None), ("E", None), ("E", 1)))
def test_every_caller_owned_buffer_keeps_its_guard_bands(name, naive, monkeypatch):
    s = setup(name)
    c = s["c"]
    n, h, w, C, L, m = c["n"], c["h"], c["w"], c["C"], c["L"], s["P"]["m"]
    e = planned(name, spectra=False, monkeypatch=monkeypatch, naive=naive)
    lib, st = e.lib, e._stream()
    wgt = (0.5 + np.arange(m) % 5 / 5.0).astype(np.float32)
    S4 = np.ascontiguousarray(MR._maps4(s["S"], n))
    om3 = np.ascontiguousarray(np.broadcast_to(s["om"], (n, h, w)))
    wd = g_f32(wgt)
    with GB.watch(outputs={}, inputs={"weights": wd}):
        _lib.check(lib.pnp_offres_tz_plan(e._h, wd.data_ptr(), 0, st), "pnp_offres_tz_plan")
    P = e.offres_tz_spectra
    spec = GB.guarded((P, 2 * h, 2 * w), torch.float32, DEV)
    with GB.watch(outputs={"out": spec}, inputs={}):
        _lib.check(lib.pnp_offres_tz_spectrum(e._h, spec.data_ptr(), st), "pnp_offres_tz_spectrum")
    for sens_n, map_n in ((1, 1), (n, n)):
        sd, od = g_c64(S4[0] if sens_n == 1 else S4), g_f32(om3[0] if map_n == 1 else om3)
        maps = GB.guarded((map_n, L, h, w), torch.complex64, DEV)
        _lib.check(lib.pnp_offres_maps(e._h, od.data_ptr(), map_n, maps.data_ptr(), st), "pnp_offres_maps")
        for batch in (1, n):
            img = g_c64(s["x"][:batch])
            out = GB.guarded((batch, h, w), torch.complex64, DEV)
            with GB.watch(outputs={"out": out}, inputs={"img": img, "maps": maps}):
                _lib.check(lib.pnp_offres_tz_apply(e._h, img.data_ptr(), maps.data_ptr(), map_n, batch, out.data_ptr(), st), "pnp_offres_tz_apply")
            with GB.watch(outputs={"out": out}, inputs={"img": img, "maps": maps, "sens": sd}):
                _lib.check(lib.pnp_offres_tz_apply_mc(e._h, img.data_ptr(), maps.data_ptr(), map_n, sd.data_ptr(), sens_n, C, batch, out.data_ptr(), st),
                           "pnp_offres_tz_apply_mc")
        yo = g_c64(s["y"])
        y1 = g_c64(s["y"][:, 0])
        xo = g_c64(s["x"], (n, 1, h, w))
        mu = g_f32(np.array([0.3, 0.05, 0.6], dtype=np.float32)[:n])
        for coils in (False, True):
            xs, zs, us = GB.guarded((n, 1, h, w), torch.float32, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
            if coils:
                with GB.watch(outputs={"x": xs, "z": zs, "u": us}, inputs={"x0": xo, "y": yo, "sens": sd, "omega": od}):
                    _lib.check(lib.pnp_reset_offres_mc_tz(e._h, xo.data_ptr(), yo.data_ptr(), sd.data_ptr(), C, sens_n, od.data_ptr(), map_n, 3,
                                                          xs.data_ptr(), zs.data_ptr(), us.data_ptr(), st), "pnp_reset_offres_mc_tz")
                with GB.watch(outputs={}, inputs={"y": yo, "sens": sd, "omega": od, "x": xs, "z": zs, "u": us}):
                    _lib.check(lib.pnp_set_kspace_offres_mc_tz(e._h, yo.data_ptr(), sd.data_ptr(), C, sens_n, od.data_ptr(), map_n, 3, st),
                               "pnp_set_kspace_offres_mc_tz")
                assert e.offres_mc_coils == C
            else:
                with GB.watch(outputs={"x": xs, "z": zs, "u": us}, inputs={"x0": xo, "y": y1, "omega": od}):
                    _lib.check(lib.pnp_reset_offres_tz(e._h, xo.data_ptr(), y1.data_ptr(), od.data_ptr(), map_n, 3, xs.data_ptr(), zs.data_ptr(),
                                                       us.data_ptr(), st), "pnp_reset_offres_tz")
                with GB.watch(outputs={}, inputs={"y": y1, "omega": od, "x": xs, "z": zs, "u": us}):
                    _lib.check(lib.pnp_set_kspace_offres_tz(e._h, y1.data_ptr(), od.data_ptr(), map_n, 3, st), "pnp_set_kspace_offres_tz")
                assert e.offres_live
            assert e.offres_tz_live
            q, res = GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n,), torch.float32, DEV)
            with GB.watch(outputs={"q": q}, inputs={"p": zs, "mu": mu}):
                _lib.check((lib.pnp_offres_mc_normal if coils else lib.pnp_offres_normal)(e._h, zs.data_ptr(), mu.data_ptr(), q.data_ptr(), st), "normal")
            with GB.watch(outputs={"z": zs, "u": us}, inputs={"x": xs, "mu": mu}):
                e.prox_dual(xs, zs, us, mu)
            with GB.watch(outputs={"out": res}, inputs={}):
                _lib.check((lib.pnp_offres_mc_cg_residual if coils else lib.pnp_offres_cg_residual)(e._h, res.data_ptr(), st), "cg_residual")
            assert torch.isfinite(res).all() and torch.isfinite(torch.view_as_real(q)).all()
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------------------

def _corrects(coils):
    """the fixture of tests/offres_ref.py (32 x 32 spiral, omega_max span = 3 pi, L = 8 least squares) through PnPEnv(offres_normal="toeplitz")
    and FixedScheduleSolver, beside the float64 restatement run the same way; (device dB, float64 dB, engine)"""
    from dt4image_restoration_amd import acquisition
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    c = OR.CORRECTS
    h, w, L = c["h"], c["w"], MR.CORRECTS_L
    if coils:
        traj, t, omega, gt, S, y = MR.corrects_problem()
    else:
        traj, t, omega, gt, y1, _ = OR.corrects_problem()
        S, y = None, y1[None]
    env = PnPEnv(max_episode_step=c["steps"], denoiser=TVDenoiser2D(scale=1.0, iters=c["tv_iters"]), device_type="cuda", cg_iters=c["K"],
                 nufft_width=c["J"], nufft_grid=c["grid"], offres_mc=bool(coils), offres_normal="toeplitz")
    eng = env._engine_for(1, h, w, torch.device("cuda", 0))
    dcf = acquisition.pipe_dcf(env, traj, iters=30, width=c["J"], grid=c["grid"])
    od, yd = f32(omega.astype(np.float32)), c64(y[None])
    eng.offres_plan_ls(t, L, band_of(omega))
    maps = eng.offres_maps(od)
    if coils:
        sd = c64(S)
        x0 = eng.offres_adjoint_mc(yd, maps, sd, dcf).reshape(1, 1, h, w)
    else:
        x0 = eng.offres_adjoint(yd[:, 0].contiguous(), maps, dcf).reshape(1, 1, h, w)
    mat = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(yd if coils else yd.reshape(1, 1, -1)), "ATy0": torch.view_as_real(x0),
           "gt": f32(gt.astype(np.float32), (1, 1, h, w)), "traj": torch.from_numpy(traj), "dcf": dcf, "omega": od, "times": torch.from_numpy(t),
           "segments": L, "b0_interp": "ls"}
    if coils:
        mat["sens"] = sd
    mu, sig = np.full((1, c["steps"]), c["mu"], dtype=np.float32), OR.corrects_schedule()[None]
    r = FixedScheduleSolver(env, max_iter=c["steps"], dc=True).run(mat, mu, sig)
    e = env._engine
    assert e.offres_tz_live and e.offres_tz_spectra == L * (L + 1) // 2 and e.offres_interpolator() == "ls" and not e.toeplitz_live
    got = TO._psnr(_np(r.x)[0, 0], gt)
    # float64, the same way: aty on the gridding model with the device's coefficients, maps and weights; the CG on the Toeplitz operator
    P = NR.plan(h, w, c["grid"][0], c["grid"][1], c["J"], traj)
    B, E, wgt = e.offres_ls_coeffs().astype(np.float64), _np(maps), _np(dcf)
    S1 = S if coils else np.ones((1, h, w), dtype=np.complex128)
    aty = MR.model_adjoint(P, B, E, S1, y[None], wgt)
    Kf = Z.full_matrix(Z.spectra(traj, h, w, B, "ls", wgt), "ls", L)
    return got, Z.corrects_psnr(Kf, E, aty, gt, S if coils else None), r


def test_the_correction_end_to_end_with_the_toeplitz_operator_single_coil():
    got, ref, r = _corrects(0)
    print(f"single-coil, L = 8 least squares, offres_normal='toeplitz': {got:.3f} dB (float64 restatement run the same way {ref:.3f}; the gridding stage's "
          f"recorded figure {LS.CORRECTS_LS[0]}), dc {r.dc.tolist()}")
    assert abs(got - ref) <= 0.01


def test_the_correction_end_to_end_with_the_toeplitz_operator_four_coils():
    got, ref, r = _corrects(MR.CORRECTS_COILS)
    print(f"4 coils, L = 8 least squares, offres_normal='toeplitz': {got:.3f} dB (float64 restatement run the same way {ref:.3f}; the gridding stage's "
          f"recorded figure {MR.CORRECTS_MC_PSNR[0]}), dc {r.dc.tolist()}")
    assert abs(got - ref) <= 0.01


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------------------------------

def test_cli_b0_normal_toeplitz_fixed_on_a_ground_truth_folder(tmp_path, monkeypatch):
    import contextlib
    import io
    from dt4image_restoration_amd import cli, env as envmod
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5), synthetic.phantom(64, 64, 6)]).astype(np.float32))
    engines = []
    orig = envmod.PnPEnv._engine_for

    def spy(self, *a):
        engines.append(orig(self, *a))
        return engines[-1]

    monkeypatch.setattr(envmod.PnPEnv, "_engine_for", spy)
    base = ["--block_size", "6", "--n_embeds", "9", "--gt", str(gtd), "--tasks", "4x_5", "--prior", "tv", "--seed", "3", "--traj", "spiral",
            "--interleaves", "8", "--b0", "40", "--readout-ms", "10", "--b0-interp", "ls"]

    def run(extra):
        with contextlib.redirect_stdout(io.StringIO()):
            out = cli.main(base + extra + ["fixed", "--max_iter", "10", "--dc"])
        assert len(out) == 1 and out[0]["n"] == 2
        return out[0]

    tz = run(["--b0-normal", "toeplitz"])
    assert engines and engines[-1].offres_tz_live and engines[-1].offres_live and not engines[-1].toeplitz_live
    grid = run([])
    assert not engines[-1].offres_tz_live and engines[-1].offres_live
    mc = run(["--b0-normal", "toeplitz", "--b0-coils", "4"])
    assert engines[-1].offres_tz_live and engines[-1].offres_mc_coils == 4
    print(f"cli --traj spiral --b0 40 --readout-ms 10 --b0-interp ls fixed: --b0-normal toeplitz {tz['psnr']:.3f} dB, nufft {grid['psnr']:.3f} dB; "
          f"--b0-coils 4 toeplitz {mc['psnr']:.3f} dB")
    assert abs(tz["psnr"] - grid["psnr"]) <= 0.05 and np.isfinite(mc["psnr"]) and mc["psnr_increment"] > 0.0
    with pytest.raises(SystemExit, match="17 segments under a least-squares plan need 153 spectra"):
        cli.main(base + ["--b0-normal", "toeplitz", "--b0-segments", "17", "fixed", "--max_iter", "2"])
