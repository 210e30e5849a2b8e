"""Off-resonance correction for multi-coil data on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against
tests/offres_mc_ref.py.  The shapes are tests/offres_mc_cases.py's: the smallest at which the coil-block x segment-block logic can go wrong.
Every figure is printed before it is asserted.  No bound here is measured on the device.

BOUNDS.
  Forms, blocks, batch, shared against per-slice maps: the bits.  C = 1, S = 1 against the single-coil pair: torch.equal.  Dyadic maps
  S_c = 2^-c i^c (S_c . p exact in float32): coil plane c of the forward against pnp_offres_forward on that image: torch.equal; the adjoint
  against the float64 combine of the device's own single-coil adjoints a_c: 4 C 2^-24 sum_c |S_c| |a_c| per pixel, a chain of 4 C fused
  operations.
  General maps, against the float64 model on the NUFFT plan with the device's own segment maps and the plan's coefficients: a coil plane
  is the single-coil operator on S_c . p, so per plane the forward bound of tests/test_gpu_offres.py (linear) / tests/test_gpu_offres_ls.py
  (least squares) evaluated on S_c . p, plus the three roundings of the product S_c . p through the operator:
  ||F_nu|| (sum_l max_m |b_l|) gamma(3) ||S_c . p||.  The adjoint: sum_c |S_c| (the single-coil adjoint bound on coil c's samples
  + gamma(4 C) |a_c|).  Adjointness: <A p, W q> - <p, A^H W q> on the device outputs is <df, W q> - <p, da> (the model pair is exactly
  adjoint).  Dense segmented restatement: the NUFFT's own error, relative l2 <= (1e-6 + twice the host test's model error for the width
  and grid ratio) x max sum |b|; J = 8 takes J = 6's figure (a wider kernel is no less accurate).
  Stage: the tolerances of tests/test_gpu_offres_ls.py - ten times the float32 restatement of the CG at mu = 0.3, K = 4, scaled by
  (||A^H W A|| + 0.3) of this operator over the single-coil linear stage's; the DC column's 1e-6 s sqrt(wmax) ||x|| + 5e-7 dc.
  The correction corrects: within 0.01 dB of each float64 figure of offres_mc_ref.CORRECTS_MC_PSNR; the gap: half the restatement's."""
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
import offres_mc_cases as MC  # noqa: E402
import offres_mc_ref as MR  # noqa: E402
import offres_ref as OR  # noqa: E402
import test_gpu_nufft as TN  # noqa: E402
import test_gpu_offres as TO  # noqa: E402
import test_gpu_offres_ls as TL  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = TO.DEV
U = TO.U
c64, f32, g_c64, g_f32, _np, _same, _bits, gamma = TO.c64, TO.f32, TO.g_c64, TO.g_f32, TO._np, TO._same, TO._bits, TO.gamma
ENV = ("PNP_OFFRES_MC_NAIVE", "PNP_OFFRES_MC_COIL_BLOCK", "PNP_OFFRES_SEG_BLOCK")
NAMES = "forward adjoint normal x z u".split()


def _engine(n, h, w, monkeypatch=None, naive=None, coil_block=None, seg_block=None):
    from dt4image_restoration_amd.engine import PnPEngine
    if monkeypatch is not None:
        for name, v in zip(ENV, (naive, coil_block, seg_block)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(int(v)))
    return PnPEngine(n, h, w, device=0, denoiser=False)


_SETUP = {}


def setup(name):
    """dict(case, traj, t, P, om, S, x, y, wgt), computed once per case"""
    if name not in _SETUP:
        c = MC.CASES[name]
        traj, t = MR.case_traj(c)
        P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
        x, y, wgt = MR.case_data(c, P["m"], seed=ord(name))
        _SETUP[name] = dict(c=c, traj=traj, t=t, P=P, om=MR.case_omega(c), S=MR.case_sens(c), x=x, y=y, wgt=wgt)
    return _SETUP[name]


def band_of(om):
    return float(np.abs(om).max()) * (1.0 + 1e-6)


def planned(name, n=None, **env):
    s = setup(name)
    c = s["c"]
    e = _engine(c["n"] if n is None else n, c["h"], c["w"], **env)
    e.nufft_plan(s["traj"], grid=c["grid"], width=c["J"])
    if c["plan"] == "ls":
        e.offres_plan_ls(s["t"], c["L"], band_of(s["om"]))
    else:
        e.offres_plan(s["t"], c["L"])
    return e


def coefficients(e, s):
    """B [L, M] float64: the numbers the device multiplies with"""
    if s["c"]["plan"] == "ls":
        return e.offres_ls_coeffs().astype(np.float64)
    return OR.weights(OR.plan(s["t"], s["c"]["L"]))


def _wd(wgt):
    return None if wgt is None else f32(wgt)


def _run(e, s, sl=None, S=None, om=None, steps=2):
    """forward, adjoint, normal operator and the iterate after `steps` TV steps for the slices `sl` of the case's data"""
    c = s["c"]
    h, w = c["h"], c["w"]
    sl = slice(0, c["n"]) if sl is None else sl
    cnt = sl.stop - sl.start
    S = s["S"] if S is None else S
    om = s["om"] if om is None else om
    sd, od, wd = c64(S), f32(om), _wd(s["wgt"])
    maps = e.offres_maps(od)
    f = e.offres_forward_mc(c64(s["x"][sl]), maps, sd)
    a = e.offres_adjoint_mc(c64(s["y"][sl]), maps, sd, wd)
    mu = f32(np.array([0.3, 0.05, 0.6], dtype=np.float32)[sl])
    x0 = c64(s["x"][sl], (cnt, 1, h, w))
    xs, zs, us = e.reset_offres_mc(x0, c64(s["y"][sl]), sd, od, wd, cg_iters=3)
    q = e.offres_mc_normal(x0, mu)
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    for _ in range(steps):
        e.step(xs, zs, us, mu, f32(np.full(cnt, 0.05, dtype=np.float32)))
    return f, a, q, xs, zs, us


# ---- 1. forms and blocks ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_both_forms_every_block_size_the_batch_and_shared_maps_give_the_same_bits(name, monkeypatch):
    s = setup(name)
    c = s["c"]
    n = c["n"]
    ref = _run(planned(name, monkeypatch=monkeypatch), s)
    assert all(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all() and bool(v.abs().max() > 0) for v in ref)
    assert tuple(ref[0].shape) == (n, c["C"], s["P"]["m"]) and tuple(ref[1].shape) == (n, c["h"], c["w"])
    envs = [dict(naive=1), dict(naive=0)]
    envs += [dict(naive=0, coil_block=k) for k in MC.COIL_BLOCKS] + [dict(naive=0, seg_block=k) for k in MC.SEG_BLOCKS]
    envs += [dict(naive=1, coil_block=2, seg_block=3), dict(coil_block=1, seg_block=1)]
    for env in envs:
        got = _run(planned(name, monkeypatch=monkeypatch, **env), s)
        for nm, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), (nm, env)
            assert _same(a, b), (nm, env)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    # a slice alone, in a handle of one slice
    e1 = planned(name, n=1)
    for j in range(n if n > 1 else 0):
        S = s["S"] if s["S"].ndim == 3 else s["S"][j:j + 1]
        om = s["om"] if s["om"].ndim == 2 else s["om"][j:j + 1]
        alone = _run(e1, s, sl=slice(j, j + 1), S=S, om=om)
        for nm, a, b in zip(NAMES, ref, alone):
            assert _same(a[j:j + 1], b), (nm, j)
    # shared maps against the same values given per slice
    if n > 1 and (s["S"].ndim == 3 or s["om"].ndim == 2):
        S = np.ascontiguousarray(np.broadcast_to(s["S"], (n,) + s["S"].shape[-3:]))
        om = np.ascontiguousarray(np.broadcast_to(s["om"], (n,) + s["om"].shape[-2:]))
        stacked = _run(planned(name), s, S=S, om=om)
        for nm, a, b in zip(NAMES, ref, stacked):
            assert _same(a, b), nm


# ---- 2. against the single-coil operator, bits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("A", "C", "E"))
def test_one_coil_of_ones_has_the_bits_of_the_single_coil_pair(name):
    s = setup(name)
    c = s["c"]
    n, h, w = c["n"], c["h"], c["w"]
    e = planned(name)
    maps = e.offres_maps(f32(s["om"]))
    ones = torch.ones((1, h, w), dtype=torch.complex64, device=DEV)
    y1 = c64(s["y"][:, :1])
    assert torch.equal(e.offres_forward_mc(c64(s["x"]), maps, ones)[:, 0], e.offres_forward(c64(s["x"]), maps))
    for wd in (None, f32((0.5 + np.arange(s["P"]["m"]) % 7 / 7.0).astype(np.float32))):
        assert torch.equal(e.offres_adjoint_mc(y1, maps, ones, wd), e.offres_adjoint(y1[:, 0].contiguous(), maps, wd))


@pytest.mark.parametrize("name", ("B", "C", "D", "E"))
def test_dyadic_maps_give_the_single_coil_bits_per_plane_and_the_combine_chain_its_bound(name):
    s = setup(name)
    c = s["c"]
    n, h, w, C = c["n"], c["h"], c["w"], c["C"]
    e = planned(name)
    maps = e.offres_maps(f32(s["om"]))
    S = MR.dyadic_sens(C, h, w)
    sd = c64(S)
    f = e.offres_forward_mc(c64(s["x"]), maps, sd)
    for k in range(C):
        img = c64((S[k] * s["x"]))                                                  # exact in float32: a power of two times a quarter turn
        assert torch.equal(f[:, k], e.offres_forward(img, maps)), k
    wd = _wd(s["wgt"])
    a = _np(e.offres_adjoint_mc(c64(s["y"]), maps, sd, wd))
    ac = np.stack([_np(e.offres_adjoint(c64(s["y"][:, k]), maps, wd)) for k in range(C)], axis=1)      # the device's own a_c
    want = (np.conj(S)[None] * ac).sum(axis=1)
    bound = 4 * C * U * (np.abs(S)[None] * np.abs(ac)).sum(axis=1)
    worst = float((np.abs(a - want) / np.maximum(bound, 1e-300)).max())
    print(f"case {name}: adjoint against the float64 combine of the device's a_c: worst |err| / bound {worst:.3f} (bound 4 C 2^-24 sum |S_c| |a_c|)")
    assert worst <= 1.0


# ---- 3. against float64, general maps -----------------------------------------------------------------------------------------------------------

def model_tol(c):
    ratio = 1.25 if min(c["grid"][0] / c["h"], c["grid"][1] / c["w"]) < 2.0 else 2.0
    return 1e-6 + 2.0 * TO.MODEL_ERR[(min(c["J"], 6), ratio)]


def forward_planes_bound(s, B, E, S4, x):
    """||Bf|| [N, C] per coil plane against the model on S_c . p (module docstring)"""
    c, P = s["c"], s["P"]
    n, L = x.shape[0], B.shape[0]
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    out = np.zeros((n, c["C"]))
    prod = NR.op_norm(P) * float(np.abs(B).max(axis=1).sum()) * gamma(3)
    for k in range(c["C"]):
        img = S4[:, k] * x
        if c["plan"] == "ls":
            planes = [NR.forward(P, E4[:, l] * img) for l in range(L)]
            b = TL.forward_err_norm(P, B, E, img, planes)
        else:
            Q = OR.plan(s["t"], L)
            b = TO.forward_err_norm(P, Q, E, img, OR.model_forward(P, Q, E, img))
        out[:, k] = b + prod * np.linalg.norm(img.reshape(n, -1), axis=1)
    return out


def adjoint_bound(s, B, E, S4, y, wgt, ac):
    c, P = s["c"], s["P"]
    out = np.zeros((y.shape[0], c["h"], c["w"]))
    for k in range(c["C"]):
        out += np.abs(S4[:, k]) * (TL.adjoint_err(P, B, E, y[:, k], wgt) + gamma(4 * c["C"]) * np.abs(ac[:, k]))
    return out


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_forward_and_adjoint_against_the_float64_model_the_dense_restatement_and_adjointness(name):
    s = setup(name)
    c, P = s["c"], s["P"]
    n, h, w, C, L = c["n"], c["h"], c["w"], c["C"], c["L"]
    e = planned(name)
    B = coefficients(e, s)
    sab = float(np.abs(B).sum(axis=0).max())
    maps = e.offres_maps(f32(s["om"]))
    E = _np(maps)
    S4 = MR._maps4(s["S"], n)
    x, y, wgt = s["x"], s["y"], s["wgt"]
    got_f = _np(e.offres_forward_mc(c64(x), maps, c64(s["S"])))
    got_a = _np(e.offres_adjoint_mc(c64(y), maps, c64(s["S"]), _wd(wgt)))
    mod_f, ac = MR.model_forward(P, B, E, s["S"], x), MR.coil_adjoints(P, B, E, y, wgt)
    mod_a = (np.conj(S4) * ac).sum(axis=1)
    bf, ba = forward_planes_bound(s, B, E, S4, x), adjoint_bound(s, B, E, S4, y, wgt, ac)
    ef = np.linalg.norm(got_f - mod_f, axis=2)
    ra = float((np.abs(got_a - mod_a) / ba).max())
    print(f"case {name} (C = {C}, L = {L} {c['plan']}, max sum |b| {sab:.2f}): forward worst ||err|| / bound over the coil planes {(ef / bf).max():.3e} "
          f"(||err|| up to {ef.max():.3e}); adjoint worst err / bound {ra:.3e}, max |err| {np.abs(got_a - mod_a).max():.3e}")
    assert (ef <= bf).all() and ra <= 1.0
    tau = LS.centres(s["t"], L)
    om64 = s["om"].astype(np.float64)
    ref_f = MR.segmented_forward(s["traj"], tau, B, om64, s["S"], x)
    ref_a = MR.segmented_adjoint(s["traj"], tau, B, om64, s["S"], y, h, w, wgt)
    tol = model_tol(c) * sab
    rf, rr = float(np.linalg.norm(got_f - ref_f) / np.linalg.norm(ref_f)), float(np.linalg.norm(got_a - ref_a) / np.linalg.norm(ref_a))
    print(f"        against the dense segmented restatement: forward rel l2 {rf:.3e}, adjoint rel l2 {rr:.3e} (tolerance {tol:.3e})")
    assert rf <= tol and rr <= tol
    yw = y if wgt is None else y * wgt.astype(np.float64)
    lhs = np.array([np.vdot(yw[j], got_f[j]) - np.vdot(got_a[j], x[j]) for j in range(n)])
    nx = np.linalg.norm(x.reshape(n, -1), axis=1)
    lim = (bf * np.linalg.norm(yw, axis=2)).sum(axis=1) + np.linalg.norm(ba.reshape(n, -1), axis=1) * nx
    print(f"        adjointness |<A p, W q> - <p, A^H W q>| {np.abs(lhs).tolist()} bound {lim.tolist()} (relative to ||p|| ||q||: "
          f"{(np.abs(lhs) / (nx * np.linalg.norm(y.reshape(n, -1), axis=1))).tolist()})")
    assert (np.abs(lhs) <= lim).all()


# ---- 4. the stage ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("C", "E"))
def test_the_stage_step_composition_cg_dc_stopped_slices_snapshots_and_workspace(name):
    """pnp_offres_mc_normal, pnp_offres_mc_cg_residual and the stage under pnp_step / pnp_prox_dual / pnp_residuals"""
    s = setup(name)
    c, P = s["c"], s["P"]
    n, h, w, C, L, K = c["n"], c["h"], c["w"], c["C"], c["L"], 4
    e = planned(name)
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
    ys = TO._rt(MR.model_forward(P, B, E, s["S"], xr.astype(np.complex128)) + 0.02 * (rng.standard_normal((n, C, m)) + 1j * rng.standard_normal((n, C, m))))
    # the condition-number factor: this operator against the single-coil linear stage at L = 3 with the same weights, float64 models
    Q3 = OR.plan(s["t"], 3)
    om0 = (s["om"] if s["om"].ndim == 2 else s["om"][0]).astype(np.float64)
    E3 = OR.maps(om0[None], Q3)
    s_lin = TL._norm_of(lambda p: OR.model_forward(P, Q3, E3, p), lambda q: OR.model_adjoint(P, Q3, E3, q, wgt), h, w)
    s_mc = MR.op_norm(P, B, E if E.ndim == 3 else E[0], s["S"] if s["S"].ndim == 3 else s["S"][0], wgt)
    scale = max(1.0, (s_mc + 0.3) / (s_lin + 0.3))
    print(f"case {name}: ||A^H W A||: {s_lin:.3f} single-coil linear L = 3, {s_mc:.3f} here: the CG tolerances are scaled by {scale:.3f}; max sum |b| {sab:.2f}")
    mu = np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    wd = f32(wgt)
    ws0 = e.workspace_bytes
    e.set_kspace_offres_mc(c64(ys), sd, od, wd, cg_iters=K)
    ws1 = e.workspace_bytes
    assert e.offres_mc_coils == C and not e.offres_live and e.ncsense_coils == 0 and e.coils == 0 and not e.offres_mc_cg_residual().any()
    assert ws1 > ws0
    e.set_kspace_offres_mc(c64(ys), sd, od, wd, cg_iters=K)                         # nothing left to grow
    assert e.workspace_bytes == ws1
    pd = c64(u0, (n, 1, h, w))
    q = _np(e.offres_mc_normal(pd, f32(mu)))[:, 0]
    comp = _np(e.offres_adjoint_mc(e.offres_forward_mc(pd, maps, sd), maps, sd, wd))
    exact = comp + mu64[:, None, None] * u0
    off = float(max((np.abs(q.real - exact.real) / np.maximum(np.abs(exact.real), 1e-30)).max(),
                    (np.abs(q.imag - exact.imag) / np.maximum(np.abs(exact.imag), 1e-30)).max()))
    print(f"offres_mc_normal against fma(mu, p, adjoint(forward(p))): worst relative distance {off:.3e} (one rounding: {U:.3e})")
    assert off <= U * (1 + 1e-6)
    aty = MR.model_adjoint(P, B, E, s["S"], ys, wgt)
    xs, zs, us = f32(xr, (n, 1, h, w)), c64(z0, (n, 1, h, w)), c64(u0, (n, 1, h, w))
    e.prox_dual(xs, zs, us, f32(mu))
    zr, ur, rr = MR.prox_dual(P, B, E, s["S"], xr, z0, u0, aty, mu64, K, wgt)
    res = e.offres_mc_cg_residual().cpu().numpy().astype(np.float64)
    bmax, brms, bres = (scale * TO.MARGIN * v for v in TO.F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"prox_dual K={K}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    dc = e.residuals(xs, zs, us, dc=True).cpu().numpy().astype(np.float64)[:, 5]
    dcr = MR.dc_misfit(P, B, E, s["S"], xr, ys, wgt)
    bdc = 1e-6 * NR.op_norm(P) * sab * math.sqrt(float(wgt.max())) * np.linalg.norm(xr.reshape(n, -1), axis=1) + 5e-7 * dcr
    print(f"dc column {dc} ref {dcr} |d| {np.abs(dc - dcr)} bound {bdc}")
    assert (np.abs(dc - dcr) <= bdc).all()
    # three steps under the TV prior: each is tv_denoise then prox_dual, bit for bit; slice 1 stopped in step 2
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = f32(np.full(n, 0.05, dtype=np.float32))
    e2 = planned(name)
    e2.set_kspace_offres_mc(c64(ys), sd, od, wd, cg_iters=K)
    t_state = torch.zeros(n, dtype=torch.float32, device=DEV)
    for step in range(3):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [v.clone() for v in (xs, zs, us, t_state, e.offres_mc_cg_residual())]
        tact = f32(np.array([0.0, 1.0 if step == 1 else 0.0], dtype=np.float32))
        x2, z2, u2 = xs.clone(), zs.clone(), us.clone()
        xp = e2.tv_denoise(z2.real - u2.real, torch.tensor(1.0, dtype=torch.float32, device=DEV) * sig, 5)
        if step == 1:
            xp[1] = x2[1]
        e2.prox_dual(xp, z2, u2, f32(mu), tact)
        e.step(xs, zs, us, f32(mu), sig, t_action=tact, t_state=t_state)
        for nm, a, b in zip("xzu", (xs, zs, us), (xp, z2, u2)):
            assert _same(a, b), (f"step {step + 1}: {nm} of pnp_step differs from tv_denoise + pnp_prox_dual")
        zr, ur, rr = MR.prox_dual(P, B, E, s["S"], _np(xs)[:, 0], zin, uin, aty, mu64, K, wgt)
        live = [0] if step == 1 else [0, 1]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:                                                               # the stopped slice keeps z, u and the CG residual bit for bit
            for nm, a, kp in zip(("x", "z", "u", "t", "cg"), (xs, zs, us, t_state, e.offres_mc_cg_residual()), keep):
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
        e.reset_offres_mc(zs.clone(), c64(ys), sd, od, wd, cg_iters=_lib.PNP_MC_MAX_CG + 1)
    with pytest.raises(_lib.PnPError, match="map_n"):
        _lib.check(e.lib.pnp_set_kspace_offres_mc(e._h, c64(ys).data_ptr(), sd.data_ptr(), C, 1 if s["S"].ndim == 3 else n, od.data_ptr(), n + 1,
                                                  wd.data_ptr(), K, None), "pnp_set_kspace_offres_mc")
    assert e.offres_mc_coils == C
    for a, b in zip((xs, zs, us), keep):
        assert _same(a, b)
    e.step(xs, zs, us, f32(mu), sig)


# ---- 4b. installed last, the plan calls, the getters ------------------------------------------------------------------------------------------------

class _Episode(TO._Episode):
    """tests/test_gpu_offres.py's episode of one stage kind, and the new kind "offres_mc" (3 coils, the handle's live plan)"""

    def __init__(self, e, kind, n, h, w, seed):
        super().__init__(e, "ns" if kind == "offres_mc" else kind, n, h, w, seed)     # y [n, 3, m], as the non-Cartesian SENSE episode's
        self.kind = kind

    def reset(self):
        if self.kind != "offres_mc":
            return super().reset()
        return self.e.reset_offres_mc(self.x0, self.y, self.sens, self.om, self.w, cg_iters=3)

    def set_kspace(self):
        if self.kind != "offres_mc":
            return super().set_kspace()
        return self.e.set_kspace_offres_mc(self.y, self.sens, self.om, self.w, cg_iters=3)


OTHERS = TO.OTHERS + ("offres",)
H_N, H_H, H_W, H_L = TO.H_N, TO.H_H, TO.H_W, TO.H_L


def test_installed_last_in_both_orders_the_plan_calls_and_the_getters():
    """pnp_set_kspace_offres_mc, pnp_reset_offres_mc: the stage installed last runs, against every other installer in both orders; the three
    plan calls drop the stage; the PNP_ERR_STATE matrix of the getters"""
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    for other in OTHERS:
        for first, second in (("offres_mc", other), (other, "offres_mc")):
            e = TO._handle()
            a = _Episode(e, first, H_N, H_H, H_W, 1)
            it = a.reset()
            a.step(it, 0); a.step(it, 1)
            want = a.state(it)
            e = TO._handle()                                                        # the same episode with the other stage's installers in between
            a, b = _Episode(e, first, H_N, H_H, H_W, 1), _Episode(e, second, H_N, H_H, H_W, 2)
            it = a.reset()
            a.step(it, 0)
            itb = b.reset()
            assert e.offres_mc_coils == (3 if second == "offres_mc" else 0)
            b.step(itb, 0)                                                          # the stage installed last runs
            eb = TO._handle()
            b2 = _Episode(eb, second, H_N, H_H, H_W, 2)
            itb2 = b2.reset()
            b2.step(itb2, 0)
            for nm, p, q in zip("xzud", b.state(itb), b2.state(itb2)):
                assert _same(p, q), (first, second, nm)
            a.set_kspace()
            assert e.offres_mc_coils == (3 if first == "offres_mc" else 0)
            a.step(it, 1)
            for nm, p, q in zip("xzud", a.state(it), want):
                assert _same(p, q), (first, second, nm)
    # the getters while this stage is live
    e = TO._handle()
    a = _Episode(e, "offres_mc", H_N, H_H, H_W, 1)
    it = a.reset()
    a.step(it, 0)
    assert e.offres_mc_coils == 3 and not e.offres_live and e.ncsense_coils == 0 and e.coils == 0
    mu = f32(np.full(H_N, 0.3, dtype=np.float32))
    for stage in ("mc", "nc", "ncsense", "offres"):
        with pytest.raises(_lib.PnPError, match=r"\(-3\)"):
            e._cg_residual(f"pnp_{stage}_cg_residual")
        with pytest.raises(_lib.PnPError, match=r"\(-3\)"):
            e._normal(f"pnp_{stage}_normal", it[1], mu)
    assert e.offres_mc_cg_residual().shape == (H_N,)
    # the three plan calls drop the stage
    for replan in (lambda: e.offres_plan(t, H_L + 1), lambda: e.offres_plan_ls(t, H_L, TL.band_of(om)),
                   lambda: e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)):
        if e.offres_segments == 0:
            e.offres_plan(t, H_L)
        a.set_kspace()
        assert e.offres_mc_coils == 3
        keep = [v.clone() for v in it]
        replan()
        assert e.offres_mc_coils == 0
        with pytest.raises(_lib.PnPError):
            a.step(it, 1)
        with pytest.raises(_lib.PnPError, match="not in multi-coil off-resonance mode"):
            e.offres_mc_cg_residual()
        for v, k in zip(it, keep):
            assert _same(v, k)
    with pytest.raises(_lib.PnPError, match="no off-resonance plan"):
        a.set_kspace()
    e.offres_plan(t, H_L)
    a.set_kspace()
    a.step(it, 1)
    e2 = TO._handle()
    a2 = _Episode(e2, "offres_mc", H_N, H_H, H_W, 1)
    it2 = a2.reset()
    a2.step(it2, 0); a2.step(it2, 1)
    for nm, p, q in zip("xzud", a.state(it), a2.state(it2)):
        assert _same(p, q), nm


# ---- 5. non-interference ----------------------------------------------------------------------------------------------------------------------------

def test_the_new_intruders_between_two_steps_of_the_other_kinds_change_nothing():
    """pnp_offres_forward_mc, pnp_offres_adjoint_mc, pnp_acquire_offres_mc between two steps of a live episode of every stage kind"""
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    m = P["m"]
    rng = np.random.default_rng(77)
    x = TO._rt(rng.standard_normal((H_N, H_H, H_W)) + 1j * rng.standard_normal((H_N, H_H, H_W)))
    wgt = (0.5 + rng.random(m)).astype(np.float32)
    gt = f32(np.stack([synthetic.phantom(H_H, H_W, 70 + j) for j in range(H_N)]).astype(np.float32), (H_N, 1, H_H, H_W))
    for kind in OTHERS + ("offres_mc",):
        ref = _Episode(TO._handle(), kind, H_N, H_H, H_W, 1)
        itr = ref.reset()
        ref.step(itr, 0); ref.step(itr, 1)
        e = TO._handle()
        ep = _Episode(e, kind, H_N, H_H, H_W, 1)
        it = ep.reset()
        ep.step(it, 0)
        live, ws = e.offres_mc_coils, e.workspace_bytes
        for C, omega in ((2, f32(om[2])), (9, f32(om[:H_N] * 3.0))):                # fewer and more coils than the episode's 3: the scratch grows
            sens = c64(synthetic.coil_maps(C, H_H, H_W))
            maps = e.offres_maps(omega)
            y = TO._rt(rng.standard_normal((H_N, C, m)) + 1j * rng.standard_normal((H_N, C, m)))
            e.offres_forward_mc(c64(x), maps, sens)
            e.offres_adjoint_mc(c64(y), maps, sens, f32(wgt))
            e.acquire_offres_mc(gt, sens, omega, 0.05, 7, dcf=f32(wgt))
        assert e.offres_mc_coils == live and e.workspace_bytes >= ws
        ep.step(it, 1)
        for nm, p, q in zip("xzud", ep.state(it), ref.state(itr)):
            assert _same(p, q), (kind, nm)


def test_the_existing_intruders_between_two_steps_of_the_new_kind_change_nothing():
    """pnp_offres_forward / _adjoint, pnp_nufft_forward_mc / _adjoint_mc, pnp_nufft_dcf and pnp_fieldmap_estimate share the block scratch"""
    traj, t, P, om = TO.setup(H_H, H_W, "spiral", 6)
    m = P["m"]
    rng = np.random.default_rng(78)
    x = TO._rt(rng.standard_normal((H_N, H_H, H_W)) + 1j * rng.standard_normal((H_N, H_H, H_W)))
    y = TO._rt(rng.standard_normal((H_N, 9, m)) + 1j * rng.standard_normal((H_N, 9, m)))
    ref = _Episode(TO._handle(), "offres_mc", H_N, H_H, H_W, 1)
    itr = ref.reset()
    ref.step(itr, 0); ref.step(itr, 1)
    e = TO._handle()
    ep = _Episode(e, "offres_mc", H_N, H_H, H_W, 1)
    it = ep.reset()
    ep.step(it, 0)
    maps = e.offres_maps(f32(om[:H_N] * 2.0))
    e.offres_forward(c64(x), maps)
    e.offres_adjoint(c64(y[:, 0]), maps, None)
    sens = c64(synthetic.coil_maps(9, H_H, H_W))
    e.nufft_forward_mc(c64(x), sens)
    e.nufft_adjoint_mc(c64(y), sens, None)
    e.nufft_dcf(iters=5)
    x1 = c64(np.broadcast_to(x[:, None], (H_N, 2, H_H, H_W)))
    e.fieldmap_estimate(x1, x1 * torch.exp(torch.tensor(0.3j, device=DEV)), 1e-3, iters=10)
    e.acquire_offres(f32(np.abs(x), (H_N, 1, H_H, H_W)), f32(om[0]), 0.01, 3)
    assert e.offres_mc_coils == 3
    ep.step(it, 1)
    for nm, p, q in zip("xzud", ep.state(it), ref.state(itr)):
        assert _same(p, q), nm


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
    od = f32(om[0])

    def refused(rc, what, code):
        assert rc == code and what in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    fwd = lambda map_n=1, sens_n=1, coils=C, batch=n: lib.pnp_offres_forward_mc(e._h, img.data_ptr(), maps.data_ptr(), map_n, sens.data_ptr(), sens_n,  # noqa: E731
                                                                                  coils, batch, out.data_ptr(), None)
    adj = lambda map_n=1, sens_n=1: lib.pnp_offres_adjoint_mc(e._h, out.data_ptr(), None, maps.data_ptr(), map_n, sens.data_ptr(), sens_n, C, n,  # noqa: E731
                                                               img.data_ptr(), None)
    ins = lambda map_n=1, sens_n=1: lib.pnp_set_kspace_offres_mc(e._h, out.data_ptr(), sens.data_ptr(), C, sens_n, od.data_ptr(), map_n, None, 4, None)  # noqa: E731
    acq = lambda map_n=1: lib.pnp_acquire_offres_mc(e._h, img.data_ptr(), sens.data_ptr(), C, 1, od.data_ptr(), map_n, None, 0.0, 0, 0, out.data_ptr(),  # noqa: E731
                                                    None, None, None)
    for call in (fwd, adj, ins, acq):
        refused(call(), b"no NUFFT plan", -3)
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)
    for call in (fwd, adj, ins, acq):
        refused(call(), b"no off-resonance plan", -3)
    e.offres_plan(t, 3)
    for call in (fwd, adj, ins, acq):
        refused(call(map_n=3), b"map_n must be 1 or n=2", -1)
    for call in (fwd, adj, ins):
        refused(call(sens_n=3), b"sens_n must be 1 or n=2", -1)
    refused(fwd(batch=n + 1), b"batch must be 1..n=2", -1)
    refused(fwd(coils=0), b"coils must be 1..32", -1)
    refused(fwd(coils=33), b"coils must be 1..32", -1)
    refused(lib.pnp_offres_mc_cg_residual(e._h, out.data_ptr(), None), b"not in multi-coil off-resonance mode", -3)
    refused(lib.pnp_offres_mc_normal(e._h, img.data_ptr(), od.data_ptr(), out.data_ptr(), None), b"not in multi-coil off-resonance mode", -3)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == 7.0).all()) and e.offres_mc_coils == 0 and lib.pnp_offres_mc_coils(None) == 0


# ---- 6. guard bands -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,naive", (("B", 0), ("C", 0), ("D", 0), ("E", 1)))
def test_every_caller_owned_buffer_keeps_its_guard_bands(name, naive, monkeypatch):
    s = setup(name)
    c, P = s["c"], s["P"]
    n, h, w, C, L, m = c["n"], c["h"], c["w"], c["C"], c["L"], s["P"]["m"]
    e = planned(name, monkeypatch=monkeypatch, naive=naive)
    lib, st = e.lib, e._stream()
    wgt = (0.5 + np.arange(m) % 5 / 5.0).astype(np.float32)
    S4 = np.ascontiguousarray(MR._maps4(s["S"], n))
    om3 = np.ascontiguousarray(np.broadcast_to(s["om"], (n, h, w)))
    for sens_n, map_n in ((1, 1), (n, n)):
        sd, od = g_c64(S4[0] if sens_n == 1 else S4), g_f32(om3[0] if map_n == 1 else om3)
        maps = GB.guarded((map_n, L, h, w), torch.complex64, DEV)
        _lib.check(lib.pnp_offres_maps(e._h, od.data_ptr(), map_n, maps.data_ptr(), st), "pnp_offres_maps")
        for batch in (1, n):
            img, smp, wd = g_c64(s["x"][:batch]), g_c64(s["y"][:batch]), g_f32(wgt)
            out_s, out_i = GB.guarded((batch, C, m), torch.complex64, DEV), GB.guarded((batch, h, w), torch.complex64, DEV)
            with GB.watch(outputs={"samples": out_s}, inputs={"img": img, "maps": maps, "sens": sd}):
                _lib.check(lib.pnp_offres_forward_mc(e._h, img.data_ptr(), maps.data_ptr(), map_n, sd.data_ptr(), sens_n, C, batch, out_s.data_ptr(), st),
                           "pnp_offres_forward_mc")
            with GB.watch(outputs={"img": out_i}, inputs={"samples": smp, "weights": wd, "maps": maps, "sens": sd}):
                _lib.check(lib.pnp_offres_adjoint_mc(e._h, smp.data_ptr(), wd.data_ptr(), maps.data_ptr(), map_n, sd.data_ptr(), sens_n, C, batch,
                                                     out_i.data_ptr(), st), "pnp_offres_adjoint_mc")
        gt = g_f32(np.stack([synthetic.phantom(h, w, 50 + j) for j in range(n)]).astype(np.float32), (n, 1, h, w))
        wd = g_f32(wgt)
        yo = GB.guarded((n, C, m), torch.complex64, DEV)
        ao, xo = GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"y": yo, "aty0": ao, "x0": xo}, inputs={"gt": gt, "sens": sd, "omega": od, "dcf": wd}):
            _lib.check(lib.pnp_acquire_offres_mc(e._h, gt.data_ptr(), sd.data_ptr(), C, sens_n, od.data_ptr(), map_n, wd.data_ptr(), 0.02, 5, 0,
                                                 yo.data_ptr(), ao.data_ptr(), xo.data_ptr(), st), "pnp_acquire_offres_mc")
        xs, zs, us = GB.guarded((n, 1, h, w), torch.float32, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"x": xs, "z": zs, "u": us}, inputs={"x0": xo, "y": yo, "sens": sd, "omega": od, "w": wd}):
            _lib.check(lib.pnp_reset_offres_mc(e._h, xo.data_ptr(), yo.data_ptr(), sd.data_ptr(), C, sens_n, od.data_ptr(), map_n, wd.data_ptr(), 3,
                                               xs.data_ptr(), zs.data_ptr(), us.data_ptr(), st), "pnp_reset_offres_mc")
        with GB.watch(outputs={}, inputs={"y": yo, "sens": sd, "omega": od, "w": wd, "x": xs, "z": zs, "u": us}):
            _lib.check(lib.pnp_set_kspace_offres_mc(e._h, yo.data_ptr(), sd.data_ptr(), C, sens_n, od.data_ptr(), map_n, wd.data_ptr(), 3, st),
                       "pnp_set_kspace_offres_mc")
        mu = g_f32(np.array([0.3, 0.05, 0.6], dtype=np.float32)[:n])
        q, res = GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n,), torch.float32, DEV)
        with GB.watch(outputs={"q": q}, inputs={"p": zs, "mu": mu}):
            _lib.check(lib.pnp_offres_mc_normal(e._h, zs.data_ptr(), mu.data_ptr(), q.data_ptr(), st), "pnp_offres_mc_normal")
        with GB.watch(outputs={"z": zs, "u": us}, inputs={"x": xs, "mu": mu}):
            e.prox_dual(xs, zs, us, mu)
        with GB.watch(outputs={"out": res}, inputs={}):
            _lib.check(lib.pnp_offres_mc_cg_residual(e._h, res.data_ptr(), st), "pnp_offres_mc_cg_residual")
        assert torch.isfinite(res).all() and torch.isfinite(torch.view_as_real(q)).all()
    assert e.offres_mc_coils == C                                                   # pnp_offres_mc_coils


# ---- 7. the correction corrects, with coils -------------------------------------------------------------------------------------------------------

def test_the_correction_corrects_with_coils_on_the_device():
    """offres_ref.CORRECTS with 4 coils: y per coil from the exact operator in float64, L = 8 least squares, Pipe weights, TV, 30 steps, K = 8.
    The float64 restatement (tests/test_offres_mc_host.py) ends at offres_mc_ref.CORRECTS_MC_PSNR for this stage and for the plain
    non-Cartesian SENSE stage on the same y."""
    c = OR.CORRECTS
    h, w = c["h"], c["w"]
    traj, t, omega, gt, S, y = MR.corrects_problem()
    P = NR.plan(h, w, c["grid"][0], c["grid"][1], c["J"], traj)
    dcf = f32(D.pipe(P, 30)[0].astype(np.float32))
    e = _engine(1, h, w)
    e.nufft_plan(traj, grid=c["grid"], width=c["J"])
    e.offres_plan_ls(t, MR.CORRECTS_L, band_of(omega))
    e.set_prior("tv", tv_scale=1.0, tv_iters=c["tv_iters"])
    sd, od, yd = c64(S), f32(omega.astype(np.float32)), c64(y[None])
    gtd = f32(gt.astype(np.float32), (1, 1, h, w))
    mu = f32(np.full(1, c["mu"], dtype=np.float32))
    out = []
    for stage in ("offres_mc", "ncsense"):
        if stage == "offres_mc":
            x0 = e.offres_adjoint_mc(yd, e.offres_maps(od), sd, dcf).reshape(1, 1, h, w)
            xs, zs, us = e.reset_offres_mc(x0, yd, sd, od, dcf, cg_iters=c["K"])
            assert e.offres_mc_coils == MR.CORRECTS_COILS
        else:
            x0 = e.nufft_adjoint_mc(yd, sd, dcf).reshape(1, 1, h, w)
            xs, zs, us = e.reset_ncsense(x0, yd, sd, dcf, cg_iters=c["K"])
        for sg in OR.corrects_schedule():
            e.step(xs, zs, us, mu, f32(np.full(1, sg, dtype=np.float32)))
        out.append(float(e.psnr(xs, gtd)[0]))
    ref = MR.CORRECTS_MC_PSNR
    print(f"4 coils, L = {MR.CORRECTS_L} least squares: {out[0]:.3f} dB (float64: {ref[0]}); the plain non-Cartesian SENSE stage on the same y: "
          f"{out[1]:.3f} dB (float64: {ref[1]})")
    assert abs(out[0] - ref[0]) <= 0.01 and abs(out[1] - ref[1]) <= 0.01
    assert out[0] - out[1] >= 0.5 * (ref[0] - ref[1])


def test_the_correction_with_coils_through_the_environment_and_the_fixed_schedule_solver():
    """PnPEnv(offres_mc=True).reset with data["omega"], data["times"] and data["sens"]: the same fixture through the public drivers ends at
    the restatement's PSNR; another episode in between is re-bound; an env without the option still refuses the dict"""
    from dt4image_restoration_amd import acquisition
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    c = OR.CORRECTS
    h, w, L, C = c["h"], c["w"], MR.CORRECTS_L, MR.CORRECTS_COILS
    traj, t, omega, gt, S, y = MR.corrects_problem()
    m = traj.shape[0]
    env = PnPEnv(max_episode_step=c["steps"], denoiser=TVDenoiser2D(scale=1.0, iters=c["tv_iters"]), device_type="cuda", cg_iters=c["K"],
                 nufft_width=c["J"], nufft_grid=c["grid"], offres_mc=True)
    eng = env._engine_for(1, h, w, torch.device("cuda", 0))
    dcf = acquisition.pipe_dcf(env, traj, iters=30, width=c["J"], grid=c["grid"])
    od, sd, yd = f32(omega.astype(np.float32)), c64(S), c64(y[None])
    eng.offres_plan_ls(t, L, band_of(omega))
    x0 = eng.offres_adjoint_mc(yd, eng.offres_maps(od), sd, dcf).reshape(1, 1, h, w)
    mat = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(yd), "ATy0": torch.view_as_real(x0), "gt": f32(gt.astype(np.float32), (1, 1, h, w)),
           "traj": torch.from_numpy(traj), "dcf": dcf, "omega": od, "times": torch.from_numpy(t), "segments": L, "b0_interp": "ls", "sens": sd}
    mu, sig = np.full((1, c["steps"]), c["mu"], dtype=np.float32), OR.corrects_schedule()[None]
    r = FixedScheduleSolver(env, max_iter=c["steps"], dc=True).run(mat, mu, sig)
    assert env._engine.offres_mc_coils == C and not env._engine.offres_live and env._engine.offres_interpolator() == "ls"
    p = TO._psnr(_np(r.x)[0, 0], gt)
    print(f"through PnPEnv(offres_mc=True) and FixedScheduleSolver: {p:.3f} dB (float64 restatement {MR.CORRECTS_MC_PSNR[0]}), dc {r.dc.tolist()}")
    assert abs(p - MR.CORRECTS_MC_PSNR[0]) <= 0.01
    # two steps of an episode, a plain non-Cartesian SENSE episode on the same handle in between: re-bound, the same bits
    act = {"mu": np.full(1, c["mu"], dtype=np.float32), "sigma_d": np.full(1, 0.05, dtype=np.float32), "T": np.zeros(1, dtype=np.float32)}
    st = env.reset(mat, "cuda")
    st, _ = env.step(st, act)
    ref, _ = env.step(OrderedDictCopy(st), act)
    other = env.reset({k: v for k, v in mat.items() if k not in ("omega", "times", "segments", "b0_interp")}, "cuda")
    assert env._engine.offres_mc_coils == 0 and env._engine.ncsense_coils == C
    env.step(other, act)
    got, _ = env.step(st, act)
    assert env._engine.offres_mc_coils == C
    for k in ("x", "z", "u"):
        assert _same(got[k], ref[k]), k
    plain = PnPEnv(max_episode_step=c["steps"], denoiser=TVDenoiser2D(scale=1.0, iters=c["tv_iters"]), device_type="cuda", cg_iters=c["K"],
                   nufft_width=c["J"], nufft_grid=c["grid"])
    with pytest.raises(ValueError, match="single-coil"):
        plain.reset(mat, "cuda")


def OrderedDictCopy(st):
    """a state dict with its own copies of the iterate (env.step works in place)"""
    from collections import OrderedDict
    return OrderedDict((k, v.clone() if k in ("x", "z", "u", "T") else v) for k, v in st.items())


# ---- 8. the CLI -------------------------------------------------------------------------------------------------------------------------------------

def test_cli_b0_coils_fixed_on_a_ground_truth_folder(tmp_path, monkeypatch):
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
            "--interleaves", "8", "--b0", "40", "--readout-ms", "10"]

    def run(extra):
        with contextlib.redirect_stdout(io.StringIO()):
            out = cli.main(base + extra + ["fixed", "--max_iter", "10", "--dc"])
        assert len(out) == 1 and out[0]["n"] == 2
        return out[0]

    mc = run(["--b0-coils", "4", "--b0-interp", "ls"])
    assert engines and engines[-1].offres_mc_coils == 4 and engines[-1].offres_interpolator() == "ls" and not engines[-1].offres_live
    one = run(["--b0-interp", "ls"])                                                 # the single-coil run of the same phantoms beside it
    assert engines[-1].offres_mc_coils == 0 and engines[-1].offres_live
    print(f"cli --traj spiral --b0 40 --readout-ms 10 --b0-interp ls fixed: --b0-coils 4: {mc['psnr']:.3f} dB (+{mc['psnr_increment']:.3f}), dc {mc.get('dc')}; "
          f"single-coil: {one['psnr']:.3f} dB (+{one['psnr_increment']:.3f}), dc {one.get('dc')}")
    assert "spiral-nc" in mc["set"] and np.isfinite(mc["psnr"]) and mc["psnr_increment"] > 0.0
