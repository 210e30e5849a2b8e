"""The Toeplitz normal operator on the MI355X, through the C ABI of include/pnpadmm_toeplitz.h (PnPEngine is the ctypes binding), against the
float64 restatement of tests/toeplitz_ref.py - which is the EXACT operator A^H W A to 1e-15 (tests/test_toeplitz_host.py), where the NUFFT
pair is a 1e-5 .. 9e-4 model of it.  Every buffer handed to the new entry points comes from tests/guard_bands.py.  Every figure is printed
before it is asserted.  No bound here is measured on the device.

SHAPES.  toeplitz_ref's 13 cases: the five of nufft_ref.CASES; (1, 80, 80) and (1, 64, 80), whose padded grid has a side of 160 (the mixed-radix
family: these handles run the composed form); the thin shapes (1, 128 / 256 / 512, 16) and (1, 16, 128 / 256 / 512), which reach every column
and row length 32 .. 1024 of the power-of-two family - the register-resident 256- and 512-point passes included - at a few thousand samples.
FORMS.  Both are run: the fused three launches (the default where the padded grid is a power of two) and the composed seven, on a handle
created under PNP_TOEPLITZ_NAIVE=1.  They need not agree bit for bit; each is held to float64.

BOUNDS (u = 2^-24).
  Spectrum, per entry: |K_dev - K_ref| <= 2^-24 |K_ref| + B, B[j,l] = M 2^-52 sum_m w_m |D_H| |D_W| / (H W) (toeplitz_ref.spectrum_bound): the
      one rounding to float32 plus the rounding of an M-term float64 sum.
  Application, per slice in the l2 norm: MARGIN = 10 times the error of the float32 restatement toeplitz_ref.apply_f32 (K rounded to
      float32, the input and the result of each of the four stages rounded to complex64, float64 arithmetic in between) against float64 -
      the rule of tests/test_gpu_sense.py.  The restatement's error is 3.4e-8 .. 4.7e-8 on these cases, so THE BOUND IS 3.4e-7 .. 4.7e-7
      relative; on case 1 (64 x 64, where the NUFFT model at 64 -> 80, J = 6 is 4.9e-4 off) it is 4.2e-7, and the test asserts that it lies
      below half of 4.9e-4: a run that silently used the NUFFT operator fails.  (The other route, from the suite's pnp_fft2c bound through
      two transforms and max |K|, is not used.)
  Multi-coil application: the same rule on the restatement that also rounds the maps' products (coil image and combine) to complex64.
  Nop: MARGIN times the float32 restatement plus 2 u ||q|| (the epilogue's fma).
  Stage: the "Stage" figures of tests/test_gpu_nufft.py and tests/test_gpu_ncsense.py (ten times the float32 restatement of
      tests/test_gpu_sense.py at mu = 0.3, K = 4: err_max 9.992e-07, err_rms 3.740e-07, d_res 2.784e-07), asserted at K = 4 and K = 8 against
      the float64 CG on the Toeplitz operator with the NUFFT model's aty, as the library forms it.
  DC column: the bits of the NUFFT stage's DC column on the same iterate (the same code runs).
  End to end: within 0.01 dB of the float64 Toeplitz restatement (toeplitz_ref.FIXTURE_PSNR: 16.572 -> 36.812 dB; FIXTURE_PSNR_MC: 17.493 ->
      32.399 dB), the bound of the two existing fixtures.  This test cannot tell the two stages apart; the application test does.
Figures measured on the MI355X are printed by the tests; none of them sets a bound."""
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as GB  # noqa: E402
import handle_cases as HC  # noqa: E402
import ncsense_ref as SR  # noqa: E402
import nufft_ref as NR  # noqa: E402
import test_gpu_ncsense as TS  # noqa: E402  (its episodes and helpers; its tests are not collected from here)
import test_gpu_nufft as TN  # noqa: E402
import toeplitz_cases as TC  # noqa: E402
import toeplitz_ref as T  # noqa: E402

from dt4image_restoration_amd import _lib, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
MARGIN = 10.0
MODEL_CASE1 = 4.9e-4                                            # the NUFFT model against the exact operator on case 1 (64 -> 80, J = 6)
g_c64, g_f32, _np, _same, _rt = TN.g_c64, TN.g_f32, TN._np, TN._same, TN._rt
NAIVE_ENV, BLOCK_ENV = "PNP_TOEPLITZ_NAIVE", "PNP_NCSENSE_COIL_BLOCK"
FORMS = ("fused", "composed")


def _engine(n, h, w, naive=False, block=None, profile=False):
    """a handle in the shipped form (fused where the padded grid is a power of two) or, naive, created under PNP_TOEPLITZ_NAIVE=1: the composed
    form; block: PNP_NCSENSE_COIL_BLOCK.  Both variables are read at pnp_create"""
    from dt4image_restoration_amd.engine import PnPEngine
    old = {k: os.environ.pop(k, None) for k in (NAIVE_ENV, BLOCK_ENV)}
    try:
        if naive:
            os.environ[NAIVE_ENV] = "1"
        if block is not None:
            os.environ[BLOCK_ENV] = str(block)
        return PnPEngine(n, h, w, device=0, denoiser=False, profile=profile)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_REF = {}


def ref(i):
    """(traj, weights float32, image complex128 rounded to complex64, K float64, B) of toeplitz_ref's case i, computed once"""
    if i not in _REF:
        n, h, w = T.case_shape(i)
        traj, wgt = T.case_traj(i), T.case_weights(i)
        _REF[i] = (traj, wgt, _rt(T.case_image(i)), T.spectrum(traj, h, w, wgt), T.spectrum_bound(traj, h, w, wgt))
    return _REF[i]


def planned(i, n=None, naive=False, block=None, weights="case", profile=False):
    """a handle with the case's NUFFT plan (the case's grid and width for the five of nufft_ref.CASES, the defaults otherwise) and spectrum"""
    traj, wgt = ref(i)[:2]
    h, w = T.case_shape(i)[1:]
    e = _engine(n or T.case_shape(i)[0], h, w, naive, block, profile)
    if i < len(NR.CASES):
        e.nufft_plan(traj, grid=NR.CASES[i][3:5], width=NR.CASES[i][5])
    else:
        e.nufft_plan(traj, width=6)
    if weights is not False:
        e.toeplitz_plan(g_f32(wgt) if isinstance(weights, str) else weights)
    return e


def raw_spectrum(e):
    out = GB.guarded((2 * e.h, 2 * e.w), torch.float32, DEV)
    with GB.watch(outputs={"out": out}):
        _lib.check(e.lib.pnp_toeplitz_spectrum(e._h, out.data_ptr(), e._stream()), "pnp_toeplitz_spectrum")
    return out


def raw_apply(e, img):
    out = GB.guarded((img.shape[0], e.h, e.w), torch.complex64, DEV)
    with GB.watch(outputs={"out": out}, inputs={"img": img}):
        _lib.check(e.lib.pnp_toeplitz_apply(e._h, img.data_ptr(), img.shape[0], out.data_ptr(), e._stream()), "pnp_toeplitz_apply")
    return out


def raw_apply_mc(e, img, sens):
    s, coils, sens_n = e._sens(sens)
    out = GB.guarded((img.shape[0], e.h, e.w), torch.complex64, DEV)
    with GB.watch(outputs={"out": out}, inputs={"img": img, "sens": sens}):
        _lib.check(e.lib.pnp_toeplitz_apply_mc(e._h, img.data_ptr(), s.data_ptr(), coils, sens_n, img.shape[0], out.data_ptr(), e._stream()),
                   "pnp_toeplitz_apply_mc")
    return out


def _l2(a, n):
    return np.linalg.norm(np.asarray(a).reshape(n, -1), axis=1)


def apply_mc_f32(K, x, S):
    """the float32 restatement of the multi-coil application: coil images and combine products rounded to complex64 as well"""
    S4 = SR._maps4(S, x.shape[0])
    out = np.zeros_like(x)
    for c in range(S4.shape[1]):
        out = _rt(out + _rt(np.conj(S4[:, c]) * T.apply_f32(K, _rt(S4[:, c] * x))))
    return out


# ---- the spectrum ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(T.N_CASES))
def test_spectrum_against_float64_and_its_bits_depend_on_trajectory_and_weights_only(i):
    traj, wgt, x, K, B = ref(i)
    n, h, w = T.case_shape(i)
    e = planned(i)
    assert e.toeplitz_planned and not e.toeplitz_live
    kd = raw_spectrum(e)
    got = _np(kd)
    r = float((np.abs(got - K) / (U * np.abs(K) + B)).max())
    print(f"case {i} {(n, h, w)} M {traj.shape[0]}: spectrum worst err / bound {r:.4f}, max B / max |K| {B.max() / np.abs(K).max():.2e}, "
          f"min K / max K {got.min() / got.max():.3f}")
    assert r <= 1.0 and got.min() < 0
    e.toeplitz_plan(g_f32(wgt))                                                     # a second build
    assert _same(raw_spectrum(e), kd)
    for nn, naive in ((1, True), (3, False)):                                       # another batch size, the other form's handle
        assert _same(raw_spectrum(planned(i, n=nn, naive=naive)), kd), (nn, naive)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e.toeplitz_plan(g_f32(wgt))
        ks = raw_spectrum(e)
    side.synchronize()
    assert _same(ks, kd)
    if i in (0, 4, 5, 9):                                                           # weights given as NULL against all-ones
        e.toeplitz_plan(None)
        k0 = raw_spectrum(e)
        e.toeplitz_plan(g_f32(np.ones(traj.shape[0], dtype=np.float32)))
        assert _same(raw_spectrum(e), k0) and not _same(k0, kd)
        k1 = T.spectrum(traj, h, w)
        assert float((np.abs(_np(k0) - k1) / (U * np.abs(k1) + T.spectrum_bound(traj, h, w))).max()) <= 1.0


# ---- the application ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(T.N_CASES))
def test_apply_against_the_float64_exact_operator(i, form):
    traj, wgt, x, K, B = ref(i)
    n, h, w = T.case_shape(i)
    e = planned(i, naive=form == "composed")
    got = _np(raw_apply(e, g_c64(x)))
    want = T.apply(K, x)
    f32 = T.apply_f32(K, x)
    bound = MARGIN * _l2(f32 - want, n) / _l2(want, n)
    err = _l2(got - want, n) / _l2(want, n)
    print(f"case {i} {(n, h, w)} {form}: apply rel l2 {err} bound {bound} (float32 restatement {bound / MARGIN})")
    assert (err <= bound).all()
    if i == 1:
        assert (bound < 0.5 * MODEL_CASE1).all()
        exact = NR.ndft_adjoint(traj, NR.ndft(traj, x), h, w, wgt.astype(np.float64))
        nufft = _np(e.nufft_adjoint(e.nufft_forward(g_c64(x)), g_f32(wgt)))
        en = float(np.linalg.norm(nufft - exact) / np.linalg.norm(exact))
        et = float(np.linalg.norm(got - exact) / np.linalg.norm(exact))
        print(f"case 1 against the exact NDFT operator: Toeplitz {et:.3e}, the device's NUFFT pair {en:.3e}")
        assert et <= bound.max() + 1e-12 and en > 0.5 * MODEL_CASE1                  # the NUFFT operator would have failed this test


@pytest.mark.parametrize("form", FORMS)
def test_bits_do_not_depend_on_the_batch_the_place_the_stream_the_maps_form_or_the_coil_block(form):
    i = 4                                                                           # 3 slices of 16 x 16
    traj, wgt, x, K, B = ref(i)
    n, h, w = T.case_shape(i)
    naive = form == "composed"
    S1 = SR.case_maps(4)                                                            # 9 coils: blocks 8 + 1 by default
    Sn = SR.case_maps(4, per_slice=True)
    e = planned(i, naive=naive)
    full, full_mc = raw_apply(e, g_c64(x)), raw_apply_mc(e, g_c64(x), g_c64(Sn))
    assert _same(raw_apply(e, g_c64(x)), full) and _same(raw_apply_mc(e, g_c64(x), g_c64(Sn)), full_mc)
    e1 = planned(i, n=1, naive=naive)
    for j in range(n):
        one = g_c64(x[j:j + 1])
        assert _same(raw_apply(e, one), full[j:j + 1]), j                           # batch 1 in the 3-slice handle: another place
        assert _same(raw_apply(e1, one), full[j:j + 1]), j                          # alone in a handle of one slice
        assert _same(raw_apply_mc(e1, one, g_c64(Sn[j])), full_mc[j:j + 1]), j
    two = raw_apply(e, g_c64(x[1:3]))
    assert _same(two, full[1:3])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a, b = raw_apply(e, g_c64(x)), raw_apply_mc(e, g_c64(x), g_c64(Sn))
    side.synchronize()
    assert _same(a, full) and _same(b, full_mc)
    shared = raw_apply_mc(e, g_c64(x), g_c64(S1))                                   # sens_n = 1 against N equal maps
    assert _same(raw_apply_mc(e, g_c64(x), g_c64(np.ascontiguousarray(np.broadcast_to(S1, (n,) + S1.shape)))), shared)
    for block in (1, 2, 3):                                                         # and the default 8 + 1 above
        eb = planned(i, naive=naive, block=block)
        assert _same(raw_apply_mc(eb, g_c64(x), g_c64(Sn)), full_mc), block
        assert _same(raw_apply(eb, g_c64(x)), full), block


@pytest.mark.parametrize("form", FORMS)
def test_apply_mc_against_float64_and_one_unit_map_is_the_single_coil_application(form):
    i = 3                                                                           # 64 x 32
    traj, wgt, x, K, B = ref(i)
    n, h, w = T.case_shape(i)
    e = planned(i, naive=form == "composed")
    for c in (1, 3, 9):
        S = _rt(synthetic.coil_maps(c, h, w))
        got = _np(raw_apply_mc(e, g_c64(x), g_c64(S)))
        want = T.apply_mc(K, x, S)
        bound = MARGIN * _l2(apply_mc_f32(K, x, S) - want, n) / _l2(want, n)
        err = _l2(got - want, n) / _l2(want, n)
        print(f"{form} C = {c}: apply_mc rel l2 {err} bound {bound}")
        assert (err <= bound).all()
    one = raw_apply_mc(e, g_c64(x), g_c64(np.ones((1, h, w), dtype=np.complex64)))
    assert torch.equal(torch.view_as_real(one), torch.view_as_real(raw_apply(e, g_c64(x))))      # as numbers


# ---- the stage ---------------------------------------------------------------------------------------------------------------------------------

def _check_stage(e, e_nufft, K64, P, S, xr, z0, u0, wgt, ys, aty, cg, normal, cg_residual, label):
    """the normal operator, one prox_dual, two steps (slice 1 stopped in the second) and the DC column of a live Toeplitz stage"""
    n, h, w = xr.shape
    mu = np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    assert e.toeplitz_live and not cg_residual(e).any()
    pd = g_c64(u0, (n, 1, h, w))
    q = _np(normal(e, pd, g_f32(mu)))[:, 0]
    qr = T.normal(K64, u0, mu64) if S is None else T.normal_mc(K64, u0, S, mu64)
    f32 = (T.apply_f32(K64, u0) if S is None else apply_mc_f32(K64, u0, S)) + mu64[:, None, None] * u0
    bq = MARGIN * _l2(f32 - qr, n) + 2 * U * _l2(qr, n)
    eq = _l2(q - qr, n)
    print(f"{label}: normal operator against float64 ||err|| {eq} bound {bq}")
    assert (eq <= bq).all()
    xs, zs, us = TS._iterate(xr, z0, u0)
    with GB.watch(outputs={"z": zs, "u": us}, inputs={"x": xs}):
        e.prox_dual(xs, zs, us, g_f32(mu))
    zr, ur, rr = T.prox_dual(K64, xr, z0, u0, aty, mu64, cg, S)
    res = cg_residual(e).cpu().numpy().astype(np.float64)
    bmax, brms, bres = (TN.MARGIN * v for v in TN.F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"{label} prox_dual K={cg}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} "
          f"d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    # the DC column: the NUFFT stage's, bit for bit, on the same iterate
    dc = e.residuals(xs, zs, us, dc=True)
    assert _same(dc[:, 5], e_nufft.residuals(xs, zs, us, dc=True)[:, 5]) and (dc[:, 5] > 0).all()
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = g_f32(np.full(n, 0.05, dtype=np.float32))
    t_state = GB.guarded((n,), torch.float32, DEV, fill=0.0)
    for step in range(2):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [t.clone() for t in (xs, zs, us, t_state, cg_residual(e))]
        tact = g_f32(np.array([0.0, 1.0 if step == 1 else 0.0, 0.0], dtype=np.float32))
        with GB.watch(outputs={"x": xs, "z": zs, "u": us, "t": t_state}, inputs={"mu": sig}):
            e.step(xs, zs, us, g_f32(mu), sig, t_action=tact, t_state=t_state)
        xd = _np(xs)[:, 0]
        zr, ur, rr = T.prox_dual(K64, xd, zin, uin, aty, mu64, cg, S)
        live = [0, 2] if step == 1 else [0, 1, 2]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"{label} step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:                                                               # the stopped slice keeps x, z, u, t and its CG residual
            for name, t, kp in zip(("x", "z", "u", "t", "cg"), (xs, zs, us, t_state, cg_residual(e)), keep):
                assert _same(t[1], kp[1]), name
    assert e.toeplitz_live


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", (4, 8))
def test_single_coil_stage_against_the_float64_cg_on_the_toeplitz_operator(K, form):
    i = 4
    P, traj, x, y = TN.case(i)
    n, h, w = NR.CASES[i][:3]
    xr, z0, u0, wgt, ys = TN._stage_inputs(i)
    K64 = T.spectrum(traj, h, w, wgt)
    e = planned(i, naive=form == "composed", weights=False)
    yd = g_c64(ys)
    with pytest.raises(_lib.PnPError, match="no Toeplitz spectrum"):                # the C installer plans nothing itself
        _lib.check(e.lib.pnp_set_kspace_nc_tz(e._h, yd.data_ptr(), K, e._stream()), "pnp_set_kspace_nc_tz")
    e.set_kspace_nc_tz(g_c64(ys), g_f32(wgt), cg_iters=K)                          # plans the spectrum for these weights, then installs
    assert e.toeplitz_planned and e.toeplitz_live and e.ncsense_coils == 0 and e.coils == 0
    en = TN.planned(i)
    en.set_kspace_nc(g_c64(ys), g_f32(wgt), cg_iters=K)
    assert not en.toeplitz_live
    _check_stage(e, en, K64, P, None, xr, z0, u0, wgt, ys, NR.adjoint(P, ys, wgt), K, lambda g, p, m: g.nc_normal(p, m),
                 lambda g: g.nc_cg_residual(), f"nc {form}")
    # the frozen case: y = 0, x0 = 0 never produces NaN
    zero = g_c64(np.zeros((n, 1, h, w), dtype=np.complex64))
    xs, zs, us = e.reset_nc_tz(zero, g_c64(np.zeros((n, P["m"]), dtype=np.complex64)), g_f32(wgt), cg_iters=K)
    e.prox_dual(xs, zs, us, g_f32(np.full(n, 0.3)))
    assert not TN._bits(zs).any() and not TN._bits(us).any() and not e.nc_cg_residual().any() and e.toeplitz_live


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", (4, 8))
def test_multi_coil_stage_against_the_float64_cg_on_the_toeplitz_operator(K, form):
    k = 4                                                                           # ncsense_ref's case 4: nufft case 4, 9 per-slice maps
    P, traj, x, y, S1, Sn = TS.case(k)
    n, h, w = NR.CASES[4][:3]
    xr, z0, u0, wgt, ys = TS._stage_inputs(k)
    K64 = T.spectrum(traj, h, w, wgt)
    e = planned(4, naive=form == "composed", weights=False)
    Sd = g_c64(Sn)
    e.set_kspace_ncsense_tz(g_c64(ys), Sd, g_f32(wgt), cg_iters=K)
    assert e.toeplitz_live and e.ncsense_coils == 9
    with pytest.raises(_lib.PnPError):
        e.nc_cg_residual()
    en = TS.planned(k)
    en.set_kspace_ncsense(g_c64(ys), Sd, g_f32(wgt), cg_iters=K)
    _check_stage(e, en, K64, P, Sn, xr, z0, u0, wgt, ys, SR.AH(P, ys, Sn, wgt), K, lambda g, p, m: g.ncsense_normal(p, m),
                 lambda g: g.ncsense_cg_residual(), f"ns {form}")


# ---- modes, state, workspace ------------------------------------------------------------------------------------------------------------------

class TzEpisode:
    """an episode of tests/handle_cases.py ("nc") or tests/test_gpu_ncsense.py ("ns") whose CG runs the Toeplitz operator"""

    def __init__(self, mode):
        self.mode = mode
        self.ep = TS._episode("nc" if mode == "tznc" else "ns")
        self.n, self.h, self.w = self.ep.n, self.ep.h, self.ep.w

    def plan(self, e):
        self.ep.plan(e)

    def reset(self, e):
        self.plan(e)
        p = self.ep
        if self.mode == "tznc":
            return e.reset_nc_tz(p.x0, p.y, p.dcf, cg_iters=p.cg_iters)
        return e.reset_ncsense_tz(p.x0, p.y, p.sens, p.dcf, cg_iters=p.cg_iters)

    def reinstall(self, e):
        self.plan(e)
        p = self.ep
        if self.mode == "tznc":
            e.set_kspace_nc_tz(p.y, p.dcf, cg_iters=p.cg_iters)
        else:
            e.set_kspace_ncsense_tz(p.y, p.sens, p.dcf, cg_iters=p.cg_iters)

    def cg_residual(self, e):
        return self.ep.cg_residual(e)


TZ = ("tznc", "tzns")


def _episode(mode):
    return TzEpisode(mode) if mode in TZ else TS._episode(mode)


_FRESH = {}


def fresh(mode):
    """two steps of the episode on a fresh handle"""
    if mode not in TZ:
        return TS.fresh(mode)
    if mode not in _FRESH:
        ep = _episode(mode)
        e = TS._tv(_engine(ep.n, ep.h, ep.w))
        _FRESH[mode] = TS._steps(e, ep, ep.reset(e), 0, 2)
    return _FRESH[mode]


@pytest.mark.parametrize("tz", TZ)
def test_mode_switches_to_and_from_every_other_mode_give_a_fresh_handles_bits(tz):
    mine = _episode(tz)
    # the Toeplitz stage is not the NUFFT stage under another name: the iterates differ
    assert HC.differing(fresh(tz)[1], fresh("nc" if tz == "tznc" else "ns")[1]) > 0
    for other in ("sc", "mc", "nc", "ns", TZ[1 - TZ.index(tz)]):
        ep = _episode(other)
        e = TS._tv(_engine(mine.n, mine.h, mine.w))
        TS._steps(e, mine, mine.reset(e), 0, 1)
        assert e.toeplitz_live
        TS._assert_same(TS._steps(e, ep, ep.reset(e), 0, 2), fresh(other), f"{other} after {tz}")
        assert e.toeplitz_live == (other in TZ)                                     # every other installer leaves Toeplitz
        TS._assert_same(TS._steps(e, mine, mine.reset(e), 0, 2), fresh(tz), f"{tz} after {other}")
        assert e.toeplitz_live and e.ncsense_coils == (4 if tz == "tzns" else 0)


def _new_intruders(e, f, own_plan, plan_spectrum):
    """the INTRUDER entries of the new table on foreign data (2 and 9 coils); a handle without a spectrum gets one first"""
    if own_plan:
        e.nufft_plan(f.traj, width=4)
    if plan_spectrum:
        e.toeplitz_plan(None)
    out = {"spectrum": e.toeplitz_spectrum(), "apply": e.toeplitz_apply(f.cimg)}
    if f.n > 1:
        out["apply n-1"] = e.toeplitz_apply(f.cimg[:f.n - 1].contiguous())
    for c in (2, 9):
        out[f"C={c} apply_mc"] = e.toeplitz_apply_mc(f.cimg, HC.c64(synthetic.coil_maps(c, f.h, f.w, radius=1.5, width=1.0)))
    return out


@pytest.mark.parametrize("mode", ("sc", "mc", "nc", "ns") + TZ)
def test_the_new_intruders_between_two_steps_of_an_episode_change_nothing(mode):
    ep = _episode(mode)
    f = HC.Foreign(ep.n, ep.h, ep.w)
    e = TS._tv(_engine(ep.n, ep.h, ep.w))
    outs = []

    def between():
        outs.append(_new_intruders(e, f, mode in ("sc", "mc"), mode not in TZ))
        assert e.toeplitz_live == (mode in TZ)

    got = TS._steps(e, ep, ep.reset(e), 0, 2, between=between)
    TS._assert_same(got, fresh(mode), f"{mode} with the new intruders")
    if mode in TZ:                                                                  # what they return does not depend on the episode either
        bare = _engine(ep.n, ep.h, ep.w)
        ep.plan(bare)
        bare.toeplitz_plan(ep.ep.dcf)
        HC.compare_outputs(outs[0], _new_intruders(bare, f, False, False), f"new intruders in a {mode} episode")


@pytest.mark.parametrize("tz", TZ)
def test_the_existing_intruders_between_two_steps_of_a_toeplitz_episode_change_nothing(tz):
    ep = _episode(tz)
    f = HC.Foreign(ep.n, ep.h, ep.w)
    e = TS._tv(_engine(ep.n, ep.h, ep.w))
    it = ep.reset(e)
    ran = []

    def between():
        t = torch.zeros(ep.n, dtype=torch.float32, device=DEV)
        ctx = HC.Ctx(f, "nc", tuple(it) + (t,), False, False)                      # "nc": the intruders use the live plan
        refused = {"pnp_mc_normal"} | ({"pnp_nc_normal"} if tz == "tzns" else set())
        for name, covers, applies, call in HC.INTRUDERS:
            if applies(ctx) and not refused & set(covers):
                call(e, ctx)
                ran.append(name)
        TS._new_intruders(e, f, False)                                              # and those of the non-Cartesian SENSE header
        assert e.toeplitz_live

    got = TS._steps(e, ep, it, 0, 2, between=between)
    print(f"intruders run in a {tz} episode: {ran}")
    assert len(ran) >= 9
    TS._assert_same(got, fresh(tz), f"{tz} with the existing intruders")


def test_every_tz_installer_followed_by_a_reinstall_restores_the_bits():
    for tz in TZ:                                                                   # the existing installers (and a re-plan) in a Toeplitz episode
        mine = _episode(tz)
        f = HC.Foreign(mine.n, mine.h, mine.w)
        for name, _, replace in HC.REPLACERS:
            e = TS._tv(_engine(mine.n, mine.h, mine.w))
            got = TS._steps(e, mine, mine.reset(e), 0, 1)
            replace(e, f)
            assert not e.toeplitz_live, name
            mine.reinstall(e)
            TS._assert_same(TS._steps(e, mine, got[:3], 1, 1)[:4], fresh(tz)[:4], f"{tz} after {name} and a re-install")
    S8 = HC.c64(synthetic.coil_maps(8, f.h, f.w))
    for mode in ("sc", "mc", "nc", "ns") + TZ:                                      # the new installers in an episode of every kind
        for which in ("set_kspace_nc_tz", "reset_nc_tz", "set_kspace_ncsense_tz", "reset_ncsense_tz"):
            ep = _episode(mode)
            e = TS._tv(_engine(ep.n, ep.h, ep.w))
            got = TS._steps(e, ep, ep.reset(e), 0, 1)
            if not e.nufft_samples:
                e.nufft_plan(f.traj, width=4)
            m = e.nufft_samples
            samples, wts = f.samples(m)
            y8 = HC.c64(HC._cuniform(f.seed, 90, (ep.n, 8, m)))
            if which == "set_kspace_nc_tz":
                e.set_kspace_nc_tz(samples, wts, cg_iters=3)
            elif which == "reset_nc_tz":
                e.reset_nc_tz(f.x1, samples, None, cg_iters=2)
            elif which == "set_kspace_ncsense_tz":
                e.set_kspace_ncsense_tz(y8, S8, wts, cg_iters=3)
            else:
                e.reset_ncsense_tz(f.x1, y8, S8, None, cg_iters=2)
            assert e.toeplitz_live and e.coils == 0 and e.ncsense_coils == (8 if "ncsense" in which else 0)
            ep.reinstall(e)
            assert e.toeplitz_live == (mode in TZ)
            TS._assert_same(TS._steps(e, ep, got[:3], 1, 1)[:4], fresh(mode)[:4], f"{mode} after {which} and a re-install")


def test_replanning_drops_what_the_header_says_it_drops():
    for tz in TZ:
        ep = _episode(tz)
        e = TS._tv(_engine(ep.n, ep.h, ep.w))
        x, z, u = ep.reset(e)
        mu = HC.f32(np.full(ep.n, 0.3))
        e.prox_dual(x, z, u, mu)
        e.toeplitz_plan(None)                                                       # a live Toeplitz stage: its constants go with the old spectrum
        assert e.toeplitz_planned and not e.toeplitz_live and e.ncsense_coils == 0
        with pytest.raises(_lib.PnPError, match="pnp_reset"):
            e.prox_dual(x, z, u, mu)
        with pytest.raises(_lib.PnPError):
            ep.cg_residual(e)
        ep.reset(e)
        assert e.toeplitz_live
        e.nufft_plan(ep.ep.traj, width=6)                                           # a new plan drops the spectrum and the stage
        assert not e.toeplitz_planned and not e.toeplitz_live
        with pytest.raises(_lib.PnPError, match="no Toeplitz spectrum"):
            e.toeplitz_spectrum()
        with pytest.raises(_lib.PnPError, match="pnp_reset"):
            e.prox_dual(x, z, u, mu)
    # a stage that is not Toeplitz keeps its constants when a spectrum is planned beside it
    ep = _episode("nc")
    e = TS._tv(_engine(ep.n, ep.h, ep.w))
    got = TS._steps(e, ep, ep.reset(e), 0, 1)
    e.toeplitz_plan(ep.dcf)
    TS._assert_same(TS._steps(e, ep, got[:3], 1, 1)[:4], fresh("nc")[:4], "nc with a spectrum planned between two steps")


def test_launch_counts_of_one_normal_operator():
    """by the profile counters (rows, cols, other), as tests/test_gpu_kspace_launches.py counts them"""
    ep = _episode("tznc")
    want = {"fused": (2, 1, 0), "composed": (2, 2, 3)}
    for form in FORMS:
        e = _engine(ep.n, ep.h, ep.w, naive=form == "composed", profile=True)
        ep.reset(e)
        e.profile_reset()
        e.nc_normal(ep.ep.x0, HC.f32(np.full(ep.n, 0.3)))
        torch.cuda.synchronize()                                                    # the event pairs are read after they completed
        p = e.profile_collect()
        got = (p["fft_rows"]["launches"], p["fft_cols_prox"]["launches"], p["other"]["launches"])
        print(f"{form}: one single-coil Nop = (rows, cols, other) {got}")
        assert got == want[form]
    e = _engine(1, 80, 80, profile=True)                                            # a mixed-radix padded grid (160): the composed form
    e.nufft_plan(ref(5)[0], width=6)
    e.toeplitz_plan(None)
    e.profile_reset()
    e.toeplitz_apply(g_c64(ref(5)[2]))
    torch.cuda.synchronize()
    p = e.profile_collect()
    assert (p["fft_rows"]["launches"], p["fft_cols_prox"]["launches"], p["other"]["launches"]) == want["composed"]


@pytest.mark.parametrize("form", FORMS)
def test_state_errors_argument_errors_and_workspace_accounting(form):
    i = 2                                                                           # 2 slices of 32 x 16
    traj, wgt, x, K, B = ref(i)
    n, h, w = T.case_shape(i)
    m = traj.shape[0]
    c = 9
    e = _engine(n, h, w, naive=form == "composed")
    img, Sd = g_c64(x), g_c64(synthetic.coil_maps(c, h, w))
    smp = g_c64(np.zeros((n, m), dtype=np.complex64))
    for call in (lambda: e.toeplitz_plan(None), lambda: e.toeplitz_spectrum(), lambda: raw_apply(e, img), lambda: raw_apply_mc(e, img, Sd)):
        with pytest.raises(_lib.PnPError, match="no NUFFT plan"):
            call()
    e.nufft_plan(traj, grid=NR.CASES[i][3:5], width=NR.CASES[i][5])
    lib, hd, st = e.lib, e._h, e._stream()
    out = GB.guarded((n, h, w), torch.complex64, DEV)
    xg, zg = GB.guarded((n, 1, h, w), torch.float32, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
    ws0 = e.workspace_bytes
    no_spectrum = [
        lambda: lib.pnp_toeplitz_spectrum(hd, out.data_ptr(), st), lambda: lib.pnp_toeplitz_apply(hd, img.data_ptr(), n, out.data_ptr(), st),
        lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), c, 1, n, out.data_ptr(), st),
        lambda: lib.pnp_set_kspace_nc_tz(hd, smp.data_ptr(), 4, st),
        lambda: lib.pnp_reset_nc_tz(hd, img.data_ptr(), smp.data_ptr(), 4, xg.data_ptr(), zg.data_ptr(), out.data_ptr(), st),
        lambda: lib.pnp_set_kspace_ncsense_tz(hd, smp.data_ptr(), Sd.data_ptr(), 1, 1, 4, st),
        lambda: lib.pnp_reset_ncsense_tz(hd, img.data_ptr(), smp.data_ptr(), Sd.data_ptr(), 1, 1, 4, xg.data_ptr(), zg.data_ptr(), out.data_ptr(), st)]
    with GB.watch(outputs={"out": out, "x": xg, "z": zg}, inputs={"out": out, "x": xg, "z": zg, "img": img}):
        for j, call in enumerate(no_spectrum):
            assert call() == -3 and b"no Toeplitz spectrum" in lib.pnp_last_error(), (j, lib.pnp_last_error())      # PNP_ERR_STATE
        assert lib.pnp_toeplitz_plan(hd, None, 1, st) == -1 and b"flags" in lib.pnp_last_error()
    assert e.workspace_bytes == ws0 and not e.toeplitz_planned
    # the plan: K 16 H W, the weights copy 4 M (none for NULL), the trajectory 16 M, the twiddles 16 (H + W), the pass buffer 32 N H W
    # (the composed form's 2H x 2W grids; the fused form keeps the H live rows only: 16 N H W)
    per = 16 if form == "fused" else 32
    e.toeplitz_plan(None)
    want = 16 * h * w + 16 * m + 16 * (h + w) + per * n * h * w
    print(f"{form}: pnp_toeplitz_plan(NULL) grew the workspace by {e.workspace_bytes - ws0} bytes, documented {want}")
    assert e.workspace_bytes - ws0 == want
    e.toeplitz_plan(g_f32(wgt))
    assert e.workspace_bytes - ws0 == want + 4 * m
    e.toeplitz_plan(g_f32(wgt))
    assert e.workspace_bytes - ws0 == want + 4 * m
    ws1 = e.workspace_bytes
    bad = [
        (lambda: lib.pnp_toeplitz_apply(hd, img.data_ptr(), n + 1, out.data_ptr(), st), "batch"),
        (lambda: lib.pnp_toeplitz_apply(hd, img.data_ptr(), 0, out.data_ptr(), st), "batch"),
        (lambda: lib.pnp_toeplitz_apply(hd, out.data_ptr(), n, out.data_ptr(), st), "alias"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), 0, 1, n, out.data_ptr(), st), "coils"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), 33, 1, n, out.data_ptr(), st), "coils"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), c, 3, n, out.data_ptr(), st), "sens_n"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), c, 1, n + 1, out.data_ptr(), st), "batch"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), Sd.data_ptr(), c, 1, n, img.data_ptr(), st), "alias"),
        (lambda: lib.pnp_toeplitz_apply_mc(hd, img.data_ptr(), None, c, 1, n, out.data_ptr(), st), "null sens"),
        (lambda: lib.pnp_toeplitz_spectrum(hd, None, st), "null out"),
        (lambda: lib.pnp_toeplitz_plan(hd, None, 2, st), "flags"),
        (lambda: lib.pnp_set_kspace_nc_tz(hd, smp.data_ptr(), 0, st), "cg_iters"),
        (lambda: lib.pnp_set_kspace_nc_tz(hd, None, 4, st), "null y"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(hd, smp.data_ptr(), Sd.data_ptr(), c, 3, 4, st), "sens_n"),
        (lambda: lib.pnp_reset_ncsense_tz(hd, img.data_ptr(), smp.data_ptr(), Sd.data_ptr(), c, 1, 65, xg.data_ptr(), zg.data_ptr(), out.data_ptr(), st),
         "cg_iters"),
    ]
    with GB.watch(outputs={"out": out, "x": xg, "z": zg}, inputs={"out": out, "x": xg, "z": zg, "img": img, "sens": Sd}):
        for call, what in bad:
            assert call() == -1 and what.encode() in lib.pnp_last_error(), (what, lib.pnp_last_error())
    assert e.workspace_bytes == ws1 and e.toeplitz_planned and not e.toeplitz_live
    raw_apply(e, img)
    assert e.workspace_bytes == ws1                                                 # the single-coil application allocates nothing
    # a multi-coil application: the pass buffer grows to N cb planes, cb = min(C, 8), and the block's coil images 8 N cb H W come with it
    raw_apply_mc(e, img, Sd)
    want = per * n * 8 * h * w - per * n * h * w + 8 * n * 8 * h * w
    print(f"{form}: pnp_toeplitz_apply_mc (C = {c}) grew the workspace by {e.workspace_bytes - ws1} bytes, documented {want}")
    assert e.workspace_bytes - ws1 == want
    raw_apply_mc(e, img, Sd)
    assert e.workspace_bytes - ws1 == want
    # a side above 512: refused in the words that name the limit, before anything is allocated
    big = _engine(1, 640, 16)
    big.nufft_plan(NR.radial(640, 16, 3), width=4)
    ws = big.workspace_bytes
    with pytest.raises(_lib.PnPError, match="h, w up to 512"):
        big.toeplitz_plan(None)
    assert big.workspace_bytes == ws and not big.toeplitz_planned
    assert str(_lib.toeplitz_size_error("pnp_toeplitz_plan", 640, 16)).encode() in big.lib.pnp_last_error()


# ---- end to end, and the command line --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("single-coil", "multi-coil"))
def test_end_to_end_tv_admm_through_the_fixed_schedule_solver_with_the_toeplitz_operator(which, record_property):
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    import tv_ref
    R, run, recorded = (NR, T.admm_tv_nc, T.FIXTURE_PSNR) if which == "single-coil" else (SR, T.admm_tv_ncmc, T.FIXTURE_PSNR_MC)
    t = R.FIXTURE
    d, P = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    x64, p0, p64 = run(d, P, mu, sig, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"{which}: float64 Toeplitz restatement: PSNR of x0 {p0}, final {p64} dB (recorded {recorded})")
    assert abs(p64[0] - recorded[1]) <= 2e-3
    env = PnPEnv(max_episode_step=t["iters"], denoiser=TVDenoiser2D(scale=t["tv_scale"], iters=t["tv_iters"]), device_type="cuda",
                 cg_iters=t["cg_iters"], nufft_width=t["width"], nc_normal="toeplitz")
    r = FixedScheduleSolver(env, max_iter=t["iters"], dc=True).run(TN._mat(d), np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    assert env._engine.toeplitz_live and env._engine.ncsense_coils == (0 if which == "single-coil" else t["coils"])
    gt = d["gt"][:, 0].astype(np.float64)
    pdev = tv_ref.psnr(_np(r.x)[:, 0], gt)
    dp, dx = float(np.abs(pdev - p64).max()), float(np.abs(_np(r.x)[:, 0] - x64).max())
    print(f"{which}: device PSNR of x0 {r.initial_psnr.reshape(-1).tolist()}, final {pdev} (engine's own {r.psnr.reshape(-1).tolist()}), "
          f"|dPSNR| {dp:.3e} dB, max |dx| {dx:.3e}, dc {r.dc.tolist()}")
    record_property("max_abs_dpsnr_db", dp)
    assert dp <= 0.01
    assert abs(float(r.psnr.reshape(-1)[0]) - float(p64[0])) <= 0.01


def test_cli_traj_radial_nc_normal_toeplitz_fixed_on_a_ground_truth_folder(tmp_path):
    from dt4image_restoration_amd import cli
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5), synthetic.phantom(64, 64, 6)]).astype(np.float32))
    base = ["--block_size", "6", "--n_embeds", "9", "--gt", str(gtd), "--tasks", "4x_5", "--prior", "tv", "--seed", "3"]
    with pytest.raises(SystemExit, match="needs --traj radial"):
        cli.main(base + ["--nc-normal", "toeplitz", "fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit, match="h, w up to 512"):
        cli.main(["--block_size", "6", "--n_embeds", "9", "--prior", "tv", "--traj", "radial", "--nc-normal", "toeplitz", "--size", "640",
                  "fixed", "--max_iter", "2"])

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = cli.main(base + ["--traj", "radial"] + extra + ["fixed", "--max_iter", "10", "--dc"])
        lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
        assert lines == out and len(out) == 1 and out[0]["n"] == 2 and "radial-nc" in out[0]["set"]
        return out[0]

    a, an = run(["--nc-normal", "toeplitz"]), run([])
    b = run(["--nc-normal", "toeplitz", "--nc-coils", "2"])
    print(f"cli --traj radial --nc-normal toeplitz fixed: {a['psnr']:.3f} dB (+{a['psnr_increment']:.3f}; the NUFFT stage {an['psnr']:.3f} dB), "
          f"--nc-coils 2: {b['psnr']:.3f} dB (+{b['psnr_increment']:.3f}); dc {a['dc']:.4f} {b['dc']:.4f}")
    for r in (a, b):
        assert np.isfinite(r["psnr"]) and r["psnr_increment"] > 1.0 and r["dc"] > 0.0
    assert abs(a["psnr"] - an["psnr"]) <= 0.05                                      # the exact operator and its 6e-4 model restore alike
    assert sorted(TC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_TOEPLITZ)
