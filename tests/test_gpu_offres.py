"""Off-resonance correction on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against tests/offres_ref.py: the exact
operator, the time-segmented model with a dense DFT, and the model on the NUFFT plan for the CG stage.  Every buffer handed to the new entry
points in the guard-band test comes from tests/guard_bands.py.  Every figure is printed before it is asserted.  No bound here is measured on
the device.

BOUNDS.
  Exact anchors, naive against shipped form, invariance: torch.equal (numbers; the sign of a zero does not count) or the bits.
  Maps: one float32 ulp of 1.0, 1.2e-7 absolute, against the float64 restatement.
  Model: against the dense segmented restatement the difference is the NUFFT's: relative l2 <= 1e-6 + twice the host test's model error
  for the width and grid ratio (tests/test_nufft_host.py: J = 4: 1.138e-03 at 2x, 1.224e-02 at 1.25x; J = 6: 1.327e-05, 5.938e-04), as
  tests/test_gpu_nufft.py asserts its acquisition.  Against the exact operator, per sample: that tolerance times ||ref|| (an l2 figure bounds
  every sample's error) plus the derived bound (1 - cos(omega_max D / 2)) ||p||_1.
  Rounding level: against the float64 model on the NUFFT plan with the device's own maps (offres_ref.model_forward / model_adjoint), the
  bounds of tests/test_gpu_nufft.py per segment plane, joined as `forward_err_norm` / `adjoint_err` say, the way tests/test_gpu_ncsense.py
  joins them over coils.  Adjointness: that model is exactly adjoint (the pair shares its weights), so <A p, W q> - <p, A^H W q> on the
  device outputs is <df, W q> - <p, da>, at most ||Bf|| ||W q|| + ||p|| ||Ba||: tests/test_gpu_ncsense.py's bound.
  Stage: the tolerances of tests/test_gpu_ncsense.py (ten times the float32 restatement of the CG at mu = 0.3, K = 4; the DC column's
  1e-6 s sqrt(wmax) ||x|| + 5e-7 dc).
  The correction corrects (32 x 32 spiral, omega_max span = 3 pi, TV, 30 steps): PSNR and DC figures are printed; the orderings are asserted.
  `offres_segments(tol = 1e-3)` asks for 107 segments there, the library takes 32: the test runs L = 32 and its bound is that L's.

MEASURED on one MI355X: maps 3.0e-08 from float64; forward / adjoint relative l2 against the dense segmented
restatement 1.3e-05 (16 x 16, J = 6), 1.1e-05 (32 x 32, J = 6), 1.1e-03 (32 x 32, J = 4), 9.2e-03 (80 x 64, J = 4), 4.7e-04 (80 x 64, J = 6),
6.0e-04 (128 x 128, J = 6), 1.4e-02 (128 x 128, J = 4): 0.38 to 0.56 of the tolerance; against the float64 model on the
plan: forward ||err|| 2.6e-06 .. 1.3e-05 (bounds 2.9e-04 .. 3.7e-03), adjoint at most 0.013 of its bound, adjointness 1.0e-09 .. 9.4e-09 of
||p|| ||q||; CG stage with density weights err_max 1.3e-06 .. 2.3e-06 of 9.99e-06, with weights in [0.5, 1.5] (||A^H W A|| 14.2 against 5.4:
tolerances times 2.516) 4.8e-06 .. 1.2e-05 of 2.51e-05; DC column 5.5e-08 of 1.3e-04; the correction: 50.549 dB against 17.735 dB for the plain stage (the float64
restatement on the CPU gives the same two figures), DC at x = gt 2.33e-02 and 9.13 around the bound 1.99."""
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
import offres_cases as OC  # noqa: E402
import offres_ref as OR  # noqa: E402
import test_gpu_nufft as TN  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
MARGIN = 10.0
F32_MU03_K4 = (9.992e-07, 3.740e-07, 2.784e-07)              # tests/test_gpu_sense.py's float32 restatement of the CG
MODEL_ERR = {(4, 2.0): 1.138e-03, (4, 1.25): 1.224e-02, (6, 2.0): 1.327e-05, (6, 1.25): 5.938e-04}      # tests/test_nufft_host.py
GRIDS = {(16, 16): (32, 32), (32, 32): (64, 64), (80, 64): (128, 80), (128, 128): (160, 160)}


def model_tol(h, w, J):
    gh, gw = GRIDS[(h, w)]
    ratio = 1.25 if min(gh / h, gw / w) < 2.0 else 2.0         # an axis below 2x takes the 1.25x figure
    return 1e-6 + 2.0 * MODEL_ERR[(J, ratio)]


def gamma(k):
    return k * U / (1.0 - k * U)


def forward_err_norm(P, Q, E, x, ref):
    """||Bf|| per slice against offres_ref.model_forward: per segment plane the forward bound of tests/test_gpu_nufft.py (the grid
    transform's error gathered through the footprint plus the rounding of the J^2-term chain), weighted by the sample's b_l; the rounding of
    the segment image E_l . p (three roundings, through an operator of norm s_nu; b0^2 + b1^2 <= 1 joins the planes in l2); two roundings
    of the blend"""
    n = x.shape[0]
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    B = OR.weights(Q)
    per = sum(B[l] * TN.forward_bound(P, E4[:, l] * x) for l in range(Q["L"]))
    img = math.sqrt(Q["L"]) * np.linalg.norm(x.reshape(n, -1), axis=1)              # sqrt(sum_l ||E_l . p||^2), |E_l| = 1
    return np.linalg.norm(per, axis=1) + NR.op_norm(P) * gamma(3) * img + gamma(2) * np.linalg.norm(ref, axis=1)


def adjoint_err(P, Q, E, y, wgt):
    """|Ba| per pixel [N,H,W] against offres_ref.model_adjoint: per segment the adjoint bound of tests/test_gpu_nufft.py on the samples
    b_l . q (the product's one more rounding before the chain is inside that bound's 2 k), through |E_l|, plus the 4 L roundings of the
    combine chain on the sum of the planes' magnitudes"""
    n = y.shape[0]
    E4 = np.broadcast_to(E, (n,) + E.shape[-3:])
    B = OR.weights(Q)
    out = np.zeros((n, P["h"], P["w"]))
    for l in range(Q["L"]):
        yl = B[l] * y
        out += np.abs(E4[:, l]) * (TN.adjoint_bound(P, yl, wgt)[0] + gamma(4 * Q["L"]) * np.abs(NR.adjoint(P, yl, wgt)))
    return out


def c64(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.complex64).to(DEV)
    return t.reshape(shape).contiguous() if shape else t.contiguous()


def f32(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(DEV)
    return t.reshape(shape).contiguous() if shape else t.contiguous()


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
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _rt(a):
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def _engine(n, h, w, monkeypatch=None, naive=None, block=None):
    from dt4image_restoration_amd.engine import PnPEngine
    if monkeypatch is not None:
        for name, v in (("PNP_OFFRES_NAIVE", naive), ("PNP_OFFRES_SEG_BLOCK", block)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(int(v)))
    return PnPEngine(n, h, w, device=0, denoiser=False)


_SETUP = {}


def setup(h, w, kind, J, hz=100.0, t_read=10e-3):
    """(traj, times, plan of the NUFFT restatement, omega [3,h,w] float32 rad/s per slice), computed once"""
    key = (h, w, kind, J, hz, t_read)
    if key not in _SETUP:
        traj, m, R = OR.case_traj(kind, h, w)
        times = acquisition.readout_times(kind, m, R, t_read, te=1e-3)
        gh, gw = GRIDS[(h, w)]
        _SETUP[key] = (traj, times, NR.plan(h, w, gh, gw, J, traj), OR.case_omega(h, w, hz, 5, n=3))
    return _SETUP[key]


def planned(n, h, w, kind, J, L, times=None, monkeypatch=None, naive=None, block=None):
    traj, t, P, _ = setup(h, w, kind, J)
    e = _engine(n, h, w, monkeypatch, naive, block)
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=J)
    e.offres_plan(t if times is None else times, L)
    return e


def _data(n, h, w, m, seed=0):
    rng = np.random.default_rng(900 + seed)
    x = _rt(rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w)))
    y = _rt(rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m)))
    wgt = (0.5 + rng.random(m)).astype(np.float32)
    return x, y, wgt


# ---- exact anchors ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,J,n", ((16, 16, "radial", 6, 2), (80, 64, "spiral", 4, 3)))
def test_one_segment_has_the_bits_of_the_multicoil_pair_at_one_coil(h, w, kind, J, n):
    traj, t, P, om = setup(h, w, kind, J)
    e = planned(n, h, w, kind, J, 1)
    assert e.offres_segments == 1 and not e.offres_live
    x, y, wgt = _data(n, h, w, P["m"])
    for omega in (om[0], om[:n]):                                                   # a shared map, a map per slice
        maps = e.offres_maps(f32(omega))
        sens = maps.reshape((1, h, w) if omega.ndim == 2 else (n, 1, h, w))
        assert _same(e.offres_forward(c64(x), maps), e.nufft_forward_mc(c64(x), sens)[:, 0])
        for wd in (None, f32(wgt)):
            assert _same(e.offres_adjoint(c64(y), maps, wd), e.nufft_adjoint_mc(c64(y).reshape(n, 1, -1), sens, wd))


@pytest.mark.parametrize("L,J", ((2, 6), (3, 4), (8, 6), (32, 4)))
def test_samples_on_segment_centres_equal_the_multicoil_pair_as_numbers(L, J):
    h = w = 32
    n = 2
    traj, _, P, om = setup(h, w, "spiral", J)
    m = P["m"]
    t = ((np.arange(m) * 7) % L) * 2.0 ** -10                                       # D = 2^-10: every t_m on a centre, every centre taken
    Q = OR.plan(t, L)
    assert Q["step"] == 2.0 ** -10 and set(np.unique(Q["b1"])) <= {0.0, 1.0} and len(np.unique(Q["seg"] + Q["b1"].astype(int))) == L
    e = planned(n, h, w, "spiral", J, L, times=t)
    x, y, wgt = _data(n, h, w, m, seed=L)
    maps = e.offres_maps(f32(om[0] * 50.0))                                         # omega tau stays moderate at tau ~ 1e-3 .. 3e-2
    coil = torch.from_numpy(Q["seg"] + Q["b1"].astype(np.int32)).to(DEV).long()
    fmc = e.nufft_forward_mc(c64(x), maps)                                          # [n, L, m]
    want = fmc.gather(1, coil.reshape(1, 1, m).expand(n, 1, m))[:, 0]
    got = e.offres_forward(c64(x), maps)
    assert torch.equal(got, want)
    ys = torch.zeros((n, L, m), dtype=torch.complex64, device=DEV)
    ys.scatter_(1, coil.reshape(1, 1, m).expand(n, 1, m), c64(y).reshape(n, 1, m))
    for wd in (None, f32(wgt)):
        assert torch.equal(e.offres_adjoint(c64(y), maps, wd), e.nufft_adjoint_mc(ys, maps, wd))


def _run_all(e, h, w, kind, J, L, sl, omega, mu_all, steps=3):
    """every output of the new entry points for the slices `sl`: forward, adjoint, normal, x, z, u after `steps` TV steps, dc, cg_res, acquire"""
    traj, t, P, om = setup(h, w, kind, J)
    n_all = len(mu_all)
    x, y, wgt = _data(n_all, h, w, P["m"], seed=3)
    cnt = sl.stop - sl.start
    od = f32(omega)
    maps = e.offres_maps(od)
    f = e.offres_forward(c64(x[sl]), maps)
    a = e.offres_adjoint(c64(y[sl]), maps, f32(wgt))
    gt = np.stack([synthetic.phantom(h, w, 60 + j) for j in range(n_all)]).astype(np.float32)
    acq = e.acquire_offres(f32(gt[sl], (cnt, 1, h, w)), od, 0.02, 41 + sl.start, dcf=f32(wgt))
    xs, zs, us = e.reset_offres(acq[2].clone(), acq[0].clone(), od, f32(wgt), cg_iters=3)
    q = e.offres_normal(c64(x[sl], (cnt, 1, h, w)), f32(mu_all[sl]))
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    for _ in range(steps):
        e.step(xs, zs, us, f32(mu_all[sl]), f32(np.full(cnt, 0.05, dtype=np.float32)))
    dc = e.residuals(xs, zs, us, dc=True)
    return f, a, q, xs, zs, us, dc, e.offres_cg_residual(), torch.cat([v.reshape(cnt, -1) for v in acq], dim=1)


NAMES = "forward adjoint normal x z u residuals cg_res acquire".split()
MU3 = np.array([0.3, 0.05, 0.6], dtype=np.float32)


@pytest.mark.parametrize("h,w,kind,J,L", ((128, 128, "spiral", 6, 8), (32, 32, "radial", 4, 3), (16, 16, "spiral", 6, 32), (80, 64, "radial", 4, 2)))
def test_the_shipped_form_equals_the_naive_form_for_every_segment_block(h, w, kind, J, L, monkeypatch):
    n = 2
    om = setup(h, w, kind, J)[3][:n]
    outs = {}
    for naive in (0, 1):
        for block in (1, 3, None):
            e = planned(n, h, w, kind, J, L, monkeypatch=monkeypatch, naive=naive, block=block)
            outs[(naive, block)] = _run_all(e, h, w, kind, J, L, slice(0, n), om, MU3[:n])
    ref = outs[(1, None)]
    assert all(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all() for v in ref)
    for key, got in outs.items():
        for name, a, b in zip(NAMES, ref, got):
            assert torch.equal(a, b), (name, key)
        if key[0] == 1:                                                             # within one form the block size changes no bit
            for name, a, b in zip(NAMES, ref, got):
                assert _same(a, b), (name, key)
    for name, a, b in zip(NAMES, outs[(0, None)], outs[(0, 1)]):
        assert _same(a, b), name
    for name, a, b in zip(NAMES, outs[(0, None)], outs[(0, 3)]):
        assert _same(a, b), name
    dflt = _run_all(planned(n, h, w, kind, J, L, monkeypatch=monkeypatch), h, w, kind, J, L, slice(0, n), om, MU3[:n])
    for name, a, b in zip(NAMES, ref, dflt):                                        # whatever mix ships
        assert torch.equal(a, b), name
    monkeypatch.setenv("PNP_OFFRES_GRID_FILTER", "1")                               # the gridding's other layout: the tile's whole bin, filtered
    filt = _run_all(planned(n, h, w, kind, J, L, monkeypatch=monkeypatch, naive=0), h, w, kind, J, L, slice(0, n), om, MU3[:n])
    monkeypatch.delenv("PNP_OFFRES_GRID_FILTER")
    for name, a, b in zip(NAMES, outs[(0, None)], filt):
        assert torch.equal(a, b), name


# ---- maps ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", (1, 3, 32))
def test_maps_are_within_one_ulp_of_the_float64_restatement(L):
    h, w, n = 80, 64, 3
    traj, t, P, om = setup(h, w, "spiral", 4)
    e = planned(n, h, w, "spiral", 4, L)
    Q = OR.plan(t, L)
    for omega in (om[1], om):
        got = _np(e.offres_maps(f32(omega)))
        ref = OR.maps(omega.astype(np.float64), Q)
        err = float(max(np.abs(got.real - ref.real).max(), np.abs(got.imag - ref.imag).max()))
        print(f"L = {L}, map_n = {1 if omega.ndim == 2 else n}: max |maps - float64| {err:.3e} (bound 1.2e-7), max |omega tau| {np.abs(omega).max() * Q['tau'].max():.2f} rad")
        assert got.shape == ref.shape and err <= 1.2e-7


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,J,L,n", ((16, 16, "radial", 6, 2, 1), (32, 32, "spiral", 6, 3, 2), (32, 32, "radial", 4, 8, 3),
                                            (80, 64, "spiral", 4, 3, 2), (80, 64, "radial", 6, 32, 1), (128, 128, "spiral", 6, 8, 2),
                                            (128, 128, "radial", 4, 1, 1)))
def test_forward_and_adjoint_against_the_segmented_and_the_exact_restatement(h, w, kind, J, L, n):
    traj, t, P, om = setup(h, w, kind, J)
    m = P["m"]
    e = planned(n, h, w, kind, J, L)
    Q = OR.plan(t, L)
    x, y, wgt = _data(n, h, w, m, seed=L)
    omega = om[:n].astype(np.float64)
    maps = e.offres_maps(f32(om[:n]))
    got_f, got_a = _np(e.offres_forward(c64(x), maps)), _np(e.offres_adjoint(c64(y), maps, f32(wgt)))
    ref_f, ref_a = OR.segmented_forward(traj, Q, omega, x), OR.segmented_adjoint(traj, Q, omega, y, h, w, wgt)
    tol = model_tol(h, w, J)
    rf = float(np.linalg.norm(got_f - ref_f) / np.linalg.norm(ref_f))
    ra = float(np.linalg.norm(got_a - ref_a) / np.linalg.norm(ref_a))
    print(f"{h}x{w} {kind} J={J} L={L}: forward rel l2 {rf:.3e}, adjoint rel l2 {ra:.3e} (tolerance {tol:.3e})")
    assert rf <= tol and ra <= tol
    if L > 1:
        ex = OR.exact_forward(traj, t, omega, x)
        om_max = float(np.abs(omega).max())
        bnd = tol * np.linalg.norm(ref_f.reshape(n, -1), axis=1) + OR.bound(om_max, Q["step"], x)
        err = np.abs(got_f - ex).max(axis=1)
        print(f"        against the exact operator: max |err| {err.tolist()} bound {bnd.tolist()} (of it the derived bound {OR.bound(om_max, Q['step'], x).tolist()})")
        assert (err <= bnd).all()
    # against the float64 model on the NUFFT plan with the device's own maps, at rounding level, and adjointness on the device outputs: the
    # model pair shares its weights and is exactly adjoint, so <A p, q> - <p, A^H q> on the device is <df, q> - <p, da>
    E = _np(maps)
    mod_f, mod_a = OR.model_forward(P, Q, E, x), OR.model_adjoint(P, Q, E, y, wgt)
    bf, ba = forward_err_norm(P, Q, E, x, mod_f), adjoint_err(P, Q, E, y, wgt)
    ef = np.linalg.norm(got_f - mod_f, axis=1)
    ra = float((np.abs(got_a - mod_a) / ba).max())
    print(f"        against the float64 model: forward ||err|| {ef.tolist()} bound {bf.tolist()}; adjoint worst err / bound {ra:.3f}")
    assert (ef <= bf).all() and ra <= 1.0
    nx, ny = np.linalg.norm(x.reshape(n, -1), axis=1), np.linalg.norm(y, axis=1)
    yw = y * wgt.astype(np.float64)                                                 # <A p, W q> = <p, A^H W q>
    lhs = np.array([np.vdot(yw[j], got_f[j]) - np.vdot(got_a[j], x[j]) for j in range(n)])
    lim = bf * np.linalg.norm(yw, axis=1) + np.linalg.norm(ba.reshape(n, -1), axis=1) * nx
    print(f"        adjointness |<A p, W q> - <p, A^H W q>| {np.abs(lhs).tolist()} bound {lim.tolist()} (relative to ||p|| ||q||: "
          f"{(np.abs(lhs) / (nx * ny)).tolist()})")
    assert (np.abs(lhs) <= lim).all()


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------------

def _normal_norm(P, Q, E, wgt, iters=40):
    """||A^H W A|| of the model on the plan (slice 0's maps) by power iteration, float64"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, P["h"], P["w"])) + 1j * rng.standard_normal((1, P["h"], P["w"]))
    s = 0.0
    for _ in range(iters):
        x /= np.linalg.norm(x)
        x = OR.model_adjoint(P, Q, E[:1], OR.model_forward(P, Q, E[:1], x), wgt)
        s = float(np.linalg.norm(x))
    return s


def _stage_inputs(n, h, w, P, Q, E, weights):
    """The CG tolerances are float32 figures taken over from stages whose normal operator is well conditioned at mu = 0.3 (the Cartesian SENSE
    projector: norm 1), and a CG's rounding error grows with the condition number kappa = (||A^H W A|| + mu) / mu.  Two sets of weights:
    "pipe", Pipe and Menon's density weights (tests/dcf_ref.py), the weights the stage is meant to run with - the tolerances are asserted as
    they stand; "generic", weights drawn from [0.5, 1.5], under which every interleaf's centre sample counts in full and ||A^H W A|| is about
    twice as large - the tolerances are scaled by kappa(generic) / kappa(pipe), both norms by float64 power iteration on the model, never
    below 1.  Returns the inputs and that factor."""
    rng = np.random.default_rng(177)
    xr = rng.random((n, h, w)).astype(np.float32).astype(np.float64)
    z0 = _rt(xr + 0.05 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    u0 = _rt(0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))))
    pipe = D.pipe(P, 30)[0].astype(np.float32)
    generic = (0.5 + rng.random(P["m"])).astype(np.float32)
    wgt, scale = pipe, 1.0
    if weights == "generic":
        s_pipe, s_gen = _normal_norm(P, Q, E, pipe), _normal_norm(P, Q, E, generic)
        wgt, scale = generic, max(1.0, (s_gen + 0.3) / (s_pipe + 0.3))
        print(f"||A^H W A||: {s_pipe:.3f} with density weights, {s_gen:.3f} with weights in [0.5, 1.5]: the CG tolerances are scaled by {scale:.3f}")
    ys = _rt(OR.model_forward(P, Q, E, xr.astype(np.complex128)) + 0.02 * (rng.standard_normal((n, P["m"])) + 1j * rng.standard_normal((n, P["m"]))))
    return xr, z0, u0, wgt, ys, scale


@pytest.mark.parametrize("K,weights", ((4, "pipe"), (8, "pipe"), (4, "generic")))
def test_the_stage_step_composition_cg_dc_stopped_slices_and_snapshots(K, weights):
    """pnp_offres_normal, pnp_offres_cg_residual, pnp_prox_dual, pnp_step, pnp_residuals, pnp_snapshot / pnp_restore in off-resonance mode"""
    h, w, kind, J, L, n = 32, 32, "spiral", 6, 3, 3
    traj, t, P, om = setup(h, w, kind, J)
    Q = OR.plan(t, L)
    e = planned(n, h, w, kind, J, L)
    with pytest.raises(_lib.PnPError, match="not in off-resonance mode"):
        e.offres_cg_residual()
    od = f32(om)
    E = _np(e.offres_maps(od))                                                      # the device's maps: the model runs on what the device uses
    xr, z0, u0, wgt, ys, scale = _stage_inputs(n, h, w, P, Q, E, weights)
    mu = np.full(n, 0.3, dtype=np.float32)
    mu64 = mu.astype(np.float64)
    wd = f32(wgt)
    e.set_kspace_offres(c64(ys), od, wd, cg_iters=K)
    assert e.offres_live and e.coils == 0 and e.ncsense_coils == 0
    for call in (e.nc_cg_residual, e.cg_residual, e.ncsense_cg_residual):           # the other modes' getters refuse
        with pytest.raises(_lib.PnPError):
            call()
    for call in (e.nc_normal, e.normal_op, e.ncsense_normal):
        with pytest.raises(_lib.PnPError):
            call(c64(u0, (n, 1, h, w)), f32(mu))
    assert not e.offres_cg_residual().any()                                         # 0 before the first solve
    # the normal operator: the composition of the two operators and one fma; then against float64
    pd = c64(u0, (n, 1, h, w))
    q = _np(e.offres_normal(pd, f32(mu)))[:, 0]
    comp = _np(e.offres_adjoint(e.offres_forward(pd, e.offres_maps(od)), e.offres_maps(od), wd))
    exact = comp + mu64[:, None, None] * u0
    off = float(max((np.abs(q.real - exact.real) / np.maximum(np.abs(exact.real), 1e-30)).max(),
                    (np.abs(q.imag - exact.imag) / np.maximum(np.abs(exact.imag), 1e-30)).max()))
    print(f"offres_normal against fma(mu, p, adjoint(forward(p))): worst relative distance {off:.3e} (one rounding: {U:.3e})")
    assert off <= U * (1 + 1e-6)
    # one prox_dual against the float64 CG on the model operator
    aty = OR.model_adjoint(P, Q, E, ys, wgt)
    xs, zs, us = f32(xr, (n, 1, h, w)), c64(z0, (n, 1, h, w)), c64(u0, (n, 1, h, w))
    e.prox_dual(xs, zs, us, f32(mu))
    zr, ur, rr = OR.prox_dual(P, Q, E, xr, z0, u0, aty, mu64, K, wgt)
    res = e.offres_cg_residual().cpu().numpy().astype(np.float64)
    bmax, brms, bres = (scale * MARGIN * v for v in F32_MU03_K4)
    d = np.abs(_np(zs)[:, 0] - zr)
    emax, erms = float(d.max() / np.abs(zr).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr) ** 2).sum()))
    umax = float(np.abs(_np(us)[:, 0] - ur).max() / np.abs(zr).max())
    dres = float((np.abs(res - rr) / rr).max())
    print(f"prox_dual K={K}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res} ref {rr} d_res {dres:.3e} / {bres:.2e}")
    assert emax <= bmax and erms <= brms and umax <= bmax and dres <= bres
    # the DC column against the model's misfit
    dc = e.residuals(xs, zs, us, dc=True).cpu().numpy().astype(np.float64)[:, 5]
    dcr = OR.dc_misfit(P, Q, E, xr, ys, wgt)
    s = NR.op_norm(P)                                                               # |E_l| = 1 and b0 + b1 = 1: the segmented operator's norm is at most the NUFFT's
    bdc = 1e-6 * s * math.sqrt(float(wgt.max())) * np.linalg.norm(xr.reshape(n, -1), axis=1) + 5e-7 * dcr
    print(f"dc column {dc} ref {dcr} |d| {np.abs(dc - dcr)} bound {bdc}")
    assert (np.abs(dc - dcr) <= bdc).all()
    # three steps under the TV prior: each is tv_denoise then prox_dual, bit for bit; the float64 stage on the device's own x; slice 1 stopped in step 2
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    sig = f32(np.full(n, 0.05, dtype=np.float32))
    e2 = planned(n, h, w, kind, J, L)
    e2.set_kspace_offres(c64(ys), od, wd, cg_iters=K)
    t_state = torch.zeros(n, dtype=torch.float32, device=DEV)
    for step in range(3):
        zin, uin = _np(zs)[:, 0], _np(us)[:, 0]
        keep = [v.clone() for v in (xs, zs, us, t_state, e.offres_cg_residual())]
        tact = f32(np.array([0.0, 1.0 if step == 1 else 0.0, 0.0], dtype=np.float32))
        # the composition on a second handle from the same state
        x2, z2, u2 = xs.clone(), zs.clone(), us.clone()
        v = z2.real - u2.real                                                       # one float32 subtraction per pixel
        xp = e2.tv_denoise(v, torch.tensor(1.0, dtype=torch.float32, device=DEV) * sig, 5)
        if step == 1:
            xp[1] = x2[1]
        e2.prox_dual(xp, z2, u2, f32(mu), tact)
        e.step(xs, zs, us, f32(mu), sig, t_action=tact, t_state=t_state)
        for name, a, b in zip("xzu", (xs, zs, us), (xp, z2, u2)):
            assert _same(a, b), (f"step {step + 1}: {name} of pnp_step differs from tv_denoise + pnp_prox_dual")
        xd = _np(xs)[:, 0]
        zr, ur, rr = OR.prox_dual(P, Q, E, xd, zin, uin, aty, mu64, K, wgt)
        live = [0, 2] if step == 1 else [0, 1, 2]
        d = np.abs(_np(zs)[live, 0] - zr[live])
        emax, erms = float(d.max() / np.abs(zr[live]).max()), float(math.sqrt((d ** 2).sum() / (np.abs(zr[live]) ** 2).sum()))
        umax = float(np.abs(_np(us)[live, 0] - ur[live]).max() / np.abs(zr[live]).max())
        print(f"step {step + 1}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {e.offres_cg_residual().cpu().numpy()}")
        assert emax <= bmax and erms <= brms and umax <= bmax
        if step == 1:                                                               # the stopped slice keeps x, z, u, t and its CG residual
            for name, a, kp in zip(("x", "z", "u", "t", "cg"), (xs, zs, us, t_state, e.offres_cg_residual()), keep):
                assert _same(a[1], kp[1]), name
    # snapshot / restore round-trips, and the restored episode continues with the same bits
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
    # the frozen case: y = 0, x0 = 0 never produces NaN
    x, z, u = e.reset_offres(c64(np.zeros((n, 1, h, w), dtype=np.complex64)), c64(np.zeros((n, P["m"]), dtype=np.complex64)), od, None, cg_iters=K)
    e.prox_dual(x, z, u, f32(mu))
    assert not _bits(z).any() and not _bits(u).any() and not e.offres_cg_residual().any()
    e.step(x, z, u, f32(mu), sig)
    assert torch.isfinite(torch.view_as_real(z)).all() and torch.isfinite(x).all() and torch.isfinite(torch.view_as_real(u)).all()


# ---- the correction corrects ----------------------------------------------------------------------------------------------------------------------

CORRECTS = OR.CORRECTS
corrects_problem = OR.corrects_problem                        # the fixture tests/test_offres_host.py runs in float64 on the CPU


def _psnr(x, gt):
    return float(10.0 * math.log10(1.0 / np.mean((np.clip(x, 0, 1) - gt) ** 2)))


def test_the_correction_corrects():
    c = CORRECTS
    h, w = c["h"], c["w"]
    traj, t, omega, gt, y, L = corrects_problem()
    m = traj.shape[0]
    e = _engine(1, h, w)
    e.nufft_plan(traj, grid=GRIDS[(h, w)], width=c["J"])
    e.offres_plan(t, L)
    dcf = e.nufft_dcf(iters=30)
    od, yd = f32(omega.astype(np.float32)), c64(y.reshape(1, m))
    mu = f32(np.full(1, c["mu"], dtype=np.float32))
    sig = OR.corrects_schedule()
    e.set_prior("tv", tv_scale=1.0, tv_iters=c["tv_iters"])
    gd = f32(gt.astype(np.float32), (1, 1, h, w))
    zg = c64(gt.astype(np.complex64), (1, 1, h, w))
    out = {}
    for name in ("offres", "plain"):
        if name == "offres":
            x0 = e.offres_adjoint(yd, e.offres_maps(od), dcf).reshape(1, 1, h, w)
            x, z, u = e.reset_offres(x0, yd, od, dcf, cg_iters=c["K"])
        else:
            x0 = e.nufft_adjoint(yd, dcf).reshape(1, 1, h, w)
            x, z, u = e.reset_nc(x0, yd, dcf, cg_iters=c["K"])
        dc_gt = float(e.residuals(gd, zg, torch.zeros_like(zg), dc=True)[0, 5])
        for k in range(c["steps"]):
            e.step(x, z, u, mu, f32(sig[k:k + 1]))
        out[name] = (_psnr(_np(x)[0, 0], gt), dc_gt)
    om_max, span = float(np.abs(omega).max()), float(t.max() - t.min())
    D = span / (L - 1)
    wsum = float(dcf.double().sum())
    lim = math.sqrt(wsum) * (float(OR.bound(om_max, D, gt[None])[0]) + model_tol(h, w, c["J"]) * float(np.abs(y).max()))
    print(f"omega_max span = {om_max * span / math.pi:.3f} pi, L = {L}: PSNR off-resonance stage {out['offres'][0]:.3f} dB, plain stage {out['plain'][0]:.3f} dB; "
          f"DC at x = gt: {out['offres'][1]:.4e} (off-resonance), {out['plain'][1]:.4e} (plain), bound {lim:.4e}")
    assert out["offres"][0] > out["plain"][0]
    assert out["offres"][1] < lim < out["plain"][1]
    assert abs(out["offres"][0] - OR.CORRECTS_PSNR[0]) <= 0.01 and abs(out["plain"][0] - OR.CORRECTS_PSNR[1]) <= 0.01      # the float64 restatement's


def test_the_correction_through_the_environment_and_the_fixed_schedule_solver():
    """PnPEnv.reset with data["omega"] / data["times"]: the same fixture through the public drivers ends at the restatement's PSNR, a second
    env.reset re-uses both plans, and an episode of another stage in between is re-bound"""
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    c = CORRECTS
    h, w = c["h"], c["w"]
    traj, t, omega, gt, y, L = corrects_problem()
    m = traj.shape[0]
    env = PnPEnv(max_episode_step=c["steps"], denoiser=TVDenoiser2D(scale=1.0, iters=c["tv_iters"]), device_type="cuda", cg_iters=c["K"],
                 nufft_width=c["J"], nufft_grid=c["grid"])
    eng = env._engine_for(1, h, w, torch.device("cuda", 0))
    dcf = acquisition.pipe_dcf(env, traj, iters=30, width=c["J"], grid=c["grid"])
    eng.offres_plan(t, L)
    x0 = eng.offres_adjoint(c64(y.reshape(1, m)), eng.offres_maps(f32(omega.astype(np.float32))), dcf).reshape(1, 1, h, w)
    mat = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(c64(y.reshape(1, 1, m))), "ATy0": torch.view_as_real(x0),
           "gt": f32(gt.astype(np.float32), (1, 1, h, w)), "traj": torch.from_numpy(traj), "dcf": dcf,
           "omega": f32(omega.astype(np.float32)), "times": torch.from_numpy(t), "segments": L}
    mu, sig = np.full((1, c["steps"]), c["mu"], dtype=np.float32), OR.corrects_schedule()[None]
    r = FixedScheduleSolver(env, max_iter=c["steps"], dc=True).run(mat, mu, sig)
    assert env._engine.offres_live and env._engine.offres_segments == L
    p = _psnr(_np(r.x)[0, 0], gt)
    print(f"through PnPEnv and FixedScheduleSolver: {p:.3f} dB (float64 restatement {OR.CORRECTS_PSNR[0]}), dc {r.dc.tolist()}")
    assert abs(p - OR.CORRECTS_PSNR[0]) <= 0.01
    auto = dict(mat)
    del auto["segments"]                                                            # the chooser, capped at the library's 32: the same L here
    st = env.reset(auto, "cuda")
    assert st["segments"] == L and env._engine.offres_planned(t, L)
    with pytest.raises(ValueError, match="times"):
        env.reset({k: v for k, v in mat.items() if k != "times"}, "cuda")
    with pytest.raises(ValueError, match="single-coil"):
        env.reset(dict(mat, sens=torch.ones((2, h, w), dtype=torch.complex64)), "cuda")


def test_cli_b0_fixed_on_a_ground_truth_folder(tmp_path):
    import contextlib
    import io
    import json
    from dt4image_restoration_amd import cli
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5), synthetic.phantom(64, 64, 6)]).astype(np.float32))
    base = ["--block_size", "6", "--n_embeds", "9", "--gt", str(gtd), "--tasks", "4x_5", "--prior", "tv", "--seed", "3", "--traj", "spiral",
            "--interleaves", "8"]

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = cli.main(base + extra + ["fixed", "--max_iter", "10", "--dc"])
        assert len(out) == 1 and out[0]["n"] == 2
        return out[0]

    plain = run([])
    zero = run(["--b0", "0", "--readout-ms", "10"])                                 # no field: one segment, E = 1 - the plain stage's numbers
    b0 = run(["--b0", "40", "--readout-ms", "10", "--b0-segments", "16"])
    auto = run(["--b0", "10", "--readout-ms", "5"])
    print(f"cli --traj spiral fixed: plain {plain['psnr']:.3f} dB; --b0 0: {zero['psnr']:.3f} dB; --b0 40 --b0-segments 16: {b0['psnr']:.3f} dB "
          f"(+{b0['psnr_increment']:.3f}); --b0 10 --readout-ms 5, auto: {auto['psnr']:.3f} dB (+{auto['psnr_increment']:.3f})")
    assert abs(zero["psnr"] - plain["psnr"]) <= 0.01
    for x in (b0, auto):
        assert "spiral-nc" in x["set"] and np.isfinite(x["psnr"]) and x["psnr_increment"] > 0.0


def test_simulate_under_a_field_map_is_the_acquisition_and_matches_the_exact_problem():
    h, w, n, J, L = 32, 32, 2, 6, 8
    traj, t, P, om = setup(h, w, "spiral", J)
    omega = om[:n] * 0.25                                                           # 25 Hz: omega_max D / 2 = 0.11 rad at L = 8
    gt = np.stack([synthetic.phantom(h, w, 1234 + j) for j in range(n)]).astype(np.float32)
    dcf = D.pipe(P, 30)[0].astype(np.float32)
    e = _engine(n, h, w)
    d = acquisition.simulate(e, gt, None, 0.02, 1234, traj=traj, dcf=dcf, nufft_width=J, nufft_grid=GRIDS[(h, w)], omega=omega, times=t, segments=L)
    assert e.offres_segments == L and d["segments"] == L and not e.offres_live
    assert torch.equal(d["omega"], f32(omega)) and np.array_equal(d["times"].numpy(), t) and tuple(d["y0"].shape) == (n, 1, P["m"], 2)
    y, aty0, x0 = e.acquire_offres(f32(gt, (n, 1, h, w)), f32(omega), 0.02, 1234, dcf=f32(dcf))
    assert _same(torch.view_as_complex(d["y0"])[:, 0], y) and _same(torch.view_as_complex(d["ATy0"]), aty0) and _same(torch.view_as_complex(d["x0"]), x0)
    ref = synthetic.make_problem_ncb0(n, h, w, traj, t, omega, dcf=dcf, sigma_n=0.02, seed=1234)      # the exact operator, the same noise
    yr = ref["y0"][:, 0, :, 0].astype(np.float64) + 1j * ref["y0"][:, 0, :, 1].astype(np.float64)
    err = np.abs(_np(y) - yr).max(axis=1)
    Q = OR.plan(t, L)
    bnd = model_tol(h, w, J) * np.linalg.norm(yr, axis=1) + OR.bound(float(np.abs(omega).max()), Q["step"], gt)
    print(f"simulate(omega=, times=) against make_problem_ncb0: max |dy| {err.tolist()} bound {bnd.tolist()}")
    assert (err <= bnd).all()
    with pytest.raises(ValueError, match="go together"):
        acquisition.simulate(e, gt, None, 0.0, 1, traj=traj, omega=omega)
    with pytest.raises(ValueError, match="need traj"):
        acquisition.simulate(e, gt, np.ones((h, w)), 0.0, 1, omega=omega, times=t)


# ---- invariance -----------------------------------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_the_batch_the_place_the_stream_or_how_the_map_is_given():
    h, w, kind, J, L, n = 32, 32, "radial", 4, 8, 3
    om = setup(h, w, kind, J)[3]
    e = planned(n, h, w, kind, J, L)
    full = _run_all(e, h, w, kind, J, L, slice(0, n), om, MU3)
    again = _run_all(e, h, w, kind, J, L, slice(0, n), om, MU3)
    for name, a, b in zip(NAMES, full, again):
        assert _same(a, b), name
    e1 = planned(1, h, w, kind, J, L)
    for j in range(n):                                                              # a slice alone, in a handle of one slice
        alone = _run_all(e1, h, w, kind, J, L, slice(j, j + 1), om[j:j + 1], MU3)
        for name, a, b in zip(NAMES, full, alone):
            assert _same(a[j:j + 1], b), (name, j)
    shared = _run_all(e, h, w, kind, J, L, slice(0, n), om[1], MU3)
    stacked = _run_all(e, h, w, kind, J, L, slice(0, n), np.ascontiguousarray(np.broadcast_to(om[1], (n, h, w))), MU3)
    for name, a, b in zip(NAMES, shared, stacked):
        assert _same(a, b), name
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _run_all(e, h, w, kind, J, L, slice(0, n), om, MU3)
    side.synchronize()
    for name, a, b in zip(NAMES, full, other):
        assert _same(a, b), name


# ---- the handle -----------------------------------------------------------------------------------------------------------------------------------

class _Episode:
    """an episode of one stage kind on a handle with both plans: install (reset), re-install (set_kspace), two steps"""

    def __init__(self, e, kind, n, h, w, seed):
        self.e, self.kind, self.n = e, kind, n
        traj, t, P, om = setup(h, w, "spiral", 6)
        m = P["m"]
        rng = np.random.default_rng(seed)
        cplx = lambda *s: c64(_rt(rng.standard_normal(s) + 1j * rng.standard_normal(s)))      # noqa: E731
        self.x0 = c64(_rt(rng.random((n, 1, h, w))))
        self.mask = torch.from_numpy(synthetic.radial_mask(h, w, 4.0)).to(DEV)
        self.sens = c64(synthetic.coil_maps(3, h, w))
        self.om = f32(om[:n] * (1.0 + 0.1 * seed))
        self.w = f32((0.5 + rng.random(m)).astype(np.float32))
        self.y = {"cart": lambda: cplx(n, 1, h, w), "mc": lambda: cplx(n, 3, h, w), "nc": lambda: cplx(n, m), "nc_tz": lambda: cplx(n, m),
                  "ns": lambda: cplx(n, 3, m), "offres": lambda: cplx(n, m)}[kind]()

    def reset(self):
        e, k = self.e, self.kind
        if k == "cart":
            return e.reset(self.x0, self.y, self.mask)
        if k == "mc":
            return e.reset(self.x0, self.y, self.mask, sens=self.sens, cg_iters=3)
        if k == "nc":
            return e.reset_nc(self.x0, self.y, self.w, cg_iters=3)
        if k == "nc_tz":
            return e.reset_nc_tz(self.x0, self.y, self.w, cg_iters=3)
        if k == "ns":
            return e.reset_ncsense(self.x0, self.y, self.sens, self.w, cg_iters=3)
        return e.reset_offres(self.x0, self.y, self.om, self.w, cg_iters=3)

    def set_kspace(self):
        e, k = self.e, self.kind
        if k == "cart":
            return e.set_kspace(self.y, self.mask)
        if k == "mc":
            return e.set_kspace(self.y, self.mask, sens=self.sens, cg_iters=3)
        if k == "nc":
            return e.set_kspace_nc(self.y, self.w, cg_iters=3)
        if k == "nc_tz":
            return e.set_kspace_nc_tz(self.y, self.w, cg_iters=3)
        if k == "ns":
            return e.set_kspace_ncsense(self.y, self.sens, self.w, cg_iters=3)
        return e.set_kspace_offres(self.y, self.om, self.w, cg_iters=3)

    def step(self, it, k):
        x, z, u = it
        mu = torch.tensor([0.2 + 0.1 * k + 0.05 * i for i in range(self.n)], dtype=torch.float32, device=DEV)
        sg = torch.tensor([(30.0 - 5.0 * k - i) / 255.0 for i in range(self.n)], dtype=torch.float32, device=DEV)
        self.e.step(x, z, u, mu, sg)

    def state(self, it):
        return [v.clone() for v in it] + [self.e.residuals(*it, dc=True)]


OTHERS = ("cart", "mc", "nc", "ns", "nc_tz")
H_N, H_H, H_W, H_L = 2, 32, 32, 3


def _handle():
    e = planned(H_N, H_H, H_W, "spiral", 6, H_L)
    e.set_prior("tv", tv_scale=1.0, tv_iters=5)
    return e


def test_the_new_stage_against_the_other_stages_in_both_orders_and_both_plan_calls():
    """pnp_set_kspace_offres, pnp_reset_offres, pnp_offres_plan: the stage installed last runs; a plan call drops the stage built on it"""
    traj, t, P, om = setup(H_H, H_W, "spiral", 6)
    for other in OTHERS:
        for first, second in (("offres", other), (other, "offres")):
            e = _handle()
            a, b = _Episode(e, first, H_N, H_H, H_W, 1), _Episode(e, second, H_N, H_H, H_W, 2)
            it = a.reset()
            a.step(it, 0); a.step(it, 1)
            want = a.state(it)
            e = _handle()                                                           # the same episode with the other stage's installers in between
            a, b = _Episode(e, first, H_N, H_H, H_W, 1), _Episode(e, second, H_N, H_H, H_W, 2)
            it = a.reset()
            a.step(it, 0)
            itb = b.reset()
            assert e.offres_live == (second == "offres")
            b.step(itb, 0)                                                          # the stage installed last runs
            eb = _handle()
            b2 = _Episode(eb, second, H_N, H_H, H_W, 2)
            itb2 = b2.reset()
            b2.step(itb2, 0)
            for name, p, q in zip("xzud", b.state(itb), b2.state(itb2)):
                assert _same(p, q), (first, second, name)
            a.set_kspace()
            assert e.offres_live == (first == "offres")
            a.step(it, 1)
            for name, p, q in zip("xzud", a.state(it), want):
                assert _same(p, q), (first, second, name)
    # both plan calls from the live stage
    e = _handle()
    a = _Episode(e, "offres", H_N, H_H, H_W, 1)
    it = a.reset()
    a.step(it, 0)
    want = [v.clone() for v in it]
    e.offres_plan(t, H_L + 1)                                                       # a new off-resonance plan drops the stage built on the old one
    assert not e.offres_live and e.offres_segments == H_L + 1
    with pytest.raises(_lib.PnPError):
        a.step(it, 1)
    with pytest.raises(_lib.PnPError, match="not in off-resonance mode"):
        e.offres_cg_residual()
    e.offres_plan(t, H_L)
    a.set_kspace()
    assert e.offres_live
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)                            # a new NUFFT plan drops the off-resonance plan and the stage
    assert not e.offres_live and e.offres_segments == 0
    with pytest.raises(_lib.PnPError, match="no off-resonance plan"):
        a.set_kspace()
    for v, k in zip(it, want):
        assert _same(v, k)                                                          # a refused call leaves the iterate as it was
    e.offres_plan(t, H_L)
    a.set_kspace()
    a.step(it, 1)
    e2 = _handle()
    a2 = _Episode(e2, "offres", H_N, H_H, H_W, 1)
    it2 = a2.reset()
    a2.step(it2, 0); a2.step(it2, 1)
    for name, p, q in zip("xzud", a.state(it), a2.state(it2)):
        assert _same(p, q), name


def test_the_intruders_between_two_steps_of_an_episode_of_every_kind_change_nothing():
    """pnp_offres_maps, pnp_offres_forward, pnp_offres_adjoint, pnp_acquire_offres between two steps of a live episode of every stage kind"""
    traj, t, P, om = setup(H_H, H_W, "spiral", 6)
    x, y, wgt = _data(H_N, H_H, H_W, P["m"], seed=8)
    gt = f32(np.stack([synthetic.phantom(H_H, H_W, 70 + j) for j in range(H_N)]).astype(np.float32), (H_N, 1, H_H, H_W))
    for kind in OTHERS + ("offres",):
        ref = _Episode(_handle(), kind, H_N, H_H, H_W, 1)
        itr = ref.reset()
        ref.step(itr, 0); ref.step(itr, 1)
        e = _handle()
        ep = _Episode(e, kind, H_N, H_H, H_W, 1)
        it = ep.reset()
        ep.step(it, 0)
        live, ws = e.offres_live, e.workspace_bytes
        for omega in (f32(om[2]), f32(om[:H_N] * 3.0)):
            maps = e.offres_maps(omega)
            e.offres_forward(c64(x), maps)
            e.offres_adjoint(c64(y), maps, f32(wgt))
            e.acquire_offres(gt, omega, 0.05, 7, dcf=f32(wgt))
        assert e.offres_live == live and e.workspace_bytes >= ws
        ep.step(it, 1)
        for name, p, q in zip("xzud", ep.state(it), ref.state(itr)):
            assert _same(p, q), (kind, name)


def test_handle_dependent_argument_errors_leave_the_outputs_untouched():
    h, w, n = 32, 32, 2
    traj, t, P, om = setup(h, w, "spiral", 6)
    e = _engine(n, h, w)
    lib = e.lib
    maps = torch.zeros((1, 3, h, w), dtype=torch.complex64, device=DEV)
    out = torch.full((n, P["m"]), 7.0, dtype=torch.complex64, device=DEV)
    img = torch.full((n, h, w), 7.0, dtype=torch.complex64, device=DEV)
    od = f32(om[0])

    def refused(rc, what, code):
        assert rc == code and what in lib.pnp_last_error(), (rc, lib.pnp_last_error())

    refused(lib.pnp_offres_plan(e._h, t.ctypes.data, 3, 0), b"no NUFFT plan", -3)
    refused(lib.pnp_offres_maps(e._h, od.data_ptr(), 1, maps.data_ptr(), None), b"no NUFFT plan", -3)
    assert e.offres_segments == 0
    e.nufft_plan(traj, grid=(P["gh"], P["gw"]), width=6)
    refused(lib.pnp_offres_maps(e._h, od.data_ptr(), 1, maps.data_ptr(), None), b"no off-resonance plan", -3)
    refused(lib.pnp_offres_forward(e._h, img.data_ptr(), maps.data_ptr(), 1, n, out.data_ptr(), None), b"no off-resonance plan", -3)
    refused(lib.pnp_offres_adjoint(e._h, out.data_ptr(), None, maps.data_ptr(), 1, n, img.data_ptr(), None), b"no off-resonance plan", -3)
    refused(lib.pnp_set_kspace_offres(e._h, out.data_ptr(), od.data_ptr(), 1, None, 4, None), b"no off-resonance plan", -3)
    refused(lib.pnp_acquire_offres(e._h, img.data_ptr(), od.data_ptr(), 1, None, 0.0, 0, 0, out.data_ptr(), None, None, None), b"no off-resonance plan", -3)
    bad = t.copy()
    bad[5] = float("nan")
    refused(lib.pnp_offres_plan(e._h, bad.ctypes.data, 3, 0), b"not finite", -1)
    same = np.full_like(t, 2e-3)
    refused(lib.pnp_offres_plan(e._h, same.ctypes.data, 2, 0), b"positive span", -1)
    assert e.offres_segments == 0
    e.offres_plan(same, 1)                                                          # L = 1 takes a zero span
    assert e.offres_segments == 1
    e.offres_plan(t, 3)
    refused(lib.pnp_offres_plan(e._h, bad.ctypes.data, 4, 0), b"not finite", -1)
    assert e.offres_segments == 3                                                   # a refused plan call leaves the plan as it was
    refused(lib.pnp_offres_maps(e._h, od.data_ptr(), 3, maps.data_ptr(), None), b"map_n must be 1 or n=2", -1)
    refused(lib.pnp_offres_forward(e._h, img.data_ptr(), maps.data_ptr(), 3, n, out.data_ptr(), None), b"map_n must be 1 or n=2", -1)
    refused(lib.pnp_offres_forward(e._h, img.data_ptr(), maps.data_ptr(), 1, n + 1, out.data_ptr(), None), b"batch must be 1..n=2", -1)
    refused(lib.pnp_offres_adjoint(e._h, out.data_ptr(), None, maps.data_ptr(), 5, n, img.data_ptr(), None), b"map_n must be 1 or n=2", -1)
    refused(lib.pnp_set_kspace_offres(e._h, out.data_ptr(), od.data_ptr(), 3, None, 4, None), b"map_n must be 1 or n=2", -1)
    refused(lib.pnp_acquire_offres(e._h, img.data_ptr(), od.data_ptr(), 3, None, 0.0, 0, 0, out.data_ptr(), None, None, None), b"map_n must be 1 or n=2", -1)
    refused(lib.pnp_offres_cg_residual(e._h, out.data_ptr(), None), b"not in off-resonance mode", -3)
    refused(lib.pnp_offres_normal(e._h, img.data_ptr(), od.data_ptr(), out.data_ptr(), None), b"not in off-resonance mode", -3)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((img == 7.0).all()) and not _bits(maps).any() and not e.offres_live


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,kind,J,L,n,naive", ((80, 64, "spiral", 4, 3, 2, 0), (16, 16, "radial", 6, 32, 3, 0), (32, 32, "spiral", 6, 8, 2, 1)))
def test_every_caller_owned_buffer_keeps_its_guard_bands(h, w, kind, J, L, n, naive, monkeypatch):
    traj, t, P, om = setup(h, w, kind, J)
    m = P["m"]
    e = planned(n, h, w, kind, J, L, monkeypatch=monkeypatch, naive=naive)
    lib, s = e.lib, e._stream()
    x, y, wgt = _data(n, h, w, m, seed=1)
    for map_n, omega in ((1, om[0]), (n, om[:n])):
        od = g_f32(omega)
        maps = GB.guarded((map_n, L, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"maps": maps}, inputs={"omega": od}):
            _lib.check(lib.pnp_offres_maps(e._h, od.data_ptr(), map_n, maps.data_ptr(), s), "pnp_offres_maps")
        for batch in (1, n):
            img, smp, wd = g_c64(x[:batch]), g_c64(y[:batch]), g_f32(wgt)
            out_s, out_i = GB.guarded((batch, m), torch.complex64, DEV), GB.guarded((batch, h, w), torch.complex64, DEV)
            with GB.watch(outputs={"samples": out_s}, inputs={"img": img, "maps": maps}):
                _lib.check(lib.pnp_offres_forward(e._h, img.data_ptr(), maps.data_ptr(), map_n, batch, out_s.data_ptr(), s), "pnp_offres_forward")
            with GB.watch(outputs={"img": out_i}, inputs={"samples": smp, "weights": wd, "maps": maps}):
                _lib.check(lib.pnp_offres_adjoint(e._h, smp.data_ptr(), wd.data_ptr(), maps.data_ptr(), map_n, batch, out_i.data_ptr(), s),
                           "pnp_offres_adjoint")
        gt = g_f32(np.stack([synthetic.phantom(h, w, 50 + j) for j in range(n)]).astype(np.float32), (n, 1, h, w))
        wd = g_f32(wgt)
        yo = GB.guarded((n, m), torch.complex64, DEV)
        ao, xo = GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"y": yo, "aty0": ao, "x0": xo}, inputs={"gt": gt, "omega": od, "dcf": wd}):
            _lib.check(lib.pnp_acquire_offres(e._h, gt.data_ptr(), od.data_ptr(), map_n, wd.data_ptr(), 0.02, 5, 0, yo.data_ptr(), ao.data_ptr(),
                                              xo.data_ptr(), s), "pnp_acquire_offres")
        xs, zs, us = GB.guarded((n, 1, h, w), torch.float32, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n, 1, h, w), torch.complex64, DEV)
        with GB.watch(outputs={"x": xs, "z": zs, "u": us}, inputs={"x0": xo, "y": yo, "omega": od, "w": wd}):
            _lib.check(lib.pnp_reset_offres(e._h, xo.data_ptr(), yo.data_ptr(), od.data_ptr(), map_n, wd.data_ptr(), 3, xs.data_ptr(), zs.data_ptr(),
                                            us.data_ptr(), s), "pnp_reset_offres")
        with GB.watch(outputs={}, inputs={"y": yo, "omega": od, "w": wd, "x": xs, "z": zs, "u": us}):
            _lib.check(lib.pnp_set_kspace_offres(e._h, yo.data_ptr(), od.data_ptr(), map_n, wd.data_ptr(), 3, s), "pnp_set_kspace_offres")
        mu = g_f32(MU3[:n])
        q, res = GB.guarded((n, 1, h, w), torch.complex64, DEV), GB.guarded((n,), torch.float32, DEV)
        with GB.watch(outputs={"q": q}, inputs={"p": zs, "mu": mu}):
            _lib.check(lib.pnp_offres_normal(e._h, zs.data_ptr(), mu.data_ptr(), q.data_ptr(), s), "pnp_offres_normal")
        with GB.watch(outputs={"z": zs, "u": us}, inputs={"x": xs, "mu": mu}):
            e.prox_dual(xs, zs, us, mu)
        with GB.watch(outputs={"out": res}, inputs={}):
            _lib.check(lib.pnp_offres_cg_residual(e._h, res.data_ptr(), s), "pnp_offres_cg_residual")
        assert torch.isfinite(res).all() and torch.isfinite(torch.view_as_real(q)).all()
    assert e.offres_segments == L and e.offres_live                                 # pnp_offres_segments, pnp_offres_live
    assert sorted(OC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_OFFRES)
