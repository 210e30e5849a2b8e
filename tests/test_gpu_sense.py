"""The multi-coil (SENSE) data-fidelity stage on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against the float64
restatement of tests/sense_ref.py.  Every figure is printed before it is asserted.

BOUNDS OF THE SOLVE CHECKS.  The GPU's K-th iterate is compared with the float64 K-th iterate (the same-K comparison: the K-th iterate is
a smooth function of the inputs).  The bound is TEN TIMES what a float32 restatement of the same K steps (sense_ref.cg_solve_f32: torch
CPU complex64, whose FFT is truly float32) measures against the float64 one on the CPU, the margin the suite gives its FFT checks, taken
per (mu, K) family as the maximum over the whole grid below (5 sizes x 4 coil counts x shared / per-slice maps and masks x 4 masks = 160
cases per family).  Measured on the CPU (err_max = max |dz| / max |z_ref|, err_rms = ||dz|| / ||z_ref||, d_res = relative difference of
cg_res; res64 = the float64 cg_res range):

      mu    K    err_max     err_rms     d_res       res64
      0.05  1    5.571e-07   2.322e-07   1.771e-07   1.2e-02 .. 3.3e-02
      0.05  4    4.099e-06   1.721e-06   4.348e-07   3.9e-03 .. 1.0e-02
      0.05  8    4.847e-06   1.998e-06   6.737e-07   2.9e-04 .. 1.9e-03
      0.3   1    5.497e-07   2.411e-07   9.134e-08   2.3e-02 .. 4.4e-02
      0.3   4    9.992e-07   3.740e-07   2.784e-07   2.5e-04 .. 1.5e-03
      0.3   8    1.040e-06   3.780e-07   4.868e-07   3.2e-06 .. 2.2e-05
      0.6   1    4.808e-07   2.122e-07   1.494e-07   2.5e-02 .. 4.5e-02
      0.6   4    5.946e-07   2.154e-07   3.632e-07   6.2e-05 .. 3.8e-04
      0.6   8    6.264e-07   2.211e-07   7.248e-07   1.6e-07 .. 1.2e-06

C = 1, S = 1, K = 2 against the single-coil pnp_prox_dual: both are float32 evaluations of the same float64 result (two CG iterations are
exact there, 5e-15); the single-coil stage is within the suite's FFT_ATOL = 3e-6 of it and the float32 restatement of the two CG
iterations measured max |dz| = 5.03e-06 / 9.44e-07 / 5.03e-07 at mu = 0.05 / 0.3 / 0.6 (128x128, 320x320, 640x320; 4x and 8x), so the
bound is 3e-6 + 10 x that.

Trajectory (sense_ref.TRAJ): |dPSNR| < 0.01 dB is asserted, the project's north-star bound; max |dx| is recorded against ten times the drift of the oracle's own
float32 mode (its denoiser in float32, cg_solve_f32) from its float64 mode over the six steps, measured on the CPU: 2.49e-06 -> 2.49e-05.

Acquisition: the bounds of tests/test_gpu_acquire.py (rms(err) / rms(ref) <= 1e-6; ATy0, x0: max abs <= 3e-6; y0: max abs <= 1e-6 max|ref|).
pnp_residuals' dc column: the bound of tests/test_gpu_residuals.py, |ddc| <= 1e-6 ||x|| + 5e-7 dc (the maps have unit RSS: ||S x|| = ||x||).
"""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sense_ref as R  # noqa: E402

from dt4image_restoration_amd import synthetic, weights  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0
F32 = {  # (mu, K): (err_max, err_rms, d_res) of the float32 restatement, from the table above
    (0.05, 1): (5.571e-07, 2.322e-07, 1.771e-07), (0.05, 4): (4.099e-06, 1.721e-06, 4.348e-07), (0.05, 8): (4.847e-06, 1.998e-06, 6.737e-07),
    (0.3, 1): (5.497e-07, 2.411e-07, 9.134e-08), (0.3, 4): (9.992e-07, 3.740e-07, 2.784e-07), (0.3, 8): (1.040e-06, 3.780e-07, 4.868e-07),
    (0.6, 1): (4.808e-07, 2.122e-07, 1.494e-07), (0.6, 4): (5.946e-07, 2.154e-07, 3.632e-07), (0.6, 8): (6.264e-07, 2.211e-07, 7.248e-07)}
RES_FAMILIES = [(0.05, 4), (0.05, 8), (0.3, 4), (0.3, 8)]
C1K2_F32 = {0.05: 5.03e-06, 0.3: 9.44e-07, 0.6: 5.03e-07}
FFT_ATOL, REL_RMS, Y0_REL_MAX = 3e-6, 1e-6, 1e-6
TRAJ_DX_F32 = 2.49e-06
DEV = "cuda"


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def c64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.complex64).to(DEV)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _install(e, cs, K):
    e.set_kspace(c64(cs["y"]), torch.from_numpy(cs["mask"]).to(DEV), sens=c64(cs["sens"]), cg_iters=K)


def _iterate(cs):
    n, h, w = cs["x"].shape
    return f32(cs["x"]).reshape(n, 1, h, w), c64(cs["z0"]).reshape(n, 1, h, w), c64(cs["u"]).reshape(n, 1, h, w)


def _rel_rms(got, ref):
    return float(np.sqrt((np.abs(got - ref) ** 2).sum() / (np.abs(ref) ** 2).sum()))


# ---- acquisition -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [0.0, 10.0 / 255.0])
@pytest.mark.parametrize("n,h,w,c,per_slice", [(2, 128, 128, 4, False), (1, 640, 320, 8, False), (2, 80, 160, 3, True), (2, 256, 256, 15, True)])
def test_acquire_mc_against_float64(n, h, w, c, per_slice, sigma):
    gt = np.stack([synthetic.phantom(h, w, 70 + i) for i in range(n)]).astype(np.float32)
    sens = synthetic.coil_maps(c, h, w)
    mask = synthetic.radial_mask(h, w, 4)
    if per_slice:
        sens = np.stack([synthetic.coil_maps(c, h, w, radius=1.3 + 0.1 * i) for i in range(n)])
        mask = np.stack([R.case_mask(h, w, "cartesian", 4, seed=i) for i in range(n)])
    sens = sens.astype(np.complex64)
    e = _engine(n, h, w)
    y, a, x0 = e.acquire(f32(gt).reshape(n, 1, h, w), torch.from_numpy(mask).to(DEV), sigma, 99, sens=c64(sens))
    yr, ar, xr = R.acquire(gt, sens, mask, sigma, 99)
    assert y.shape == (n, c, h, w) and a.shape == (n, 1, h, w) and x0.shape == (n, 1, h, w)
    yg, ag, xg = _np(y), _np(a)[:, 0], _np(x0)[:, 0]
    ymx, ymax, yrel = float(np.abs(yg - yr).max()), float(np.abs(yr).max()), _rel_rms(yg, yr)
    amx, arel, xmx = float(np.abs(ag - ar).max()), _rel_rms(ag, ar), float(np.abs(xg - xr).max())
    print(f"{n}x{h}x{w} C={c} per_slice={per_slice} sigma={sigma:.4f}: y0 max {ymx:.3e} (max|ref| {ymax:.1f}) rel {yrel:.3e}; "
          f"ATy0 max {amx:.3e} rel {arel:.3e}; x0 max {xmx:.3e}")
    assert yrel <= REL_RMS and ymx <= Y0_REL_MAX * ymax
    assert arel <= REL_RMS and amx <= FFT_ATOL and xmx <= FFT_ATOL
    m4 = np.broadcast_to(mask[None, None] if mask.ndim == 2 else mask[:, None], (n, c, h, w))
    assert not _bits(y).cpu().numpy().reshape(n, c, h, w, 2)[~m4].any()          # off-mask bins are +0.0 bit for bit
    assert torch.equal(torch.view_as_real(x0), torch.view_as_real(a).clamp_min(0))
    assert e.coils == 0                                                           # an acquisition does not change the handle's mode


@pytest.mark.parametrize("h,w", [(128, 128), (320, 320), (640, 320)])
@pytest.mark.parametrize("sigma", [0.0, 10.0 / 255.0])
def test_one_coil_with_unit_map_equals_pnp_acquire_bit_for_bit(h, w, sigma):
    n = 2
    e = _engine(n, h, w)
    gt = f32(np.stack([synthetic.phantom(h, w, 5 + i) for i in range(n)])).reshape(n, 1, h, w)
    mask = torch.from_numpy(synthetic.radial_mask(h, w, 4)).to(DEV)
    one = torch.ones((1, h, w), dtype=torch.complex64, device=DEV)
    single = e.acquire(gt, mask, sigma, 1234)
    multi = e.acquire(gt, mask, sigma, 1234, sens=one)
    for name, a, b in zip(("y0", "ATy0", "x0"), single, multi):
        assert _same(a, b.reshape(a.shape)), name
    other = e.acquire(gt, mask, 10.0 / 255.0, 1234, sens=torch.ones((2, h, w), dtype=torch.complex64, device=DEV))[0]
    assert not _same(other[:, 0], other[:, 1])                                   # coil 1 draws its own noise streams


# ---- the solve -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(128, 128), (320, 320)])
def test_one_coil_two_iterations_match_the_single_coil_stage(h, w):
    n = 2
    e = _engine(n, h, w)
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=5)
    y0 = c64(d["y0"][..., 0] + 1j * d["y0"][..., 1])
    mask = torch.from_numpy(d["mask"]).to(DEV)
    cs = R.solve_case(h, w, 1, False, "radial", 4)
    one = torch.ones((1, h, w), dtype=torch.complex64, device=DEV)
    for mu in R.SOLVE_MUS:
        mut = torch.full((n,), mu, dtype=torch.float32, device=DEV)
        x, z1, u1 = _iterate(cs)
        _, z2, u2 = _iterate(cs)
        e.set_kspace(y0, mask)
        assert e.coils == 0
        e.prox_dual(x, z1, u1, mut)
        e.set_kspace(y0, mask, sens=one, cg_iters=2)
        assert e.coils == 1
        e.prox_dual(x, z2, u2, mut)
        dz, du = float((z1 - z2).abs().max()), float((u1 - u2).abs().max())
        res = e.cg_residual().cpu().numpy()
        bound = FFT_ATOL + MARGIN * C1K2_F32[mu]
        print(f"{h}x{w} mu={mu}: max |z_mc - z_single| = {dz:.3e}, |du| = {du:.3e} (bound {bound:.2e}); cg_res {res}")
        assert dz <= bound and du <= bound
        assert (res < 1e-5).all()                                                 # exact after two iterations, to float32


def _check_solves(e, h, w, coils, per_slice, kind, accel, ref, failures):
    cs, kept = ref
    for mu in R.SOLVE_MUS:
        for K in R.SOLVE_KS:
            _install(e, cs, K)
            x, z, u = _iterate(cs)
            e.prox_dual(x, z, u, torch.full((2,), mu, dtype=torch.float32, device=DEV))
            res = e.cg_residual().cpu().numpy().astype(np.float64)
            zr, rr = kept[mu][K]
            emax, erms = R.solve_errors(_np(z)[:, 0], zr)
            ur = cs["u"] + cs["x"] - zr
            umax = float(np.abs(_np(u)[:, 0] - ur).max() / np.abs(zr).max())
            dres = float((np.abs(res - rr) / rr).max())
            bmax, brms, bres = (MARGIN * v for v in F32[(mu, K)])
            tag = f"{h}x{w} C={coils} per_slice={per_slice} {kind}{accel}x mu={mu} K={K}"
            print(f"{tag}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  "
                  f"cg_res {res[0]:.4e} {res[1]:.4e} ref {rr[0]:.4e} {rr[1]:.4e} d_res {dres:.3e}")
            if not (emax <= bmax and erms <= brms and umax <= 2 * bmax):
                failures.append((tag, emax, erms, umax))
            if (mu, K) in RES_FAMILIES and not dres <= bres:
                failures.append((tag, "cg_res", dres, bres))


def _reference(args):
    h, w, coils, per_slice, kind, accel = args
    cs = R.solve_case(h, w, coils, per_slice, kind, accel)
    kept = {}
    for mu in R.SOLVE_MUS:
        m = np.full(2, np.float64(np.float32(mu)))
        kept[mu] = R.cg_solve(cs["z0"], cs["x"], cs["u"], cs["aty"], cs["sens"], cs["mask"], m, max(R.SOLVE_KS), record=R.SOLVE_KS)[3]
    return cs, kept


@pytest.mark.parametrize("coils", R.SOLVE_COILS)
@pytest.mark.parametrize("h,w", R.SOLVE_SIZES)
def test_k_step_solve_and_cg_residual_against_float64(h, w, coils):
    """The whole grid: this (size, coils) x {shared, per-slice maps and masks} x {radial, cartesian} x {4x, 8x} x mu x K; cg_res is
    compared in every case of the families mu in {0.05, 0.3}, K in {4, 8}."""
    combos = [(h, w, coils, ps, kind, accel) for ps in (False, True) for kind, accel in R.SOLVE_MASKS]
    for kind, accel in R.SOLVE_MASKS:                       # (the mask cache is filled before the threads read it)
        for seed in (0, 1):
            R.case_mask(h, w, kind, accel, seed)
    with ThreadPoolExecutor(max_workers=8) as pool:
        refs = list(pool.map(_reference, combos))
    e = _engine(2, h, w)
    failures = []
    for args, ref in zip(combos, refs):
        _check_solves(e, *args, ref, failures)
    assert not failures, failures


# ---- exact properties ----------------------------------------------------------------------------------------------------------------

def _batch_case(h, w, coils, n):
    """n slices with their own maps and masks (slice i of `solve_case(n=...)`)."""
    return R.solve_case(h, w, coils, True, "cartesian", 4, n=n)


@pytest.mark.parametrize("h,w", [(128, 128), (320, 320)])
def test_stopped_slices_reproducibility_batch_position_and_streams(h, w):
    coils, n, K = 4, 3, 4
    cs = _batch_case(h, w, coils, n)
    e = _engine(n, h, w)
    _install(e, cs, K)
    mu = torch.tensor([0.05, 0.3, 0.6], device=DEV)
    x, z, u = _iterate(cs)
    e.prox_dual(x, z, u, mu)
    # two runs: the same bits
    _, z2, u2 = _iterate(cs)
    e.prox_dual(x, z2, u2, mu)
    assert _same(z, z2) and _same(u, u2)
    res = e.cg_residual()
    # a stopped slice keeps z, u bit for bit; the others give the bits of the run without a stop
    _, z3, u3 = _iterate(cs)
    z0, u0 = z3.clone(), u3.clone()
    e.prox_dual(x, z3, u3, mu, t_action=torch.tensor([0.0, 1.0, 0.0], device=DEV))
    assert _same(z3[1], z0[1]) and _same(u3[1], u0[1])
    assert _same(z3[0], z[0]) and _same(z3[2], z[2]) and _same(u3[0], u[0]) and _same(u3[2], u[2])
    assert _same(e.cg_residual(), res)                                             # the stopped slice keeps its earlier value
    # a non-default stream: the same bits
    side = torch.cuda.Stream()
    _, z4, u4 = _iterate(cs)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        e.prox_dual(x, z4, u4, mu)
    side.synchronize()
    assert _same(z4, z) and _same(u4, u)
    # every slice alone (a handle of one slice): the bits it has at its place in the batch
    e1 = _engine(1, h, w)
    for i in range(n):
        e1.set_kspace(c64(cs["y"][i:i + 1]), torch.from_numpy(cs["mask"][i:i + 1]).to(DEV), sens=c64(cs["sens"][i:i + 1]), cg_iters=K)
        xi, zi, ui = (t[i:i + 1].clone() for t in _iterate(cs))
        e1.prox_dual(xi, zi, ui, mu[i:i + 1].clone())
        assert _same(zi[0], z[i]) and _same(ui[0], u[i]), i
        assert _same(e1.cg_residual()[0], res[i]), i
    # ... and at another place: the batch reversed
    rev = {k: (np.ascontiguousarray(v[::-1]) if k != "aty" else v) for k, v in cs.items()}
    _install(e, rev, K)
    xr, zr, ur = _iterate(rev)
    e.prox_dual(xr, zr, ur, mu.flip(0).contiguous())
    assert _same(zr.flip(0), z) and _same(ur.flip(0), u)


def test_single_coil_reset_after_multi_coil_use_equals_a_fresh_handle():
    n, h, w = 2, 128, 128
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=9)
    x0, y0 = c64(d["x0"][..., 0] + 1j * d["x0"][..., 1]), c64(d["y0"][..., 0] + 1j * d["y0"][..., 1])
    mask = torch.from_numpy(d["mask"]).to(DEV)
    mu = torch.tensor([0.1, 0.4], device=DEV)
    used, fresh = _engine(n, h, w), _engine(n, h, w)
    ws0 = used.workspace_bytes
    cs = R.solve_case(h, w, 4, False, "radial", 8)
    _install(used, cs, 8)
    assert used.coils == 4 and used.workspace_bytes > ws0 + 2 * n * 4 * h * w * 8       # y and scratch at least
    xm, zm, um = _iterate(cs)
    used.prox_dual(xm, zm, um, mu)
    out = []
    for e in (used, fresh):
        x, z, u = e.reset(x0, y0, mask)
        assert e.coils == 0
        for _ in range(2):
            e.prox_dual(x, z, u, mu)
        out.append((x, z, u, e.residuals(x, z, u, dc=True)))
    for a, b in zip(*out):
        assert _same(a, b)
    with pytest.raises(Exception, match="single-coil"):
        used.cg_residual()
    ws1 = used.workspace_bytes
    _install(used, cs, 8)                                                           # a second install grows nothing
    assert used.workspace_bytes == ws1


def test_reset_mc_sets_the_iterate_and_the_normal_operator_matches_float64():
    n, h, w, coils = 2, 80, 160, 3
    cs = R.solve_case(h, w, coils, True, "radial", 4)
    e = _engine(n, h, w)
    x0 = c64(cs["z0"]).reshape(n, 1, h, w)
    x, z, u = e.reset(x0, c64(cs["y"]), torch.from_numpy(cs["mask"]).to(DEV), sens=c64(cs["sens"]), cg_iters=3)
    assert e.coils == coils
    assert _same(z, x0) and _same(x, x0.real.contiguous()) and not _bits(u).any()
    assert not e.cg_residual().any()                                                # 0 before the first solve
    p = c64(cs["u"]).reshape(n, 1, h, w)
    mu = torch.tensor([0.05, 0.6], device=DEV)
    q = _np(e.normal_op(p, mu))[:, 0]
    qr = R.nop(cs["u"], cs["sens"], cs["mask"], np.array([np.float32(0.05), np.float32(0.6)], dtype=np.float64))
    rel = _rel_rms(q, qr)
    print(f"Nop against float64: rel rms {rel:.3e}")
    assert rel <= 2 * REL_RMS                                                       # two transforms, the suite's 1e-6 each


def test_residuals_dc_in_multi_coil_mode():
    for (h, w, coils, ps) in ((128, 128, 4, False), (320, 320, 8, True), (80, 1024, 2, True)):
        cs = R.solve_case(h, w, coils, ps, "radial", 4)
        e = _engine(2, h, w)
        _install(e, cs, 4)
        x, z, u = _iterate(cs)
        got = e.residuals(x, z, u, dc=True).cpu().double().numpy()
        ref = R.dc_misfit(cs["x"], cs["y"], cs["sens"], cs["mask"])
        xn = np.sqrt((cs["x"].reshape(2, -1) ** 2).sum(1))
        ddc, bound = np.abs(got[:, 5] - ref), 1e-6 * xn + 5e-7 * ref
        print(f"{h}x{w} C={coils}: dc {got[:, 5]} ref {ref} |ddc| / bound {float((ddc / bound).max()):.3e}")
        assert (ddc <= bound).all()
        prim = np.sqrt((np.abs(cs["x"] - cs["z0"]) ** 2).reshape(2, -1).sum(1))
        assert np.abs(got[:, 0] - prim).max() <= 5e-7 * prim.max()


# ---- through PnPEnv --------------------------------------------------------------------------------------------------------------------

def _env(**kw):
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    return PnPEnv(30, UNetDenoiser2D.seeded(0, "unit_gain"), "cuda", **kw)


def _mat(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def test_interleaved_multi_and_single_coil_episodes_and_snapshots():
    n, h, w = 2, 64, 64
    mc = _mat(synthetic.make_problem_mc(n, h, w, 4, accel=4.0, seed=3))
    sc = _mat(synthetic.make_problem(n, h, w, accel=4.0, seed=4))
    act = [{"T": torch.zeros(n), "mu": torch.full((n,), 0.1 + 0.1 * k), "sigma_d": torch.full((n,), (40.0 - 5 * k) / 255.0)} for k in range(3)]

    def alone(mat):
        env = _env(cg_iters=4)
        st = env.reset(mat, "cuda")
        for a in act:
            st, _ = env.step(st, a)
        return st["x"].clone(), st["z"].clone(), st["u"].clone()

    want_mc, want_sc = alone(mc), alone(sc)
    env = _env(cg_iters=4)
    a, b = env.reset(mc, "cuda"), env.reset(sc, "cuda")          # one denoiser, one engine: the second reset replaces the constants
    assert a["sens"] is not None and b["sens"] is None and env._engine.coils == 0
    for k in range(3):
        a, _ = env.step(a, act[k])
        assert env._engine.coils == 4
        b, _ = env.step(b, act[k])
        assert env._engine.coils == 0
    for got, want in ((a, want_mc), (b, want_sc)):
        for key, t in zip(("x", "z", "u"), want):
            assert _same(got[key], t), key
    assert float((want_mc[0] - want_sc[0]).abs().max()) > 1e-3
    # snapshot and restore inside a multi-coil episode
    st = env.reset(mc, "cuda")
    st, _ = env.step(st, act[0])
    snap = env.snapshot(st)
    st, _ = env.step(st, act[1])
    st, _ = env.step(st, act[2])
    r = env.residuals(st, prev=snap, dc=True)
    assert bool((r[:, 4] > 0).all()) and bool((r[:, 5] > 0).all())
    env.restore(st, snap)
    st, _ = env.step(st, act[1])
    st, _ = env.step(st, act[2])
    for key, t in zip(("x", "z", "u"), want_mc):
        assert _same(st[key], t), key


def test_trajectory_against_the_float64_reference(record_property):
    t = R.TRAJ
    d, mu, sig = R.trajectory_problem()
    x64, p64 = R.trajectory(False)
    e = _engine(t["n"], t["h"], t["w"], denoiser=True)
    e.load_weights(weights.generate_unet_weights(t["weights_seed"], "unit_gain"))
    cplx = lambda a: c64(a[..., 0] + 1j * a[..., 1])
    x, z, u = e.reset(cplx(d["x0"]), cplx(d["y0"]), torch.from_numpy(d["mask"]).to(DEV), sens=c64(d["sens"]), cg_iters=t["cg_iters"])
    gt = f32(d["gt"])
    worst_dx = worst_dp = 0.0
    for k in range(t["steps"]):
        e.step(x, z, u, f32(mu[:, k]), f32(sig[:, k]))
        dx = float(np.abs(_np(x)[:, 0] - x64[k]).max())
        dp = float(np.abs(e.psnr(x, gt).cpu().double().numpy() - p64[k]).max())
        print(f"step {k + 1}: max |dx| = {dx:.3e}, |dPSNR| = {dp:.3e} dB, psnr64 {p64[k]}, cg_res {e.cg_residual().cpu().numpy()}")
        worst_dx, worst_dp = max(worst_dx, dx), max(worst_dp, dp)
    print(f"trajectory: max |dx| = {worst_dx:.3e} (bound {MARGIN * TRAJ_DX_F32:.2e}), |dPSNR| = {worst_dp:.3e} dB")
    record_property("max_abs_dx", worst_dx)                                         # recorded against ten times the oracle's own f32 drift
    record_property("max_abs_dx_reference", MARGIN * TRAJ_DX_F32)
    record_property("max_abs_dpsnr_db", worst_dp)
    assert worst_dp < 0.01


# ---- the timed sizes ---------------------------------------------------------------------------------------------------------------------

def _timed_case(n, h, w, coils=8):
    """n slices of one phantom family with shared maps and mask; float64 copies of slices 0 and n - 1 only."""
    sens = synthetic.coil_maps(coils, h, w).astype(np.complex64)
    mask = synthetic.radial_mask(h, w, 8)
    gt = np.stack([synthetic.phantom(h, w, 300 + i) for i in range(n)]).astype(np.float32)
    return gt, sens, mask


@pytest.mark.parametrize("n,h,w,kind", [(64, 256, 256, "f32"), (16, 512, 512, "f32"), (64, 256, 256, "bf16"), (16, 512, 512, "no_denoiser")])
def test_one_step_at_the_timed_sizes_on_two_slices(n, h, w, kind):
    coils, K, mu = 8, 8, 0.3
    gt, sens, mask = _timed_case(n, h, w)
    e = _engine(n, h, w, denoiser=kind != "no_denoiser", bf16_convs=kind == "bf16")
    if kind != "no_denoiser":
        e.load_weights(weights.generate_unet_weights(0, "unit_gain"))
    sd, md = c64(sens), torch.from_numpy(mask).to(DEV)
    y, aty, x0 = e.acquire(f32(gt).reshape(n, 1, h, w), md, 10.0 / 255.0, 7, sens=sd)
    x, z, u = e.reset(x0, y, md, sens=sd, cg_iters=K)
    u.copy_(0.05 * x0)                                                             # a non-trivial dual
    z_in, u_in = _np(z)[:, 0], _np(u)[:, 0]
    mut = torch.full((n,), mu, dtype=torch.float32, device=DEV)
    if kind == "no_denoiser":
        e.prox_dual(x, z, u, mut)
    else:
        e.step(x, z, u, mut, torch.full((n,), 20.0 / 255.0, dtype=torch.float32, device=DEV))
    res = e.cg_residual().cpu().numpy()
    xs, zs, us, ys = _np(x)[:, 0], _np(z)[:, 0], _np(u)[:, 0], _np(y)
    bmax, brms, bres = (MARGIN * v for v in F32[(mu, K)])
    for i in (0, n - 1):
        # the float64 data-fidelity stage on the GPU's own denoiser output: the check is of the new stage alone
        zr, ur, rr = R.prox_dual(xs[i:i + 1], z_in[i:i + 1], u_in[i:i + 1], ys[i:i + 1], sens, mask, np.array([np.float64(np.float32(mu))]), K)
        emax, erms = R.solve_errors(zs[i:i + 1], zr)
        umax = float(np.abs(us[i:i + 1] - ur).max() / np.abs(zr).max())
        dres = abs(res[i] - rr[0]) / rr[0]
        print(f"{kind} {n}x{h}x{w} slice {i}: err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}  cg_res {res[i]:.4e} "
              f"ref {rr[0]:.4e} d_res {dres:.3e}")
        assert emax <= bmax and erms <= brms and umax <= 2 * bmax and dres <= bres


# ---- drivers -----------------------------------------------------------------------------------------------------------------------------

def _cli(capsys, argv):
    from dt4image_restoration_amd import cli
    out = cli.main(argv)
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if l.startswith("{")]
    assert [json.loads(l) for l in lines] == out
    return lines, out


def test_cli_eval_and_fixed_with_coils(capsys):
    base = ["--block_size", "18", "--n_embeds", "9", "--limit", "2", "--coils", "4", "--cg-iters", "6"]
    _, out = _cli(capsys, base + ["eval", "--max_timesteps", "4", "--residuals"])
    assert len(out) == 2
    for o in out:
        assert o["n"] == 2 and all(np.isfinite(v) for v in o.values() if isinstance(v, float)) and o["dc"] > 0 and 5.0 < o["psnr"] < 60.0
    _, dev = _cli(capsys, base + ["--acquire", "device", "eval", "--max_timesteps", "4"])
    for a, b in zip(out, dev):                                                     # the problems acquired on the device: the same sets
        assert abs((a["psnr"] - a["psnr_increment"]) - (b["psnr"] - b["psnr_increment"])) < 1e-3
    _, fx = _cli(capsys, base + ["--size", "64", "fixed", "--mu", "0.3", "--sigma-start", "15", "--sigma-end", "15", "--tol", "0.02",
                                 "--max_iter", "16", "--dc"])
    print(fx)
    assert len(fx) == 2
    for o in fx:
        assert o["n"] == 2 and all(1 <= i <= 16 for i in o["iterations"]) and o["delta"] > 0 and o["dc"] > 0


def test_fixed_schedule_solver_stops_on_delta_on_a_multi_coil_problem():
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    n, h, w, iters = 2, 64, 64, 16
    mat = _mat(synthetic.make_problem_mc(n, h, w, 4, accel=4.0, seed=1234))
    run = lambda tol, max_iter=iters: FixedScheduleSolver(_env(cg_iters=6), max_iter=max_iter, tol=tol).run(
        mat, np.full((n, max_iter), 0.3, np.float32), np.full((n, max_iter), 15.0 / 255.0, np.float32))
    free = run(None)
    d = free.delta.numpy()
    print("delta:", d)
    assert (d > 0).all() and (d[:, -1] < d[:, 0]).all()
    tol = float(np.sqrt(d[:, 4] * d[:, 5]).max())                                  # between the deltas of iterations 5 and 6
    stopped = run(tol)
    its = stopped.iterations.tolist()
    print("tol", tol, "iterations", its)
    assert all(1 <= i < iters for i in its)
    for i, it in enumerate(its):
        assert d[i, it - 1] <= tol and (it == 1 or d[i, it - 2] > tol)             # the first iteration whose delta is under the tolerance
        short = run(None, max_iter=it)
        assert _same(stopped.x[i], short.x[i]) and _same(stopped.z[i], short.z[i])  # stopped there bit for bit
