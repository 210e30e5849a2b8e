"""Coil noise pre-whitening (pnp_noise_cov, pnp_whiten_matrix, pnp_whiten_apply) on the MI355X, through the C ABI, against the float64
restatement of tests/prewhiten_ref.py.  Every caller-owned buffer of the three entry points' own tests (covariance, matrix, apply, overlap)
comes from tests/guard_bands.py, the inputs frozen; the end-to-end, reconstruction and command-line tests go through the Python functions
(`acquisition.noise_scan` / `prewhiten` / `simulate`, `PnPEngine.*`), which allocate plain torch tensors themselves: plumbing around calls the
guarded tests already cover.  The reconstruction test hands the device the reference's start x0 (float64 `A^H y`, clipped, rounded once), so
that the comparison is of the whitening and the ten steps and not of a second transform.  Every figure is printed before it is asserted.

BOUNDS (none of them measured on the device).
  covariance   |dPsi[a][b]| <= 4 S 2^-53 (1 / S) sum_s |n_a| |n_b|: the float64 summation bound of S exact products (prewhiten_ref.cov_bound).
  matrix       |wmat - complex64(W_ref)| <= 2^-22 max |W_ref|, the same for lmat: the float64 factorisation error (~ cond C 2^-53) is far
               below one float32 rounding, so the bound is two roundings.
  apply        ten times the float32 restatement's own error (prewhiten_ref.apply_f32 against float64, max abs), measured on the CPU with
               the per-slice matrices of prewhiten_ref.case_planes:
                   N x C x H x W     2x3x16x16   1x8x16x80   3x17x32x16  1x33x16x16  1x64x16x32
                   max |f32 - f64|   2.024e-07   2.360e-07   3.035e-07   3.632e-07   7.652e-07
  end to end   covariance of the whitened scan within C 2^-21 of the identity (max norm): float32 rounding of W and of the mixed samples.
  pipeline     prewhiten_ref.FIXTURE (1 x 64 x 80, 8 coils, 4x Cartesian mask, rho 0.4, gain spread 6, sigma_n 4/255, TV prior, 10 steps, 8 CG
               iterations).  Measured on the CPU in float64: 26.304 dB with pre-whitening, 24.505 dB without: a gain of 1.799 dB, asserted on
               the device at half of it.  The float32 restatement of the whitened pipeline is within 8.508e-07 dB and max |dx| 2.598e-06 of the
               float64 one; the device is bound at ten times each (the rule of tests/test_gpu_tv.py).
"""
import io
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402
import prewhiten_ref as R  # noqa: E402
import sense_ref as SR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 10.0
APPLY_F32 = (2.024e-07, 2.360e-07, 3.035e-07, 3.632e-07, 7.652e-07)
REF_GAIN_DB = 1.799
PIPE_F32 = (8.508e-07, 2.598e-06)                          # |dPSNR| dB, max |dx|


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def _np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _bits(t):
    if t.dtype == torch.complex128:
        return torch.view_as_real(t).contiguous().view(torch.int64)
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def g_in(a, dtype, name):
    a = np.ascontiguousarray(a)
    return G.guarded(a.shape, dtype, DEV, fill=torch.from_numpy(a), name=name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def cov(e, noise):
    """pnp_noise_cov on guarded buffers: noise complex64 ndarray [M,C,S] -> psi tensor [M,C,C] complex128."""
    m, c, s = noise.shape
    x = g_in(noise, torch.complex64, "noise")
    psi = G.guarded((m, c, c), torch.complex128, DEV, name="psi")
    with G.watch(outputs={"psi": psi}, inputs={"noise": x}):
        _lib.check(e.lib.pnp_noise_cov(e._h, x.data_ptr(), m, c, s, 0, psi.data_ptr(), _stream()), "pnp_noise_cov")
    return psi


def factor(e, psi_np, with_l=True):
    p = np.asarray(psi_np, dtype=np.complex128)
    p = p[None] if p.ndim == 2 else p
    m, c, _ = p.shape
    psi = g_in(p, torch.complex128, "psi")
    wmat = G.guarded((m, c, c), torch.complex64, DEV, name="wmat")
    lmat = G.guarded((m, c, c), torch.complex64, DEV, name="lmat") if with_l else None
    info = G.guarded((m,), torch.int32, DEV, name="info")
    with G.watch(outputs={"wmat": wmat, "lmat": lmat, "info": info}, inputs={"psi": psi}):
        _lib.check(e.lib.pnp_whiten_matrix(e._h, psi.data_ptr(), m, c, 0, wmat.data_ptr(), lmat.data_ptr() if with_l else None, info.data_ptr(),
                                           _stream()), "pnp_whiten_matrix")
    return wmat, lmat, info


def mix(e, x_np, w_np, inplace=False):
    """pnp_whiten_apply on guarded buffers; returns the output tensor [N,C,H,W]."""
    n, c, h, w = x_np.shape
    w_np = np.asarray(w_np, dtype=np.complex64)
    wn = 1 if w_np.ndim == 2 else w_np.shape[0]
    x = g_in(x_np, torch.complex64, "in")
    wm = g_in(w_np.reshape(wn, c, c), torch.complex64, "wmat")
    if inplace:
        with G.watch(outputs={"in": x}, inputs={"wmat": wm}):
            _lib.check(e.lib.pnp_whiten_apply(e._h, x.data_ptr(), c, wm.data_ptr(), wn, x.data_ptr(), _stream()), "pnp_whiten_apply")
        return x
    out = G.guarded((n, c, h, w), torch.complex64, DEV, name="out")
    with G.watch(outputs={"out": out}, inputs={"in": x, "wmat": wm}):
        _lib.check(e.lib.pnp_whiten_apply(e._h, x.data_ptr(), c, wm.data_ptr(), wn, out.data_ptr(), _stream()), "pnp_whiten_apply")
    return out


# ---- covariance ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def e16():
    return _engine(2, 16, 16)


@pytest.mark.parametrize("s", R.COV_SAMPLES)
@pytest.mark.parametrize("c", R.COV_COILS)
def test_covariance_against_float64(c, s, e16):
    noise = R.case_noise(2, c, s)
    psi = _np(cov(e16, noise))
    ref, bound = R.cov(noise), R.cov_bound(noise)
    err = np.abs(psi - ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"C {c} S {s}: max |dPsi| {err.max():.3e}, largest |dPsi| / bound {worst:.3e}")
    assert (err <= bound).all()
    assert np.array_equal(psi, psi.conj().transpose(0, 2, 1)) and not psi[:, np.arange(c), np.arange(c)].imag.any()


def test_covariance_bits_do_not_depend_on_the_batch_the_stream_the_call_or_the_handle(e16):
    c, s = 5, 5000
    noise = R.case_noise(3, c, s)
    whole = cov(e16, noise)
    assert _same(whole, cov(e16, noise))
    for k in range(3):
        assert _same(cov(e16, noise[k:k + 1])[0], whole[k])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = cov(e16, noise)
    side.synchronize()
    assert _same(on_side, whole)
    other = _engine(1, 32, 16, denoiser=True, bf16_convs=True)
    assert _same(cov(other, noise), whole)


# ---- matrix --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.COV_COILS)
def test_matrix_against_float64(c, e16):
    psi = R.case_psi(c)
    W, L, info = R.factor(psi)
    assert info == 0
    wmat, lmat, inf = factor(e16, psi)
    w, l = _np(wmat)[0], _np(lmat)[0]
    ew, el = float(np.abs(w - R.rounded(W)).max()), float(np.abs(l - R.rounded(L)).max())
    bw, bl = 2.0 ** -22 * np.abs(W).max(), 2.0 ** -22 * np.abs(L).max()
    print(f"C {c} cond {np.linalg.cond(psi):.3g}: |dW| {ew:.3e} / {bw:.3e}  |dL| {el:.3e} / {bl:.3e}")
    assert int(inf[0]) == 0 and ew <= bw and el <= bl
    iu = torch.triu_indices(c, c, 1, device=DEV)
    for m in (wmat, lmat):
        assert not bool(_bits(m)[0][iu[0], iu[1]].any())                         # exact +0 above the diagonal
    w_only, none, _ = factor(e16, psi, with_l=False)
    assert none is None and _same(w_only, wmat)


@pytest.mark.parametrize("c", (1, 8, 64))
def test_the_identity_gives_the_identity_bit_for_bit(c, e16):
    wmat, lmat, info = factor(e16, np.eye(c))
    eye = torch.eye(c, dtype=torch.complex64, device=DEV)[None]
    assert int(info[0]) == 0 and _same(wmat, eye) and _same(lmat, eye)


def test_an_indefinite_matrix_is_flagged_gives_the_identity_and_leaves_its_neighbour_alone(e16):
    c = 8
    good = R.case_psi(c)
    bad = good.copy()
    bad[5, 5] = -1.0                                                             # pivot 5 is the first to fail
    assert R.factor_one(bad)[2] == 6
    nan = good.copy()
    nan[3, 1] = np.nan
    wg, lg, _ = factor(e16, good)
    wmat, lmat, info = factor(e16, np.stack([good, bad, nan, np.zeros((c, c))]))
    eye = torch.eye(c, dtype=torch.complex64, device=DEV)
    print("info", info.tolist())
    assert info.tolist() == [0, 6, R.factor_one(nan)[2], 1]
    assert _same(wmat[0], wg[0]) and _same(lmat[0], lg[0])
    for k in (1, 2, 3):
        assert _same(wmat[k], eye) and _same(lmat[k], eye)
    assert bool(torch.isfinite(torch.view_as_real(wmat)).all())


# ---- apply ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(R.APPLY_CASES)))
def test_apply_against_float64_and_its_bit_for_bit_properties(i):
    n, c, h, w = R.APPLY_CASES[i]
    x, wm = R.case_planes(i)
    e = _engine(n, h, w)
    out = mix(e, x, wm)
    err = float(np.abs(_np(out) - R.apply(wm, x)).max())
    print(f"case {i} {R.APPLY_CASES[i]}: max |out - float64| {err:.3e} / {MARGIN * APPLY_F32[i]:.2e}")
    assert err <= MARGIN * APPLY_F32[i]
    assert _same(mix(e, x, wm, inplace=True), out)                               # in place
    one = mix(e, x, wm[0])
    assert _same(mix(e, x, np.stack([wm[0]] * n)), one)                          # wmat_n = 1 against the matrix repeated
    assert _same(mix(e, x, wm[0], inplace=True), one)
    xt = torch.from_numpy(x).to(DEV)
    ident = mix(e, x, np.eye(c, dtype=np.complex64))
    assert _same(ident, xt + 0.0)                                                # the identity copies the planes (a -0 comes out as +0)
    junk = wm.copy()
    junk[:, np.triu_indices(c, 1)[0], np.triu_indices(c, 1)[1]] = np.complex64(complex(np.nan, 3e38))
    assert _same(mix(e, x, junk), out)                                           # nothing above the diagonal is read
    assert not bool(_bits(out).reshape(n, c, h * w, 2)[:, :, 5].any())           # a bin that is zero in every coil stays (+)zero
    if c <= 32:
        low = np.tril(wm)
        assert _same(e.coil_compress_apply(xt, torch.from_numpy(low).to(DEV), c), out)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = mix(e, x, wm)
    side.synchronize()
    assert _same(on_side, out)
    if n > 1:
        e1 = _engine(1, h, w, denoiser=(i == 0))
        for k in range(n):
            assert _same(mix(e1, x[k:k + 1], wm[k:k + 1])[0], out[k])
    else:
        e3 = _engine(3, h, w)
        for k in range(3):
            xx = np.stack([x[0] * np.float32(2)] * 3)
            xx[k] = x[0]
            assert _same(mix(e3, xx, wm[0])[k], out[0])


def test_apply_refuses_partial_overlap_and_a_wrong_matrix_count():
    e = _engine(2, 16, 16)
    c = 4
    buf = G.guarded((2 * 2, c, 16, 16), torch.complex64, DEV, fill=1.0, name="buf")
    wm = G.guarded((3, c, c), torch.complex64, DEV, fill=0.0, name="wmat")
    before = G.snapshot(buf)
    base = buf.data_ptr()
    for off in (8, 2048 * c, 16 * 16 * 8 * c, 2 * c * 16 * 16 * 8 - 8):
        assert e.lib.pnp_whiten_apply(e._h, base, c, wm.data_ptr(), 1, base + off, None) == -1 and b"overlap" in e.lib.pnp_last_error()
        assert e.lib.pnp_whiten_apply(e._h, base + off, c, wm.data_ptr(), 1, base, None) == -1 and b"overlap" in e.lib.pnp_last_error()
    assert e.lib.pnp_whiten_apply(e._h, base, c, wm.data_ptr(), 3, base, None) == -1 and b"wmat_n" in e.lib.pnp_last_error()
    assert e.lib.pnp_whiten_apply(e._h, base, c, base + 64, 1, base, None) == -1 and b"alias" in e.lib.pnp_last_error()
    G.check({"buf": buf, "wmat": wm}, {"buf": before})
    assert e.lib.pnp_whiten_apply(e._h, base, c, wm.data_ptr(), 1, base + 2 * c * 16 * 16 * 8, None) == 0    # adjacent: no overlap
    G.check({"buf": buf, "wmat": wm})


# ---- algebraic end to end --------------------------------------------------------------------------------------------------------------

def test_whitening_a_scan_by_its_own_covariance_gives_the_identity_and_the_workspace_grows_once():
    c, s = 8, 4096
    e = _engine(1, 64, 64)
    psi_model = synthetic.noise_cov_model(c, 0.5, 5.0, 9)
    scan = acquisition.noise_scan(e, c, s, noise_cov=psi_model, sigma_n=0.7, seed=31)
    assert scan.shape == (c, s) and scan.dtype == torch.complex64
    ws0 = e.workspace_bytes
    psi = e.noise_cov(scan)
    ws1 = e.workspace_bytes
    assert ws1 - ws0 == R.workspace_bytes(1, c, s) == 16 * c * c * 4
    est = float(np.abs(_np(psi) / (2 * 0.7 ** 2) - psi_model).max() / np.abs(psi_model).max())
    print(f"covariance of the scan against the model (statistical, S = {s}): relative {est:.3e}")
    wmat, lmat, info = e.whiten_matrix(psi)
    assert int(info[0]) == 0
    planes = scan.reshape(c, 1, 64, 64).permute(1, 0, 2, 3).contiguous().clone()    # (one slice: the permuted view IS contiguous - copy, the scan is read again below)
    e.whiten_apply(planes, wmat, out=planes)
    again = _np(e.noise_cov(planes.reshape(c, s)))
    err = float(np.abs(again - np.eye(c)).max())
    print(f"covariance of the whitened scan: max |Psi' - I| {err:.3e} / {c * 2.0 ** -21:.3e}")
    assert err <= c * 2.0 ** -21
    assert e.workspace_bytes == ws1 and e.coils == 0                            # later calls allocate nothing; the mode is untouched
    # the scan is the white scan of the same seed mixed by the MODEL's factor L (not the measured one): scan = L white, up to the float32
    # accumulation of the mix, 4 C operations per output: |d| <= 4 C 2^-24 (|L| |white|), entry by entry
    white = _np(acquisition.noise_scan(e, c, s, sigma_n=0.7, seed=31))
    lm = np.tril(_np(e.whiten_matrix(torch.from_numpy(psi_model).to(DEV))[1]))
    d = np.abs(lm @ white - _np(scan))
    bound = 4 * c * 2.0 ** -24 * (np.abs(lm) @ np.abs(white))
    print(f"scan against L white: max |d| {d.max():.3e}, largest |d| / bound {float((d / bound).max()):.3e}")
    assert (d <= bound).all()


# ---- reconstruction ----------------------------------------------------------------------------------------------------------------------

def _device_pipeline(prewhiten):
    t, d = R.FIXTURE, R.fixture()
    n, h, w = t["n"], t["h"], t["w"]
    e = _engine(n, h, w)
    e.set_prior("tv", t["tv_scale"], t["tv_iters"])
    y = torch.from_numpy(d["y"]).to(DEV)
    sens = torch.from_numpy(d["sens"]).to(DEV)
    if prewhiten:
        y, sens, wmat, psi = acquisition.prewhiten(e, y, torch.from_numpy(d["scan"]).to(DEV), sens=sens)
        assert wmat.shape == (t["coils"], t["coils"]) and psi.dtype == torch.complex128
    x0 = torch.from_numpy(R.pipeline(prewhiten)[2].astype(np.complex64)).to(DEV).reshape(n, 1, h, w)
    x, z, u = e.reset(x0, y, torch.from_numpy(d["mask"]).to(DEV), sens=sens, cg_iters=t["cg_iters"])
    for k in range(t["iters"]):
        e.step(x, z, u, torch.full((n,), float(d["mu"][k]), device=DEV), torch.full((n,), float(d["sigma"][k]), device=DEV))
    xs = _np(x)[:, 0]
    return xs, SR.psnr(xs, d["gt"])


def test_the_whitened_reconstruction_against_the_float64_pipeline_and_its_gain_over_no_whitening():
    xr, pr, _ = R.pipeline(True)
    _, pr_raw, _ = R.pipeline(False)
    gain_ref = float((pr - pr_raw)[0])
    print(f"reference: {pr[0]:.4f} dB whitened, {pr_raw[0]:.4f} dB raw, gain {gain_ref:.4f} dB (recorded {REF_GAIN_DB})")
    assert abs(gain_ref - REF_GAIN_DB) <= 2e-3 and gain_ref >= 0.5
    xd, pd = _device_pipeline(True)
    _, pd_raw = _device_pipeline(False)
    dp, dx = float(np.abs(pd - pr).max()), float(np.abs(xd - xr).max())
    gain = float((pd - pd_raw)[0])
    print(f"device: {pd[0]:.4f} dB whitened, {pd_raw[0]:.4f} dB raw, gain {gain:.4f} dB; |dPSNR| {dp:.3e} / {MARGIN * PIPE_F32[0]:.2e} dB, "
          f"max |dx| {dx:.3e} / {MARGIN * PIPE_F32[1]:.2e}")
    assert gain >= 0.5 * REF_GAIN_DB
    assert dp <= MARGIN * PIPE_F32[0] and dx <= MARGIN * PIPE_F32[1]


# ---- command line ------------------------------------------------------------------------------------------------------------------------

def test_cli_prewhiten_runs_and_prints_the_psnr_of_the_python_pipeline():
    from dt4image_restoration_amd import cli
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    size, coils, rho, seed, iters, limit = 64, 8, 0.4, 3, 6, 2
    argv = ["--block_size", "6", "--n_embeds", "9", "--size", str(size), "--limit", str(limit), "--coils", str(coils), "--noise-cov", str(rho),
            "--prewhiten", "--sens", "estimate", "--mask", "cartesian", "--prior", "tv", "--seed", str(seed), "fixed", "--max_iter", str(iters)]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = cli.main(argv)
    lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
    assert len(lines) == 2 and [l["psnr"] for l in lines] == [o["psnr"] for o in out] and all(np.isfinite(l["psnr"]) for l in lines)
    # the same run from the Python functions: the first synthetic set (4x, sigma_n 10 / 255)
    accel, sig = 4, 10
    env = PnPEnv(max_episode_step=iters, denoiser=TVDenoiser2D(), device_type="cuda", cg_iters=8)
    solver = FixedScheduleSolver(env, max_iter=iters, tol=None, sync_every=5, device_type=torch.device("cuda", torch.cuda.current_device()))
    psi = synthetic.noise_cov_model(coils, rho, 1.0, seed)
    mask = acquisition.make_mask(size, size, accel, "cartesian", seed)
    gt = np.stack([synthetic.phantom(size, size, seed + accel + i) for i in range(limit)]).astype(np.float32)
    p = acquisition.simulate(env, gt, mask, sig / 255.0, seed + accel, sens=synthetic.coil_maps(coils, size, size).astype(np.complex64),
                             noise_cov=psi)
    scan = acquisition.noise_scan(env, coils, acquisition.SCAN_SAMPLES, noise_cov=psi, sigma_n=acquisition.unit_scan_sigma(psi),
                                  seed=seed + acquisition.SCAN_SEED)
    y, none, wmat, _ = acquisition.prewhiten(env, p["y0"], scan)
    assert none is None
    p["y0"] = torch.view_as_real(y)
    p["sens"] = acquisition.estimate_sens(env, p["y0"], mask=p["mask"], window="hann", thresh=0.05)
    t = np.arange(iters) / max(iters - 1, 1)
    sigma = (50.0 * (5.0 / 50.0) ** t / 255.0).astype(np.float32)
    r = solver.run(p, np.full((limit, iters), 0.3, dtype=np.float32), np.tile(sigma, (limit, 1)))
    want = float(r.psnr.mean())
    print("cli", lines[0]["psnr"], "python", want)
    assert lines[0]["psnr"] == want
