"""Simulated CS-MRI acquisition on the device: ground-truth images in, the reference's evaluation-data layout out.

The reference evaluates on `.mat` files holding `x0, y0, ATy0, mask, gt` (dataset/datasets.py:153-160,191-199), one folder per
task `2x_5 ... 8x_15`; the files are an external download.  `synthetic.make_problem` builds the same dict on the CPU in numpy
float64 from an analytic phantom.  `simulate` builds it on the GPU (pnp_acquire) from ANY ground truth - phantoms or a folder of
images read by `data.load_gt_dir` - with the noise `make_problem` draws, number for number:

    y0 = mask * (fft_c(gt) + sigma_n * (g_re + i g_im)),  ATy0 = ifft_c(y0),  x0 = max(ATy0, 0) on both planes

and `PnPEnv.reset` takes the result as it stands, without a trip through host memory.
"""
from __future__ import annotations

import math
import re
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib, synthetic
from .weights import hash_uniform

MASK_KINDS = ("radial", "cartesian", "uniform")
NC_KINDS = ("radial-nc", "spiral-nc", "rosette-nc")          # task_problem: non-Cartesian acquisitions (no mask: a trajectory)


def _engine(engine_or_env, n: int, h: int, w: int, device: torch.device):
    if hasattr(engine_or_env, "acquire"):
        return engine_or_env
    if hasattr(engine_or_env, "_engine_for"):                # a PnPEnv: the handle its reset will use for this shape
        return engine_or_env._engine_for(n, h, w, device)
    raise TypeError(f"simulate: expected a PnPEngine or a PnPEnv, got {type(engine_or_env).__name__}")


SCAN_SAMPLES = 4096          # samples per channel of the noise-only scan the command line takes
SCAN_SEED = 9000             # ... and the offset of its seed from the run's


def unit_scan_sigma(noise_cov=None) -> float:
    """The sigma_n at which `noise_scan(..., noise_cov)` has a mean channel variance of 1 (sigma_n^2 * 2 * mean diag Psi = 1): whitening by
    that scan's covariance keeps the overall scale of the data, so a penalty mu means the same with and without it."""
    d = 1.0 if noise_cov is None else float(np.real(np.diagonal(np.asarray(torch.as_tensor(noise_cov).cpu()))).mean())
    return 1.0 / math.sqrt(2.0 * d)


def _factor(eng, noise_cov, coils: int):
    """(wmat, lmat) complex64 [C,C] of a covariance [C,C] on the engine's device (pnp_whiten_matrix); PnPError when it is not positive
    definite.  Reads the one int32 `info` back: a setup-time step."""
    psi = torch.as_tensor(noise_cov)
    if psi.dim() != 2 or tuple(psi.shape) != (coils, coils):
        raise ValueError(f"noise_cov: expected [{coils},{coils}], got {tuple(psi.shape)}")
    wmat, lmat, info = eng.whiten_matrix(psi.to(eng.device, torch.complex128).contiguous())
    bad = int(info[0])
    if bad:
        raise _lib.PnPError(f"noise_cov is not positive definite: the pivot of column {bad - 1} fails (pnp_whiten_matrix info = {bad})")
    return wmat, lmat


def noise_scan(engine_or_env, coils: int, samples: int, noise_cov=None, sigma_n: float = 1.0, seed: int = 0) -> torch.Tensor:
    """A noise-only scan on the device: complex64 [coils, samples] with covariance sigma_n^2 * 2 * noise_cov (each white sample is
    sigma_n (g_re + i g_im) with unit-variance parts, as in `simulate`), for `PnPEngine.noise_cov` / `prewhiten`.  The white noise is
    pnp_acquire_mc's, run with gt = 0 and a full mask (so coils <= 32), mixed by L (noise_cov = L L^H) with pnp_whiten_apply in place;
    noise_cov None leaves it white.  Sample s of coil c is bin s of the engine's [N,H,W] planes in row-major order, so samples <=
    N H W.  A PnPEnv is asked for a handle of ceil(samples / 4096) slices of 64 x 64."""
    coils, samples = int(coils), int(samples)
    if not 1 <= coils <= 32:
        raise ValueError(f"noise_scan: coils must be 1..32, got {coils}")
    if samples < 1:
        raise ValueError(f"noise_scan: samples must be >= 1, got {samples}")
    if not torch.cuda.is_available():
        raise RuntimeError("noise_scan needs a ROCm GPU")
    eng = engine_or_env if hasattr(engine_or_env, "acquire") else None
    if eng is None:
        eng = _engine(engine_or_env, (samples + 4095) // 4096, 64, 64, torch.device("cuda", torch.cuda.current_device()))
    n, h, w = eng.n, eng.h, eng.w
    if samples > n * h * w:
        raise ValueError(f"noise_scan: the engine [{n},{h},{w}] holds {n * h * w} samples per coil, fewer than {samples}")
    lmat = _factor(eng, noise_cov, coils)[1] if noise_cov is not None else None
    gt = torch.zeros((n, 1, h, w), dtype=torch.float32, device=eng.device)
    ones = torch.ones((h, w), dtype=torch.bool, device=eng.device)
    sens = torch.ones((coils, h, w), dtype=torch.complex64, device=eng.device)
    y = eng.acquire(gt, ones, float(sigma_n), int(seed), sens=sens)[0]
    if lmat is not None:
        eng.whiten_apply(y, lmat, out=y)
    return y.permute(1, 0, 2, 3).reshape(coils, n * h * w)[:, :samples].contiguous()


def prewhiten(engine_or_env, y0, noise, sens=None, inplace: bool = True):
    """Noise pre-whitening on the device (pnp_noise_cov, pnp_whiten_matrix, pnp_whiten_apply): the head of the chain whiten -> compress
    -> maps -> SENSE.  y0: multi-coil k-space, complex [N,C,H,W] or real [N,C,H,W,2]; noise: a noise-only scan complex64 [C,S] (e.g.
    `noise_scan`); sens: the coil maps, complex [C,H,W] or [N,C,H,W], mixed by the same W (the maps of whitened data are W S), or None -
    estimate them from the whitened k-space afterwards.  inplace: y0 (when it already is a contiguous complex64 tensor on the engine's
    device) and a per-slice sens are overwritten, no second [N,C,H,W] buffer.  Returns (y0_w, sens_w or None, wmat complex64 [C,C], psi
    complex128 [C,C]); raises PnPError when the measured covariance is not positive definite (info != 0) - the one host read, made at
    setup time.  Whitened noise has covariance I: sigma_n^2 * 2 * Psi of `noise_scan` becomes unit variance per complex sample."""
    y = torch.as_tensor(y0)
    if not y.is_complex():
        if y.dim() != 5 or y.shape[-1] != 2:
            raise ValueError(f"y0: expected complex [N,C,H,W] or real [N,C,H,W,2], got {tuple(y.shape)}")
        y = torch.view_as_complex(y.float().contiguous())
    if y.dim() != 4:
        raise ValueError(f"y0: expected [N,C,H,W], got {tuple(y.shape)}")
    n, c, h, w = (int(v) for v in y.shape)
    nz = torch.as_tensor(noise)
    if not nz.is_complex() or nz.dim() != 2 or nz.shape[0] != c:
        raise ValueError(f"noise: expected complex [{c},S], got {tuple(nz.shape)}")
    s = None
    if sens is not None:
        s = torch.as_tensor(sens)
        if not s.is_complex() or s.dim() not in (3, 4) or tuple(s.shape[-3:]) != (c, h, w) or (s.dim() == 4 and s.shape[0] != n):
            raise ValueError(f"sens: expected complex [{c},{h},{w}] or [{n},{c},{h},{w}], got {tuple(s.shape)}")
    if not torch.cuda.is_available():
        raise RuntimeError("prewhiten needs a ROCm GPU")
    eng = engine_or_env if hasattr(engine_or_env, "whiten_apply") else None
    if eng is None:
        eng = _engine(engine_or_env, n, h, w, torch.device("cuda", torch.cuda.current_device()))
    if (eng.n, eng.h, eng.w) != (n, h, w):
        raise ValueError(f"y0 {tuple(y.shape)} does not fit the engine [{eng.n},{eng.h},{eng.w}]")
    psi = eng.noise_cov(nz.to(eng.device, torch.complex64).contiguous())
    wmat, _ = _factor(eng, psi, c)
    y = y.to(eng.device, torch.complex64).contiguous()
    y = eng.whiten_apply(y, wmat, out=y if inplace else None)
    if s is not None:
        s = s.to(eng.device, torch.complex64)
        if s.dim() == 3:
            s = s[None].expand(n, c, h, w).contiguous()      # one matrix, but whitened maps are stored per slice: [N,C,H,W] for `reset`
            s = eng.whiten_apply(s, wmat, out=s)
        else:
            s = s.contiguous()
            s = eng.whiten_apply(s, wmat, out=s if inplace else None)
    return y, s, wmat, psi


def radial_trajectory(h: int, w: int, spokes: int, readout: int = None, golden: bool = True) -> np.ndarray:
    """float64 [spokes * R, 2]: the (ky, kx) of a radial acquisition in cycles per pixel (include/pnpadmm.h, "non-Cartesian sampling").
    Spoke s has the angle s pi (sqrt 5 - 1) / 2 (golden) or s pi / spokes; its R = readout (default 2 max(h, w)) samples sit at
    r_j = (j - R/2) / R, (ky, kx) = (r sin, r cos).  Sample j of spoke s is row s R + j."""
    spokes = int(spokes)
    R = 2 * max(int(h), int(w)) if readout is None else int(readout)
    if spokes < 1 or R < 2:
        raise ValueError(f"radial_trajectory: need spokes >= 1 and readout >= 2, got {spokes}, {R}")
    r = (np.arange(R, dtype=np.float64) - R / 2) / R
    out = np.empty((spokes, R, 2), dtype=np.float64)
    for s in range(spokes):
        a = s * math.pi * (math.sqrt(5.0) - 1.0) / 2.0 if golden else s * math.pi / spokes
        out[s, :, 0] = r * math.sin(a)
        out[s, :, 1] = r * math.cos(a)
    return out.reshape(-1, 2)


def radial_dcf(traj, h: int, w: int) -> np.ndarray:
    """float32 [M]: the ramp density compensation of a radial trajectory, max(|r|, 1 / (2 R)) scaled so that the weights sum to h w (the
    slice size is not in the trajectory).  R, the readout length, is read from the trajectory itself: the first two samples of a
    `radial_trajectory` are 1 / R apart."""
    t = np.asarray(traj.detach().cpu().numpy() if isinstance(traj, torch.Tensor) else traj, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 2:
        raise ValueError(f"radial_dcf: expected a radial trajectory [M,2] with M >= 2, got {t.shape}")
    step = float(np.hypot(*(t[1] - t[0])))
    if not step > 0.0:
        raise ValueError("radial_dcf: the first two samples coincide: not a radial_trajectory")
    R = int(round(1.0 / step))
    d = np.maximum(np.hypot(t[:, 0], t[:, 1]), 1.0 / (2.0 * R))
    return (d * (h * w / d.sum())).astype(np.float32)


def spiral_trajectory(h: int, w: int, interleaves: int, readout: int = None, turns: float = None) -> np.ndarray:
    """float64 [interleaves * R, 2]: the (ky, kx) of an Archimedean spiral acquisition in cycles per pixel.  Sample j of interleaf l (row
    l R + j) sits at t = j / R, a = 2 pi (turns t + l / L), (ky, kx) = (0.5 t sin a, 0.5 t cos a): every interleaf starts at k = 0 and
    |k| < 0.5.  turns (default ceil(max(h, w) / (2 L)), at least 1): revolutions per interleaf; the default puts neighbouring arms of the
    L interleaves 1 / max(h, w) apart, the Nyquist spacing.  readout (default max(2 max(h, w), ceil(pi turns max(h, w)))): samples per
    interleaf; the default keeps the step along the arm at the edge, pi turns / R, within 1 / max(h, w)."""
    L, side = int(interleaves), max(int(h), int(w))
    if L < 1:
        raise ValueError(f"spiral_trajectory: need interleaves >= 1, got {L}")
    turns = float(max(1, math.ceil(side / (2.0 * L)))) if turns is None else float(turns)
    R = max(2 * side, int(math.ceil(math.pi * turns * side))) if readout is None else int(readout)
    if R < 2 or not turns > 0.0:
        raise ValueError(f"spiral_trajectory: need readout >= 2 and turns > 0, got {R}, {turns}")
    t = np.arange(R, dtype=np.float64) / R
    out = np.empty((L, R, 2), dtype=np.float64)
    for l in range(L):
        a = 2.0 * math.pi * (turns * t + l / L)
        out[l, :, 0] = 0.5 * t * np.sin(a)
        out[l, :, 1] = 0.5 * t * np.cos(a)
    return out.reshape(-1, 2)


def rosette_trajectory(h: int, w: int, petals: int, readout: int = None) -> np.ndarray:
    """float64 [R, 2]: the (ky, kx) of a rosette in cycles per pixel, one shot.  Sample j sits at t = j / R, r = 0.5 sin(pi petals t),
    a = pi (petals - 2) t, (ky, kx) = (r sin a, r cos a): `petals` petals through k = 0, |k| <= 0.5 (0.5 itself only where a sample
    falls on a petal's tip).  readout (default ceil(pi petals max(h, w) / 2)): the default keeps the step along the curve, at most
    pi petals / (2 R), within 1 / max(h, w)."""
    P, side = int(petals), max(int(h), int(w))
    if P < 1:
        raise ValueError(f"rosette_trajectory: need petals >= 1, got {P}")
    R = int(math.ceil(0.5 * math.pi * P * side)) if readout is None else int(readout)
    if R < 2:
        raise ValueError(f"rosette_trajectory: need readout >= 2, got {R}")
    t = np.arange(R, dtype=np.float64) / R
    r = 0.5 * np.sin(math.pi * P * t)
    a = math.pi * (P - 2) * t
    return np.stack([r * np.sin(a), r * np.cos(a)], axis=1)


def readout_times(traj_kind: str, m: int, readout: int, t_read: float, te: float = 0.0) -> np.ndarray:
    """float64 [m] seconds: the time of every sample of a `radial_trajectory`, `spiral_trajectory` or `rosette_trajectory` of m samples.  The
    generators emit `readout` samples per spoke / interleaf / petal (a rosette is one shot: readout = m), in order; sample i of each is taken
    at te + i t_read / readout.  traj_kind: "radial", "spiral" or "rosette"."""
    m, readout = int(m), int(readout)
    if traj_kind not in ("radial", "spiral", "rosette"):
        raise ValueError(f"readout_times: traj_kind must be radial, spiral or rosette, got {traj_kind!r}")
    if readout < 1 or m < 1 or m % readout:
        raise ValueError(f"readout_times: m = {m} is not a whole number of readouts of {readout} samples")
    if not (math.isfinite(t_read) and t_read > 0.0 and math.isfinite(te)):
        raise ValueError(f"readout_times: need t_read > 0 and a finite te, got {t_read}, {te}")
    return np.tile(float(te) + np.arange(readout, dtype=np.float64) * float(t_read) / readout, m // readout)


def offres_segments(omega_max: float, span: float, tol: float = 1e-3) -> int:
    """The smallest number of time segments L whose linear interpolator keeps the model error of include/pnpadmm_offres.h,
    1 - cos(omega_max D / 2) with D = span / (L - 1), within tol: omega_max in rad/s, span = t_max - t_min in seconds.  1 where there is
    nothing to correct (omega_max span = 0).  The answer is arithmetic and may exceed what pnp_offres_plan takes (`OFFRES_MAX_SEGMENTS`): the
    linear interpolator needs about 11 segments per radian of omega_max span at tol = 1e-3; `offres_bound` gives the error of a given L."""
    omega_max, span = abs(float(omega_max)), float(span)
    if not (math.isfinite(omega_max) and math.isfinite(span) and span >= 0.0 and 0.0 < tol < 1.0):
        raise ValueError(f"offres_segments: need finite omega_max, span >= 0 and 0 < tol < 1, got {omega_max}, {span}, {tol}")
    if omega_max * span == 0.0:
        return 1
    L = max(2, int(omega_max * span / (2.0 * math.acos(1.0 - tol))))              # from just below the closed form, then exactly
    while not (omega_max * span / (L - 1) / 2.0 <= math.pi and 1.0 - math.cos(omega_max * span / (L - 1) / 2.0) <= tol):
        L += 1
    while L > 2 and omega_max * span / (L - 2) / 2.0 <= math.pi and 1.0 - math.cos(omega_max * span / (L - 2) / 2.0) <= tol:
        L -= 1
    return L


OFFRES_MAX_SEGMENTS = _lib.PNP_MC_MAX_COILS                  # segments pnp_offres_plan takes


def offres_bound(omega_max: float, span: float, segments: int) -> float:
    """The model error 1 - cos(omega_max D / 2), D = span / (segments - 1), of `segments` >= 2 time segments (per unit of ||p||_1)."""
    if int(segments) < 2:
        raise ValueError(f"offres_bound: need segments >= 2, got {segments}")
    return 1.0 - math.cos(min(abs(float(omega_max)) * float(span) / (int(segments) - 1) / 2.0, math.pi))


OFFRES_LS_RIDGE = 1e-10                                      # kOffresLsRidge of csrc/offres_ls_plan.h


def _sinc(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    safe = np.where(x == 0.0, 1.0, x)
    return np.where(x == 0.0, 1.0, np.sin(safe) / safe)


def offres_ls_centres(times, segments: int) -> np.ndarray:
    """float64 [L]: the segment centres of pnp_offres_plan / pnp_offres_plan_ls: t_min + l D, D = span / (L - 1); L = 1: the midpoint."""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    L, lo, hi = int(segments), float(t.min()), float(t.max())
    if L == 1:
        return np.array([0.5 * (lo + hi)])
    return lo + np.arange(L, dtype=np.float64) * ((hi - lo) / (L - 1))


def offres_ls_coeffs(times, segments: int, omega_max: float) -> np.ndarray:
    """float64 [L, M]: the numpy statement of the least-squares temporal interpolator's plan (include/pnpadmm_offres_ls.h): b(t) = G^-1 r(t)
    with G[l][l'] = sinc(omega_max (tau_l - tau_l')) + OFFRES_LS_RIDGE [l == l'], r_l(t) = sinc(omega_max (t - tau_l)), by a float64 Cholesky
    factor of G.  L = 1: all ones.  The library stores float32(b); G is ill-conditioned by design, so two correct solvers may differ in b far
    more than in the fit (`offres_ls_error` measures the fit)."""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    L, om = int(segments), float(omega_max)
    if not 1 <= L <= OFFRES_MAX_SEGMENTS or t.size < 1 or not np.isfinite(t).all():
        raise ValueError(f"offres_ls_coeffs: need 1 <= segments <= {OFFRES_MAX_SEGMENTS} and finite times, got {L}")
    if L == 1:
        return np.ones((1, t.size))
    if not (math.isfinite(om) and om > 0.0 and t.max() > t.min()):
        raise ValueError(f"offres_ls_coeffs: segments = {L} needs a finite omega_max > 0 and times of a positive span, got {omega_max}")
    tau = offres_ls_centres(t, L)
    G = _sinc(om * (tau[:, None] - tau[None, :])) + OFFRES_LS_RIDGE * np.eye(L)
    C = np.linalg.cholesky(G)                                # raises LinAlgError on a failed pivot
    r = _sinc(om * (t[None, :] - tau[:, None]))
    z = np.linalg.solve(C, r)
    return np.linalg.solve(C.T, z)


def offres_ls_error(times, segments: int, omega_max: float, omega=None, coef=None) -> float:
    """The worst model error max |exp(-i omega t) - sum_l b_l(t) exp(-i omega tau_l)| over the given times and over a frequency grid of
    max(16 L + 1, 257) equispaced points across |omega| <= omega_max - or over the values of the field map `omega` (rad/s) when given.  The
    coefficients are `coef` [L, M] (the device's own, say) or float32(offres_ls_coeffs): what the library multiplies with."""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    L = int(segments)
    b = np.asarray(offres_ls_coeffs(t, L, omega_max) if coef is None else coef).astype(np.float32).astype(np.float64).reshape(L, t.size)
    tau = offres_ls_centres(t, L)
    if omega is None:
        om = np.linspace(-abs(float(omega_max)), abs(float(omega_max)), max(16 * L + 1, 257))
    else:
        om = np.unique(np.asarray(torch.as_tensor(omega).detach().cpu().numpy(), dtype=np.float64).reshape(-1))
    worst = 0.0
    for k0 in range(0, om.size, 512):                        # [K, M] blocks: a 256 x 256 map has 65536 values
        o = om[k0:k0 + 512]
        fit = np.exp(-1j * o[:, None, None] * tau[None, :, None]) * b[None]
        worst = max(worst, float(np.abs(np.exp(-1j * o[:, None] * t[None, :]) - fit.sum(axis=1)).max()))
    return worst


def offres_ls_segments(omega_max: float, span: float, tol: float = 1e-3) -> int:
    """`offres_segments` for the least-squares interpolator: the smallest L whose `offres_ls_error` on 257 equispaced times across the span
    is <= tol; 1 where there is nothing to correct.  A result above OFFRES_MAX_SEGMENTS is reported as it is (OFFRES_MAX_SEGMENTS + 1: "more
    than the library takes" - the plan's float64 Cholesky factor is not established beyond)."""
    omega_max, span = abs(float(omega_max)), float(span)
    if not (math.isfinite(omega_max) and math.isfinite(span) and span >= 0.0 and 0.0 < tol < 1.0):
        raise ValueError(f"offres_ls_segments: need finite omega_max, span >= 0 and 0 < tol < 1, got {omega_max}, {span}, {tol}")
    if omega_max * span == 0.0:
        return 1
    t = np.linspace(0.0, span, 257)
    for L in range(2, OFFRES_MAX_SEGMENTS + 1):
        if L < omega_max * span / math.pi:                   # fewer centres than the band's Nyquist count: no fit to try
            continue
        try:
            if offres_ls_error(t, L, omega_max) <= tol:
                return L
        except np.linalg.LinAlgError:
            continue
    return OFFRES_MAX_SEGMENTS + 1


def pipe_dcf(engine_or_env, traj, iters: int = 30, width: int = 6, grid=None) -> torch.Tensor:
    """float32 [M] on the engine's device: density weights of ANY trajectory by Pipe and Menon's iteration w <- w / (Psi w) on the
    engine's own gridding kernel (pnp_nufft_dcf, include/pnpadmm_dcf.h), `iters` iterations from ones, scaled to sum h w as `radial_dcf`.
    Plans the trajectory first (width, grid as `PnPEngine.nufft_plan`) unless the live plan is this one.  engine_or_env: a PnPEngine, or
    a PnPEnv that holds one (the handle of its latest reset or `simulate`)."""
    eng = engine_or_env if hasattr(engine_or_env, "nufft_dcf") else getattr(engine_or_env, "_engine", None)
    if eng is None or not hasattr(eng, "nufft_dcf"):
        raise TypeError(f"pipe_dcf: expected a PnPEngine, or a PnPEnv that holds one, got {type(engine_or_env).__name__}")
    t = np.ascontiguousarray(traj.detach().cpu().numpy() if isinstance(traj, torch.Tensor) else traj, dtype=np.float64)
    if not eng.nufft_planned(t, grid, width):
        eng.nufft_plan(t, grid=grid, width=width)
    return eng.nufft_dcf(iters=iters)


FIELD_MAP_STREAM = 9601      # hash streams of the field map scan's noise: 9601 + 8 c + 4 e (+ 0, 1 real; + 2, 3 imaginary), coil c, echo e


def field_map_dte(omega_max: float, margin: float = 0.8) -> float:
    """The largest echo spacing dte (seconds) with omega_max * dte <= margin * pi: the two-echo field map estimate has no phase
    unwrapping, so it is valid only while |omega| dte < pi (include/pnpadmm_fieldmap.h); omega_max in rad/s, 0 < margin < 1."""
    omega_max, margin = abs(float(omega_max)), float(margin)
    if not (math.isfinite(omega_max) and omega_max > 0.0 and 0.0 < margin < 1.0):
        raise ValueError(f"field_map_dte: need finite omega_max > 0 and 0 < margin < 1, got {omega_max}, {margin}")
    return margin * math.pi / omega_max


def field_map_scan(gt, omega, te: float, dte: float, sigma_n: float, seed: int, sens=None) -> Tuple[np.ndarray, np.ndarray]:
    """The two echo images of a field map scan, complex64 [N,C,H,W] on the host (C = 1 without sens):
        x_e = S_c gt exp(-i omega te_e) + sigma_n (g_re + i g_im),   te_1 = te, te_2 = te + dte
    with the sign of include/pnpadmm_offres.h and readouts short enough that the blur is neglected.  gt [N,H,W] or [N,1,H,W]; omega rad/s
    [H,W] or [N,H,W]; sens complex [C,H,W] or None.  Slice i draws its noise from the `synthetic` counter hash at seed + i on the streams
    FIELD_MAP_STREAM + 8 c + 4 e, so a slice's scan does not depend on the batch it is in."""
    g = torch.as_tensor(gt).detach().cpu().numpy().astype(np.float64)
    if g.ndim == 4 and g.shape[1] == 1:
        g = g[:, 0]
    if g.ndim != 3:
        raise ValueError(f"field_map_scan: gt must be [N,H,W] or [N,1,H,W], got {g.shape}")
    n, h, w = g.shape
    om = torch.as_tensor(omega).detach().cpu().numpy().astype(np.float64)
    if om.shape not in ((h, w), (n, h, w)):
        raise ValueError(f"field_map_scan: omega must be [{h},{w}] or [{n},{h},{w}], got {om.shape}")
    om = np.broadcast_to(om, (n, h, w))
    te, dte, sigma_n = float(te), float(dte), float(sigma_n)
    if not (math.isfinite(te) and te >= 0.0 and math.isfinite(dte) and dte > 0.0 and math.isfinite(sigma_n) and sigma_n >= 0.0):
        raise ValueError(f"field_map_scan: need te >= 0, dte > 0 and sigma_n >= 0, all finite, got {te}, {dte}, {sigma_n}")
    s = np.ones((1, h, w), dtype=np.complex128) if sens is None else torch.as_tensor(sens).detach().cpu().numpy().astype(np.complex128)
    if s.ndim != 3 or s.shape[1:] != (h, w) or not 1 <= s.shape[0] <= _lib.PNP_MC_MAX_COILS:
        raise ValueError(f"field_map_scan: sens must be [C,{h},{w}] with C = 1..{_lib.PNP_MC_MAX_COILS}, got {s.shape}")
    out = []
    for e, t in enumerate((te, te + dte)):
        x = np.empty((n, s.shape[0], h, w), dtype=np.complex64)
        for i in range(n):
            for c in range(s.shape[0]):
                st = FIELD_MAP_STREAM + 8 * c + 4 * e
                noise = (synthetic._gauss(int(seed) + i, st, h * w) + 1j * synthetic._gauss(int(seed) + i, st + 2, h * w)).reshape(h, w)
                x[i, c] = s[c] * g[i] * np.exp(-1j * om[i] * t) + sigma_n * noise
        out.append(x)
    return out[0], out[1]


def estimate_field_map(engine_or_env, x1, x2, dte: float, beta: float = 0.05, iters: int = 200) -> torch.Tensor:
    """float32 [N,H,W] rad/s on the engine's device: the field map of the echo images x1, x2 (complex64 [N,C,H,W], `field_map_scan`'s or a
    scanner's) by the regularised two-echo fit on the device (pnp_fieldmap_estimate, include/pnpadmm_fieldmap.h).  No phase unwrapping: valid
    for |omega| dte < pi (`field_map_dte`).  engine_or_env: a PnPEngine, or a PnPEnv that holds one (the handle of its latest reset or
    `simulate`)."""
    eng = engine_or_env if hasattr(engine_or_env, "fieldmap_estimate") else getattr(engine_or_env, "_engine", None)
    if eng is None or not hasattr(eng, "fieldmap_estimate"):
        raise TypeError(f"estimate_field_map: expected a PnPEngine, or a PnPEnv that holds one, got {type(engine_or_env).__name__}")
    a = torch.as_tensor(x1).to(eng.device, torch.complex64).contiguous()
    b = torch.as_tensor(x2).to(eng.device, torch.complex64).contiguous()
    return eng.fieldmap_estimate(a, b, float(dte), beta=float(beta), iters=int(iters))


def _simulate_nc(eng, g: torch.Tensor, traj, dcf, sigma_n: float, seed: int, width: int, grid, sens=None, omega=None, times=None,
                 segments=None, interpolator: str = "linear", omega_max=None) -> Dict[str, torch.Tensor]:
    t = np.ascontiguousarray(traj.detach().cpu().numpy() if isinstance(traj, torch.Tensor) else traj, dtype=np.float64)
    eng.nufft_plan(t, grid=grid, width=width)
    d = None if dcf is None else torch.as_tensor(dcf).to(eng.device, torch.float32).contiguous()
    om = None
    if omega is not None:                                    # under a field map: the time-segmented acquisition, y [N,1,M]
        tm = np.ascontiguousarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        om = torch.as_tensor(omega).to(eng.device, torch.float32).contiguous()
        L = segments
        ls = interpolator == "ls"
        if ls:                                               # the band of the least-squares fit: given, or the map's own
            top = float(om.abs().max())
            if omega_max is None:
                omega_max = top * (1.0 + 1e-6)
            elif top > float(omega_max):
                raise ValueError(f"simulate: the field map reaches {top:g} rad/s, outside the band omega_max = {float(omega_max):g}")
        if L is None or L == "auto":
            om_max, span = float(omega_max) if ls else float(om.abs().max()), float(tm.max() - tm.min())
            L = offres_ls_segments(om_max, span) if ls else offres_segments(om_max, span)
            if L > OFFRES_MAX_SEGMENTS:                      # the library's most: a larger model error, said aloud
                import warnings
                err = offres_ls_error(tm, OFFRES_MAX_SEGMENTS, om_max) if ls else offres_bound(om_max, span, OFFRES_MAX_SEGMENTS)
                warnings.warn(f"simulate: tol = 1e-3 needs {'more than ' if ls else ''}{L - 1 if ls else L} time segments for omega_max span = "
                              f"{om_max * span:.3g} rad; using {OFFRES_MAX_SEGMENTS} (model error {err:.2e} ||p||_1)")
                L = OFFRES_MAX_SEGMENTS
        if ls and int(L) > 1:
            eng.offres_plan_ls(tm, int(L), float(omega_max))
        elif ls:
            eng.offres_plan_ls(tm, 1, 0.0)
        else:
            eng.offres_plan(tm, int(L))
        if sens is not None:                                   # coils times segments (include/pnpadmm_offres_mc.h): y [N,C,M]
            sens = torch.as_tensor(sens).to(eng.device, torch.complex64).contiguous()
            y, aty0, x0 = eng.acquire_offres_mc(g, sens, om, float(sigma_n), seed, dcf=d)
        else:
            y, aty0, x0 = eng.acquire_offres(g, om, float(sigma_n), seed, dcf=d)
            y = y.reshape(eng.n, 1, -1)
    elif sens is not None:                                     # non-Cartesian SENSE: y [N,C,M]
        sens = torch.as_tensor(sens).to(eng.device, torch.complex64).contiguous()
        y, aty0, x0 = eng.acquire_ncsense(g, sens, float(sigma_n), seed, dcf=d)
    else:
        y, aty0, x0 = eng.acquire_nc(g, float(sigma_n), seed, dcf=d)
        y = y.reshape(eng.n, 1, -1)
    out = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(y), "ATy0": torch.view_as_real(aty0), "gt": g,
           "x0_raw": aty0.real.contiguous(), "traj": torch.from_numpy(t)}
    if d is not None:
        out["dcf"] = d
    if sens is not None:
        out["sens"] = sens
    if om is not None:
        out["omega"], out["times"], out["segments"] = om, torch.from_numpy(tm), int(L)
        if interpolator == "ls":                             # (a linear acquisition's dict is the one it always was)
            out["b0_interp"] = _lib.OFFRES_INTERPOLATORS["ls"]
    return out


def simulate(engine_or_env, gt, mask, sigma_n: float, seed: int, first_slice: int = 0, sens=None, noise_cov=None, traj=None, dcf=None,
             nufft_width: int = 6, nufft_grid=None, omega=None, times=None, segments="auto", interpolator: str = "linear",
             omega_max=None, offres_mc: bool = False) -> Dict[str, torch.Tensor]:
    """The collated `.mat` dict `PnPEnv.reset` reads, acquired on the device: x0, y0, ATy0 float32 [N,1,H,W,2] (real views of the
    complex outputs), mask bool [H,W] (or [N,H,W]), gt float32 [N,1,H,W], x0_raw = Re ATy0 [N,1,H,W]; every tensor on the GPU.
    gt: [N,H,W] or [N,1,H,W] in [0, 1] (array or tensor), mask: [H,W] or [N,H,W] in the centred layout.  Slice i draws the noise of
    seed + first_slice + i, so shards of one job agree with the unsharded job (as in `synthetic.make_problem`).
    sens: coil sensitivity maps, complex [C,H,W] (shared) or [N,C,H,W] - the multi-coil acquisition (pnp_acquire_mc): y0 is then
    [N,C,H,W,2], ATy0 = sum_c conj(S_c) ifft_c(y_c), and the dict carries `sens` (complex64, on the GPU) for `PnPEnv.reset`.
    noise_cov (with sens): the channel noise covariance Psi, complex [C,C] Hermitian positive definite (e.g. `synthetic.noise_cov_model`):
    y_c = mask * (fft_c(S_c gt) + sigma_n * sum_k L[c][k] noise_k), Psi = L L^H - the noise-free acquisition plus the masked white noise
    of the plain call mixed by L on the device (pnp_whiten_apply, in place; an unsampled bin stays exactly zero).  ATy0 is the sum of
    the two parts' A^H (the noise part through the maps mixed by L^H), x0 its clip at 0; the dict carries `noise_cov` (complex128).
    traj (float64 [M,2], e.g. `radial_trajectory`; mask is then ignored and may be None): the non-Cartesian acquisition (pnp_nufft_plan +
    pnp_acquire_nc): y0 is [N,1,M,2], ATy0 = A^H (dcf y) with dcf float32 [M] or None, and the dict carries `traj` and `dcf`
    (when given) in place of `mask`.  traj with sens: the non-Cartesian SENSE acquisition (pnp_acquire_ncsense): y0 is [N,C,M,2],
    ATy0 = sum_c conj(S_c) F_nu^H (dcf y_c), and the dict carries `sens` too; traj with noise_cov is refused.
    traj with omega (field map in rad/s, float32 [H,W] or [N,H,W]) and times (seconds, [M], e.g. `readout_times`): the acquisition under
    main-field inhomogeneity by the time-segmented operator (pnp_offres_plan + pnp_acquire_offres, include/pnpadmm_offres.h) with
    `segments` segments ("auto": `offres_segments` of max |omega| and the span of the times); single-coil only.  The dict carries `omega`,
    `times` and `segments` beside `traj`.  interpolator "ls": the least-squares temporal interpolator (pnp_offres_plan_ls,
    include/pnpadmm_offres_ls.h) over |omega| <= omega_max (None: the map's max |omega| (1 + 1e-6); a map beyond a given omega_max is
    refused), "auto" segments by `offres_ls_segments`; the dict then carries `b0_interp` = 2 (pnp_offres_interpolator's code: a dict of
    numbers stays one).  offres_mc=True lifts "single-coil only": traj with omega, times AND sens is the multi-coil acquisition under the
    field map (pnp_acquire_offres_mc, include/pnpadmm_offres_mc.h), y0 [N,C,M,2], the dict carries `sens` beside `omega`, `times` and
    `segments`, and `PnPEnv(offres_mc=True).reset` installs the coils x segments stage.  The default False keeps the refusal."""
    if interpolator not in _lib.OFFRES_INTERPOLATORS:
        raise ValueError(f"simulate: interpolator must be one of {sorted(_lib.OFFRES_INTERPOLATORS)}, got {interpolator!r}")
    if (interpolator != "linear" or omega_max is not None) and omega is None:
        raise ValueError("simulate: interpolator and omega_max go with omega")
    if omega_max is not None and interpolator != "ls":
        raise ValueError("simulate: omega_max goes with interpolator='ls'")
    if not torch.cuda.is_available():
        raise RuntimeError("simulate needs a ROCm GPU; the CPU route is synthetic.make_problem")
    g = torch.as_tensor(gt)
    if g.dim() not in (3, 4) or (g.dim() == 4 and g.shape[1] != 1):
        raise ValueError(f"gt: expected [N,H,W] or [N,1,H,W], got {tuple(g.shape)}")
    h, w = int(g.shape[-2]), int(g.shape[-1])
    n = g.numel() // (h * w)
    eng = engine_or_env if hasattr(engine_or_env, "acquire") else None
    device = eng.device if eng is not None else torch.device("cuda", torch.cuda.current_device())
    eng = _engine(engine_or_env, n, h, w, device)
    if (eng.n, eng.h, eng.w) != (n, h, w):
        raise ValueError(f"gt {tuple(g.shape)} does not fit the engine [{eng.n},{eng.h},{eng.w}]")
    g = g.to(eng.device, torch.float32).reshape(n, 1, h, w).contiguous()
    if traj is not None:
        if noise_cov is not None:
            raise ValueError("simulate: a non-Cartesian acquisition draws white noise (traj with noise_cov is not supported)")
        if (omega is None) != (times is None):
            raise ValueError("simulate: omega and times go together")
        if omega is not None and sens is not None and not offres_mc:
            raise ValueError("simulate: the off-resonance acquisition is single-coil (omega with sens is not supported)")
        return _simulate_nc(eng, g, traj, dcf, sigma_n, int(seed) + int(first_slice), nufft_width, nufft_grid, sens=sens, omega=omega,
                            times=times, segments=segments, interpolator=interpolator, omega_max=omega_max)
    if omega is not None or times is not None:
        raise ValueError("simulate: omega and times need traj (a non-Cartesian acquisition)")
    m = torch.as_tensor(mask)
    if m.numel() == h * w:
        m = m.reshape(h, w)
    elif m.numel() == n * h * w:
        m = m.reshape(n, h, w)
    else:
        raise ValueError(f"mask: expected [{h},{w}] or [{n},{h},{w}], got {tuple(m.shape)}")
    m = (m != 0).to(eng.device).contiguous()
    if sens is not None:
        sens = torch.as_tensor(sens).to(eng.device, torch.complex64).contiguous()
    if noise_cov is not None:
        if sens is None:
            raise ValueError("simulate: noise_cov needs sens (a multi-coil acquisition)")
        c = int(sens.shape[-3])
        _, lmat = _factor(eng, noise_cov, c)
        y0, aty0, _ = eng.acquire(g, m, 0.0, int(seed) + int(first_slice), sens=sens)
        sn = (sens[None].expand(n, c, h, w) if sens.dim() == 3 else sens).contiguous()
        mixed = eng.coil_compress_apply(sn, lmat.conj().transpose(0, 1).resolve_conj().contiguous(), c)      # A^H (L n) = sum_k conj((L^H S)_k) ifft_c(n_k)
        yn, atn, _ = eng.acquire(torch.zeros_like(g), m, float(sigma_n), int(seed) + int(first_slice), sens=mixed)
        eng.whiten_apply(yn, lmat, out=yn)
        y0 = y0 + yn
        aty0 = aty0 + atn
        x0 = torch.view_as_complex(torch.view_as_real(aty0).clamp_min(0.0))
    else:
        y0, aty0, x0 = eng.acquire(g, m, float(sigma_n), int(seed) + int(first_slice), sens=sens)
    out = {"x0": torch.view_as_real(x0), "y0": torch.view_as_real(y0), "ATy0": torch.view_as_real(aty0), "mask": m, "gt": g,
           "x0_raw": aty0.real.contiguous()}
    if sens is not None:
        out["sens"] = sens
    if noise_cov is not None:
        out["noise_cov"] = torch.as_tensor(noise_cov).to(eng.device, torch.complex128)
    return out


def _centred_run(ok: np.ndarray) -> int:
    """Largest even a with ok[L/2 - a/2 : L/2 + a/2] all true (ok: bool [L], L even)."""
    half = len(ok) // 2
    a = 0
    while a < half and ok[half + a] and ok[half - 1 - a]:
        a += 1
    return 2 * a


def acs_block(mask) -> Tuple[int, int]:
    """(acs_h, acs_w): the largest centred rectangle with even sides that `mask` (bool [H,W], or [N,H,W]: the intersection over the
    slices) samples completely - bins -acs_h/2 <= ky - H/2 < acs_h/2, -acs_w/2 <= kx - W/2 < acs_w/2 of the centred layout, the
    calibration block `estimate_sens` reads.  A mask of whole columns gives (H, its centred run of columns), one of whole rows
    (its centred run of rows, W); any other (radial) the centred square widened until a bin is missing.  ValueError when not even
    the centre 2 x 2 bins are sampled."""
    m = np.asarray(mask) != 0
    if m.ndim == 3:
        m = m.all(axis=0)
    if m.ndim != 2 or m.shape[0] % 2 or m.shape[1] % 2:
        raise ValueError(f"acs_block: expected a mask [H,W] or [N,H,W] with even H, W, got {tuple(np.asarray(mask).shape)}")
    h, w = m.shape
    a = _centred_run(m.all(axis=0))                          # whole columns
    if a >= 2:
        return h, a
    a = _centred_run(m.all(axis=1))                          # whole rows
    if a >= 2:
        return a, w
    a = 0
    while 2 * (a + 1) <= min(h, w) and m[h // 2 - a - 1:h // 2 + a + 1, w // 2 - a - 1:w // 2 + a + 1].all():
        a += 1
    if a == 0:
        raise ValueError("acs_block: the mask does not sample the centre 2 x 2 bins of k-space: no calibration block")
    return 2 * a, 2 * a


SENS_METHODS = ("lowres", "espirit")


def estimate_sens(engine_or_env, y0, mask=None, acs=None, window: str = "hann", thresh: float = 0.05, method: str = "lowres", ksize: int = 6,
                  sv_thresh: float = 0.02, crop: float = 0.9, iters: int = 16, cal: Tuple[int, int] = (24, 24)) -> torch.Tensor:
    """Coil sensitivity maps estimated on the device from the calibration block of multi-coil k-space (pnp_estimate_sens): complex64
    [N,C,H,W] on the GPU, ready for `data['sens']` / `PnPEngine.reset(..., sens=)`.  y0: [N,C,H,W] complex, or [N,C,H,W,2] real
    (array or tensor), centred layout.  acs = (acs_h, acs_w), or None for `acs_block(mask)`: the largest centred block the mask
    samples completely.  method "lowres" (the default) is the low-resolution estimate (window, transform back, divide by the
    root-sum-of-squares over the coils).  method "espirit" is ESPIRiT (pnp_espirit_sens, at most 16 coils) with ksize x ksize kernels,
    sv_thresh, crop and iters as `PnPEngine.espirit_sens`; each side of the block is first cropped to at most `cal` (a whole-column
    block of H rows would only cost time).  A block with fewer (acs_h - ksize + 1)(acs_w - ksize + 1) windows than C ksize^2 calibrates
    badly: at 128 x 128 with 8 coils, 6 x 6 kernels and a 24 x 10 block (95 windows for 288 columns) the eigenvalue inside the object
    drops to 0.80 - take a smaller ksize for a narrow block."""
    if method not in SENS_METHODS:
        raise ValueError(f"method must be one of {SENS_METHODS}, got {method!r}")
    if not torch.cuda.is_available():
        raise RuntimeError("estimate_sens needs a ROCm GPU")
    y = torch.as_tensor(y0)
    if not y.is_complex():
        if y.dim() != 5 or y.shape[-1] != 2:
            raise ValueError(f"y0: expected complex [N,C,H,W] or real [N,C,H,W,2], got {tuple(y.shape)}")
        y = torch.view_as_complex(y.float().contiguous())
    if y.dim() != 4:
        raise ValueError(f"y0: expected [N,C,H,W], got {tuple(y.shape)}")
    n, _, h, w = (int(v) for v in y.shape)
    if acs is None:
        if mask is None:
            raise ValueError("estimate_sens: give acs=(acs_h, acs_w) or the sampling mask")
        acs = acs_block(torch.as_tensor(mask).cpu().numpy())
    eng = engine_or_env if hasattr(engine_or_env, "estimate_sens") else None
    device = eng.device if eng is not None else torch.device("cuda", torch.cuda.current_device())
    if eng is None:
        eng = _engine(engine_or_env, n, h, w, device)
    if (eng.n, eng.h, eng.w) != (n, h, w):
        raise ValueError(f"y0 {tuple(y.shape)} does not fit the engine [{eng.n},{eng.h},{eng.w}]")
    y = y.to(eng.device, torch.complex64).contiguous()
    if method == "lowres":
        return eng.estimate_sens(y, acs, window=window, thresh=thresh)
    acs = tuple(min(int(a), int(c) & ~1) for a, c in zip(acs, cal))
    return eng.espirit_sens(y, acs, ksize=ksize, sv_thresh=sv_thresh, crop=crop, iters=iters, window=window, thresh=thresh)


def coils_for_energy(eig, energy: float) -> int:
    """The virtual coils a batch keeps for an energy target: per slice the smallest V whose leading eigenvalues (eig [N,C], descending)
    reach `energy` of their sum, and the largest of those over the slices.  A slice without energy counts 1."""
    e = np.asarray(eig, dtype=np.float64)
    if e.ndim != 2 or e.shape[1] < 1:
        raise ValueError(f"eig: expected [N,C], got {e.shape}")
    if not 0.0 < energy <= 1.0:
        raise ValueError(f"energy must be in (0, 1], got {energy}")
    total = e.sum(axis=1)
    reached = np.cumsum(e, axis=1) >= energy * total[:, None]
    v = np.where(reached.any(axis=1), reached.argmax(axis=1) + 1, e.shape[1])
    return int(np.where(total > 0, v, 1).max())


def compress_coils(engine_or_env, y0, mask=None, acs=None, out_coils=None, energy=None, sens=None) -> Dict[str, torch.Tensor]:
    """Coil compression on the device (pnp_coil_compress_matrix, pnp_coil_compress_apply): the C channels of y0 mixed down to V virtual
    coils by the leading eigenvectors of the calibration block's channel covariance, per slice.  y0: [N,C,H,W] complex, or [N,C,H,W,2]
    real (array or tensor), centred layout, C <= 64.  acs = (acs_h, acs_w), or None for `acs_block(mask)`.  Exactly one of out_coils (V
    itself, 1..min(C, 32)) and energy (in (0, 1]: `coils_for_energy` of the eigenvalues - each slice's smallest V that reaches this
    share of the trace, the batch takes the largest; this costs ONE host read of the [N,C] eigenvalues at setup) must be given.  sens:
    the coil maps, complex [C,H,W] (shared: broadcast to the batch first, since every slice has its own matrix) or [N,C,H,W], mixed by
    the same matrices.  Returns a dict: y0 complex64 [N,V,H,W], cmat complex64 [N,C,C], eig float32 [N,C], out_coils, and sens
    complex64 [N,V,H,W] when maps were given; every tensor on the GPU."""
    if (out_coils is None) == (energy is None):
        raise ValueError("compress_coils: give exactly one of out_coils and energy")
    if energy is not None and not 0.0 < energy <= 1.0:
        raise ValueError(f"compress_coils: energy must be in (0, 1], got {energy}")
    y = torch.as_tensor(y0)
    if not y.is_complex():
        if y.dim() != 5 or y.shape[-1] != 2:
            raise ValueError(f"y0: expected complex [N,C,H,W] or real [N,C,H,W,2], got {tuple(y.shape)}")
        y = torch.view_as_complex(y.float().contiguous())
    if y.dim() != 4:
        raise ValueError(f"y0: expected [N,C,H,W], got {tuple(y.shape)}")
    n, c, h, w = (int(v) for v in y.shape)
    if out_coils is not None and not 1 <= int(out_coils) <= min(c, 32):
        raise ValueError(f"compress_coils: out_coils must be 1..{min(c, 32)}, got {out_coils}")
    if acs is None:
        if mask is None:
            raise ValueError("compress_coils: give acs=(acs_h, acs_w) or the sampling mask")
        acs = acs_block(torch.as_tensor(mask).cpu().numpy())
    s = None
    if sens is not None:
        s = torch.as_tensor(sens)
        if not s.is_complex() or s.dim() not in (3, 4) or tuple(s.shape[-3:]) != (c, h, w) or (s.dim() == 4 and s.shape[0] != n):
            raise ValueError(f"sens: expected complex [{c},{h},{w}] or [{n},{c},{h},{w}], got {tuple(s.shape)}")
    if not torch.cuda.is_available():
        raise RuntimeError("compress_coils needs a ROCm GPU")
    eng = engine_or_env if hasattr(engine_or_env, "coil_compress_matrix") else None
    device = eng.device if eng is not None else torch.device("cuda", torch.cuda.current_device())
    if eng is None:
        eng = _engine(engine_or_env, n, h, w, device)
    if (eng.n, eng.h, eng.w) != (n, h, w):
        raise ValueError(f"y0 {tuple(y.shape)} does not fit the engine [{eng.n},{eng.h},{eng.w}]")
    y = y.to(eng.device, torch.complex64).contiguous()
    cmat, eig = eng.coil_compress_matrix(y, acs)
    v = int(out_coils) if out_coils is not None else min(coils_for_energy(eig.cpu().numpy(), energy), 32)
    out = {"y0": eng.coil_compress_apply(y, cmat, v), "cmat": cmat, "eig": eig, "out_coils": v}
    if s is not None:
        s = s.to(eng.device, torch.complex64)
        s = (s[None].expand(n, c, h, w) if s.dim() == 3 else s).contiguous()
        out["sens"] = eng.coil_compress_apply(s, cmat, v)
    return out


def _centre_block(w: int, center_fraction: float) -> np.ndarray:
    nc = int(round(w * center_fraction))
    lo = (w - nc) // 2
    centre = np.zeros(w, dtype=bool)
    centre[lo:lo + nc] = True
    return centre


def cartesian_mask(h: int, w: int, accel: float, center_fraction: float = 0.08, seed: int = 0, kind: str = "random") -> np.ndarray:
    """Bool [h,w] of whole columns (constant along H), centred layout.  A centred block of round(w * center_fraction) columns is
    always sampled.  "random": exactly ceil(w / accel) columns; the outer ones are those with the smallest keys of
    hash_uniform(seed, 9101, w) (ties by column index).  "equispaced": a comb of K columns floor((2 j + 1) w / (2 K)) over the whole
    width, laid under the centre block, with the smallest K whose sampled fraction reaches 1 / accel; neighbouring teeth are floor or
    ceil of w / K apart, so the gaps between consecutive outer columns on one side of the centre block differ by at most 1."""
    if kind not in ("random", "equispaced"):
        raise ValueError(f"kind must be 'random' or 'equispaced', got {kind!r}")
    if not accel >= 1.0:
        raise ValueError(f"accel must be >= 1, got {accel}")
    centre = _centre_block(w, center_fraction)
    target = int(math.ceil(w / accel))
    cols = centre.copy()
    if kind == "random":
        outer = np.flatnonzero(~centre)
        k = min(max(target - int(centre.sum()), 0), len(outer))
        keys = hash_uniform(seed, 9101, w).astype(np.float64)[outer]
        cols[outer[np.argsort(keys, kind="stable")[:k]]] = True
    else:
        for k in range(0, w + 1):
            cols = centre.copy()
            if k:
                cols[((2 * np.arange(k) + 1) * w) // (2 * k)] = True
            if cols.sum() >= target:
                break
    return np.broadcast_to(cols[None, :], (h, w)).copy()


def uniform_mask(h: int, w: int, accel: int, offset: int = None, center_fraction: float = 0.08) -> np.ndarray:
    """Bool [h,w] of whole columns, centred layout: the integer comb offset + k accel (offset: accel // 2 by default) laid under the
    centred block of round(w * center_fraction) columns of `cartesian_mask` (at least the two centre columns, so that there always is a
    calibration block) - the sampling GRAPPA works on (`grappa_geometry` reads it back).  ValueError unless accel is a whole number that
    divides w."""
    if accel != int(accel) or int(accel) < 1 or w % int(accel):
        raise ValueError(f"uniform_mask: accel must be a whole number that divides w={w}, got {accel}")
    accel = int(accel)
    offset = accel // 2 if offset is None else int(offset)
    if not 0 <= offset < accel:
        raise ValueError(f"uniform_mask: offset must be 0..{accel - 1}, got {offset}")
    cols = _centre_block(w, max(center_fraction, 2.0 / w))
    cols[offset::accel] = True
    return np.broadcast_to(cols[None, :], (h, w)).copy()


def _comb_of(cols: np.ndarray) -> Tuple[int, int, int]:
    """(accel, offset, acs_w) of one row of a whole-column mask (bool [W], W even), or ValueError"""
    w = len(cols)
    acs_w = _centred_run(cols)
    if acs_w < 2:
        raise ValueError("the mask does not sample the centre columns of k-space: no calibration block")
    lo, hi = w // 2, w // 2                                  # the whole run of sampled columns around the centre
    while lo > 0 and cols[lo - 1]:
        lo -= 1
    while hi < w and cols[hi]:
        hi += 1
    outer = cols.copy()
    outer[lo:hi] = False
    teeth = np.flatnonzero(outer)
    if len(teeth) == 0:
        raise ValueError("the mask has no comb of columns outside its centre block")
    for accel in range(2, w // 2 + 1):
        if w % accel:
            continue
        comb = np.zeros(w, dtype=bool)
        comb[int(teeth[0]) % accel::accel] = True
        comb[lo:hi] = False
        if np.array_equal(comb, outer):
            return accel, int(teeth[0]) % accel, acs_w
    raise ValueError("the columns outside the centre block are not one integer comb x = offset (mod accel) with accel dividing the width")


def grappa_geometry(mask) -> Tuple[int, int, int, int]:
    """(accel, offset, acs_h, acs_w) of a mask GRAPPA can work on: whole columns (bool [H,W]; or [N,H,W], every slice on the same comb -
    acs_w is then the narrowest centre), the integer comb x = offset (mod accel) with accel dividing W, plus a fully sampled centre
    (acs_h = H, acs_w = its largest centred even run, as `acs_block`).  ValueError for every other mask: radial, random columns, an
    `equispaced` comb whose spacing is not a whole number, a comb without a centre."""
    m = np.asarray(torch.as_tensor(mask).cpu()) != 0
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1] % 2 or m.shape[2] % 2:
        raise ValueError(f"grappa_geometry: expected a mask [H,W] or [N,H,W] with even H, W, got {tuple(np.asarray(mask).shape)}")
    if not (m == m[:, :1, :]).all():
        raise ValueError("grappa_geometry: the mask is not made of whole columns")
    found = []
    for cols in m[:, 0, :]:
        try:
            found.append(_comb_of(cols))
        except ValueError as e:
            raise ValueError(f"grappa_geometry: {e}") from None
    if any(f[:2] != found[0][:2] for f in found):
        raise ValueError("grappa_geometry: the slices' masks are not on one comb")
    return found[0][0], found[0][1], int(m.shape[1]), min(f[2] for f in found)


def coil_images(eng, kspace: torch.Tensor) -> torch.Tensor:
    """ifft_c of every coil of kspace complex64 [N,C,H,W] with the engine's transform, coil by coil (the engine transforms N planes per
    call): setup-time plumbing."""
    return torch.stack([eng.fft2c(kspace[:, c].contiguous(), inverse=True) for c in range(kspace.shape[1])], dim=1)


def grappa(engine_or_env, y0, mask, kernel: Tuple[int, int] = (5, 4), lam: float = 1e-2, sens=None) -> Dict[str, torch.Tensor]:
    """GRAPPA on the device (pnp_grappa_weights, pnp_grappa_apply): the missing columns of multi-coil k-space synthesised from their
    acquired neighbours with weights calibrated, per slice, on the fully sampled centre of its own y0.  y0: [N,C,H,W] complex, or
    [N,C,H,W,2] real (array or tensor), centred layout, C <= 32; mask: what `grappa_geometry` accepts (`uniform_mask`); kernel = (by, bx)
    rows by acquired columns; lam: the Tikhonov weight relative to the mean diagonal of the normal matrix (1e-2: a default from a scan on
    the analytic coils, not a tuned value).  Returns a dict, every tensor on the GPU: y0 complex64 [N,C,H,W] filled k-space (measured bins
    are copies), wts complex64 [N,nt,ns], info int32 [N] (non-zero: that slice's calibration failed and its missing bins stay zero; it is
    not read here), rss float32 [N,H,W] the root-sum-of-squares image of the filled k-space, and with sens (complex [C,H,W] or
    [N,C,H,W]) also x0 float32 [N,1,H,W] = max(Re sum_c conj(S_c) ifft_c(filled_c), 0), the map-combined image - an initial iterate.  The
    two images are setup-time torch arithmetic over the engine's inverse transform."""
    y = torch.as_tensor(y0)
    if not y.is_complex():
        if y.dim() != 5 or y.shape[-1] != 2:
            raise ValueError(f"y0: expected complex [N,C,H,W] or real [N,C,H,W,2], got {tuple(y.shape)}")
        y = torch.view_as_complex(y.float().contiguous())
    if y.dim() != 4:
        raise ValueError(f"y0: expected [N,C,H,W], got {tuple(y.shape)}")
    n, c, h, w = (int(v) for v in y.shape)
    m = torch.as_tensor(mask)
    if m.numel() not in (h * w, n * h * w):
        raise ValueError(f"mask: expected [{h},{w}] or [{n},{h},{w}], got {tuple(m.shape)}")
    m = m.reshape((h, w) if m.numel() == h * w else (n, h, w))
    accel, offset, acs_h, acs_w = grappa_geometry(m)
    by, bx = (int(v) for v in kernel)
    if acs_h < by or acs_w < (bx - 1) * accel + 1:
        raise ValueError(f"grappa: the {acs_h} x {acs_w} calibration block holds no {by} x {bx} kernel at acceleration {accel} "
                         f"(it spans {(bx - 1) * accel + 1} columns)")
    s = None
    if sens is not None:
        s = torch.as_tensor(sens)
        if not s.is_complex() or s.dim() not in (3, 4) or tuple(s.shape[-3:]) != (c, h, w) or (s.dim() == 4 and s.shape[0] != n):
            raise ValueError(f"sens: expected complex [{c},{h},{w}] or [{n},{c},{h},{w}], got {tuple(s.shape)}")
    if not torch.cuda.is_available():
        raise RuntimeError("grappa needs a ROCm GPU")
    eng = engine_or_env if hasattr(engine_or_env, "grappa_apply") else None
    if eng is None:
        eng = _engine(engine_or_env, n, h, w, torch.device("cuda", torch.cuda.current_device()))
    if (eng.n, eng.h, eng.w) != (n, h, w):
        raise ValueError(f"y0 {tuple(y.shape)} does not fit the engine [{eng.n},{eng.h},{eng.w}]")
    y = y.to(eng.device, torch.complex64).contiguous()
    m = (m != 0).to(eng.device).contiguous()
    wts, info = eng.grappa_weights(y, (acs_h, acs_w), accel, kernel=(by, bx), lam=lam)
    filled = eng.grappa_apply(y, wts, m, accel, offset, kernel=(by, bx))
    img = coil_images(eng, filled)
    out = {"y0": filled, "wts": wts, "info": info, "rss": (img.real ** 2 + img.imag ** 2).sum(dim=1).sqrt()}
    if s is not None:
        s = s.to(eng.device, torch.complex64)
        out["x0"] = (s.conj() * img).sum(dim=1, keepdim=True).real.clamp_min(0.0).contiguous()
    return out


def parse_task(task: str) -> Tuple[int, float]:
    """'4x_10' -> (4, 10 / 255): the task names `data.task_from_filename` produces."""
    m = re.fullmatch(r"(\d+)x_(\d+)", task)
    if m is None:
        raise ValueError(f"task {task!r} is not '<accel>x_<sigma>'")
    return int(m.group(1)), int(m.group(2)) / 255.0


def make_mask(h: int, w: int, accel: float, kind: str = "radial", seed: int = 0) -> np.ndarray:
    if kind == "radial":
        return synthetic.radial_mask(h, w, accel)
    if kind == "cartesian":
        return cartesian_mask(h, w, accel, seed=seed)
    if kind == "uniform":                                    # a centre of 3 accel + 4 columns: room for four window columns of a 4-column GRAPPA kernel
        return uniform_mask(h, w, accel, center_fraction=max(0.08, (3 * int(accel) + 4) / w))
    raise ValueError(f"mask kind must be one of {MASK_KINDS}, got {kind!r}")


def task_problem(task: str, gt, engine_or_env, seed: int = 0, first_slice: int = 0, mask_kind: str = "radial",
                 mask=None, coils: int = 0, noise_cov=None, spokes: int = None, b0_interp: str = "linear", b0_coils: int = 0,
                 nc_weights: str = "dcf",
                 b0_map: str = "true", b0_dte_ms: float = None, b0_beta: float = 0.05, b0_iters: int = 200, b0_scan_noise: float = None,
                 nufft_width: int = 6, b0_hz: float = None, readout_ms: float = None, b0_segments="auto",
                 nufft_grid=None, interleaves: int = None, petals: int = None, dcf_iters: int = 30) -> Dict[str, torch.Tensor]:
    """`simulate` for a named task: '4x_10' = acceleration 4, sigma_n = 10 / 255.  mask: a ready mask, or None for
    `make_mask(h, w, accel, mask_kind, seed)` (the same for every shard of a job).  coils > 0: a multi-coil acquisition with the
    analytic maps `synthetic.coil_maps(coils, h, w)`; noise_cov: their channel noise covariance (`simulate`).
    mask_kind "radial-nc": a true radial acquisition, samples off the grid (`simulate(traj=)`): golden-angle `radial_trajectory` of
    `spokes` spokes (None: ceil(h / accel)); "spiral-nc": `spiral_trajectory` of `interleaves` interleaves (None: ceil(h / (2 accel)),
    about the samples of the radial acquisition); "rosette-nc": `rosette_trajectory` of `petals` petals (None: an odd count near
    h / accel).  nc_weights: "none"; "pipe", the iterated density weights `pipe_dcf` (`dcf_iters` iterations); "dcf", the weights written
    for the trajectory: the ramp `radial_dcf` on "radial-nc" and `pipe_dcf` on the other two (the ramp is never applied to a trajectory
    it was not written for).  With coils > 0 the non-Cartesian SENSE acquisition with the maps `synthetic.coil_maps(coils, h, w)`.
    b0_hz (with a non-Cartesian mask_kind, single-coil): the acquisition under main-field inhomogeneity - the smooth map
    `synthetic.field_map(h, w, b0_hz, seed)` shared by the slices, every readout (spoke, interleaf, shot) `readout_ms` long
    (`readout_times`), by the time-segmented operator with `b0_segments` segments ("auto": `simulate`'s rule); the dict then carries
    `omega`, `times` and `segments`, and `PnPEnv.reset` installs the off-resonance stage.
    b0_map (with b0_hz): "true" hands the solver the map that made the data; "estimate" does what a scanner does: it simulates a two-echo
    field map scan of the task's own ground truth under the true map (`field_map_scan`: echo spacing `b0_dte_ms`, None for
    `field_map_dte(2 pi b0_hz)`; image noise `b0_scan_noise`, None for the task's sigma_n), estimates the map on the device
    (`estimate_field_map` with `b0_beta`, `b0_iters`: no phase unwrapping, so b0_hz * b0_dte_ms must stay below 500) and installs the
    estimate, float32 [N,H,W], as `omega`; the truth stays under `omega_true`.  The data y are the true map's either way.
    b0_interp (with b0_hz): "linear", or "ls" for the least-squares temporal interpolator (`simulate(interpolator=)`).
    b0_coils (with b0_hz, 1..32; not with coils): the multi-coil acquisition under the field map, with the maps
    `synthetic.coil_maps(b0_coils, h, w)` (`simulate(..., sens=, offres_mc=True)`); the dict then carries `sens` too and
    `PnPEnv(offres_mc=True).reset` installs the coils x segments stage.  The map is the true one: b0_map="estimate" is refused with b0_coils."""
    accel, sigma_n = parse_task(task)
    b0_coils = int(b0_coils)
    if b0_coils:
        if not 1 <= b0_coils <= _lib.PNP_MC_MAX_COILS:
            raise ValueError(f"task_problem: b0_coils must be 1..{_lib.PNP_MC_MAX_COILS}, got {b0_coils}")
        if b0_hz is None:
            raise ValueError("task_problem: b0_coils needs b0_hz (the multi-coil acquisition under a field map)")
        if coils:
            raise ValueError("task_problem: b0_coils is the coil count of the off-resonance acquisition; it does not go with coils")
        if b0_map == "estimate":
            raise ValueError("task_problem: b0_map='estimate' is not supported with b0_coils: estimating the field map inside a multi-coil "
                             "episode is out of scope (estimate it beforehand and pass the map)")
    if b0_interp not in _lib.OFFRES_INTERPOLATORS:
        raise ValueError(f"task_problem: b0_interp must be one of {sorted(_lib.OFFRES_INTERPOLATORS)}, got {b0_interp!r}")
    if b0_interp != "linear" and b0_hz is None:
        raise ValueError("task_problem: b0_interp needs b0_hz (a field map to correct)")
    interp = {} if b0_interp == "linear" else {"interpolator": b0_interp}      # the linear call is the call it always was
    if b0_map not in ("true", "estimate"):
        raise ValueError(f"task_problem: b0_map must be 'true' or 'estimate', got {b0_map!r}")
    if b0_map == "estimate" and b0_hz is None:
        raise ValueError("task_problem: b0_map='estimate' needs b0_hz (a field map to estimate)")
    h, w = (int(v) for v in torch.as_tensor(gt).shape[-2:])
    if mask_kind in NC_KINDS:
        if noise_cov is not None or mask is not None:
            raise ValueError(f"task_problem: mask_kind {mask_kind!r} takes no mask and no noise_cov")
        if nc_weights not in ("none", "dcf", "pipe"):
            raise ValueError(f"nc_weights must be 'none', 'dcf' or 'pipe', got {nc_weights!r}")
        if mask_kind == "radial-nc":
            traj = radial_trajectory(h, w, int(math.ceil(h / accel)) if spokes is None else int(spokes))
        elif mask_kind == "spiral-nc":
            traj = spiral_trajectory(h, w, int(math.ceil(h / (2.0 * accel))) if interleaves is None else int(interleaves))
        else:
            traj = rosette_trajectory(h, w, (int(math.ceil(h / accel)) | 1) if petals is None else int(petals))
        sens = synthetic.coil_maps(coils, h, w).astype(np.complex64) if coils else None
        if nc_weights == "none":
            dcf = None
        elif nc_weights == "dcf" and mask_kind == "radial-nc":
            dcf = radial_dcf(traj, h, w)
        else:                                                # the handle `simulate` will use plans this trajectory and iterates on it
            g = torch.as_tensor(gt)
            eng = engine_or_env if hasattr(engine_or_env, "acquire") else None
            device = eng.device if eng is not None else torch.device("cuda", torch.cuda.current_device())
            dcf = pipe_dcf(_engine(engine_or_env, g.numel() // (h * w), h, w, device), traj, iters=dcf_iters, width=nufft_width, grid=nufft_grid)
        if b0_hz is None:
            return simulate(engine_or_env, gt, None, sigma_n, seed, first_slice, sens=sens, traj=traj, dcf=dcf, nufft_width=nufft_width,
                            nufft_grid=nufft_grid)
        # under main-field inhomogeneity: one smooth field map of at most b0_hz shared by the slices, every readout readout_ms long
        if coils:
            raise ValueError("task_problem: the off-resonance acquisition is single-coil (b0_hz with coils is not supported)")
        if readout_ms is None or not (math.isfinite(readout_ms) and readout_ms > 0.0 and math.isfinite(b0_hz) and b0_hz >= 0.0):
            raise ValueError(f"task_problem: b0_hz needs b0_hz >= 0 and readout_ms > 0, got {b0_hz}, {readout_ms}")
        m = traj.shape[0]
        if mask_kind == "radial-nc":                         # samples per spoke / interleaf / shot, as the generators emit them
            readout = 2 * max(h, w)
        elif mask_kind == "spiral-nc":
            readout = m // (int(math.ceil(h / (2.0 * accel))) if interleaves is None else int(interleaves))
        else:
            readout = m
        times = readout_times(mask_kind[:-3], m, readout, float(readout_ms) * 1e-3)
        omega = (2.0 * math.pi * synthetic.field_map(h, w, float(b0_hz), seed)).astype(np.float32)
        if b0_coils:
            return simulate(engine_or_env, gt, None, sigma_n, seed, first_slice, sens=synthetic.coil_maps(b0_coils, h, w).astype(np.complex64),
                            traj=traj, dcf=dcf, nufft_width=nufft_width, nufft_grid=nufft_grid, omega=omega, times=times, segments=b0_segments,
                            offres_mc=True, **interp)
        if b0_map == "true":
            return simulate(engine_or_env, gt, None, sigma_n, seed, first_slice, traj=traj, dcf=dcf, nufft_width=nufft_width,
                            nufft_grid=nufft_grid, omega=omega, times=times, segments=b0_segments, **interp)
        dte = field_map_dte(2.0 * math.pi * max(float(b0_hz), 1.0)) if b0_dte_ms is None else float(b0_dte_ms) * 1e-3
        noise = sigma_n if b0_scan_noise is None else float(b0_scan_noise)
        if not (math.isfinite(dte) and dte > 0.0 and math.isfinite(noise) and noise >= 0.0 and math.isfinite(b0_beta) and b0_beta > 0.0
                and 0 <= int(b0_iters) <= _lib.PNP_FIELDMAP_MAX_ITERS):
            raise ValueError(f"task_problem: b0_map='estimate' needs b0_dte_ms > 0, b0_scan_noise >= 0, b0_beta > 0 and b0_iters in "
                             f"0..{_lib.PNP_FIELDMAP_MAX_ITERS}, got {b0_dte_ms}, {b0_scan_noise}, {b0_beta}, {b0_iters}")
        if 2.0 * math.pi * float(b0_hz) * dte >= math.pi:
            raise ValueError(f"task_problem: the two-echo estimate has no phase unwrapping: b0_hz * b0_dte_ms must stay below 500, got "
                             f"{b0_hz} * {dte * 1e3:g}")
        out = simulate(engine_or_env, gt, None, sigma_n, seed, first_slice, traj=traj, dcf=dcf, nufft_width=nufft_width, nufft_grid=nufft_grid,
                       omega=omega, times=times, segments=b0_segments, **interp)
        g = torch.as_tensor(gt)
        eng = engine_or_env if hasattr(engine_or_env, "acquire") else None
        device = eng.device if eng is not None else torch.device("cuda", torch.cuda.current_device())
        x1, x2 = field_map_scan(g.reshape(-1, h, w), omega, 0.0, dte, noise, int(seed) + int(first_slice))
        out["omega_true"] = torch.as_tensor(out.get("omega", omega))
        out["omega"] = estimate_field_map(_engine(engine_or_env, g.numel() // (h * w), h, w, device), x1, x2, dte, beta=b0_beta, iters=b0_iters)
        return out
    if b0_hz is not None or readout_ms is not None:
        raise ValueError("task_problem: b0_hz and readout_ms need a non-Cartesian mask_kind (radial-nc, spiral-nc, rosette-nc)")
    if mask is None:
        mask = make_mask(h, w, accel, mask_kind, seed)
    sens = synthetic.coil_maps(coils, h, w).astype(np.complex64) if coils else None
    return simulate(engine_or_env, gt, mask, sigma_n, seed, first_slice, sens=sens, noise_cov=noise_cov)
