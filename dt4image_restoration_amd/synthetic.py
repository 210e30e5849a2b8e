"""Seeded synthetic CS-MRI problems in the reference's evaluation-data layout.

The reference evaluates on `.mat` files holding `x0, y0, ATy0` (float32 [...,H,W,2],
real/imag last), `mask` [H,W] and `gt` [1,H,W] (dataset/datasets.py:153-160,191-199); the
files are an external download.  This module builds the same dict from an analytic
phantom so every box (and the golden-vector generator) sees identical inputs:

* gt      : sum of random ellipses in [0,1], per-slice parameters from (seed, slice index)
* mask    : radial lines through the k-space centre, sampled fraction >= 1/accel
* y0      : mask * (fft_c(gt) + complex Gaussian noise, sigma_n per component)
* x0=ATy0 : ifft_c(y0); x0 real part clipped at 0 like datasets.py:160,199
            (np.clip on the stacked array clips the imaginary plane too - reproduced)
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np

from .weights import hash_uniform


def fft2c_np(a: np.ndarray) -> np.ndarray:
    """Centred orthonormal 2-D DFT over the last two axes (transformations.py:6-12)."""
    return np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def ifft2c_np(a: np.ndarray) -> np.ndarray:
    """Centred orthonormal inverse 2-D DFT (transformations.py:14-19)."""
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def radial_mask(h: int, w: int, accel: float) -> np.ndarray:
    """Bool [h,w]: L lines through the centre at angles k*pi/L, nearest-pixel rasterised,
    L = smallest count whose sampled fraction is >= 1/accel."""
    cy, cx = h // 2, w // 2
    r = math.hypot(h, w) / 2.0
    t = np.arange(-r, r + 0.25, 0.25)
    target = 1.0 / accel

    def raster(nlines: int) -> np.ndarray:
        m = np.zeros((h, w), dtype=bool)
        for k in range(nlines):
            th = math.pi * k / nlines
            ys = np.rint(cy + t * math.sin(th)).astype(np.int64)
            xs = np.rint(cx + t * math.cos(th)).astype(np.int64)
            ok = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
            m[ys[ok], xs[ok]] = True
        return m

    lo, hi = 1, 4 * max(h, w)
    while lo < hi:                       # sampled fraction is monotone enough in L; bisect
        mid = (lo + hi) // 2
        if raster(mid).mean() >= target:
            hi = mid
        else:
            lo = mid + 1
    return raster(lo)


def phantom(h: int, w: int, seed: int) -> np.ndarray:
    """float64 [h,w] in [0,1]: 6-10 soft-edged ellipses."""
    u = (hash_uniform(seed, 7001, 64).astype(np.float64) + 1.0) * 0.5   # [0,1)
    n_ell = 6 + int(u[0] * 5)
    yy, xx = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing="ij")
    img = np.zeros((h, w))
    # body ellipse
    body = ((xx / 0.85) ** 2 + (yy / 0.9) ** 2)
    img += 0.35 * np.clip((1.0 - body) * 12.0, 0.0, 1.0)
    for e in range(n_ell):
        p = u[1 + 6 * e: 7 + 6 * e]
        cx, cy = (p[0] - 0.5) * 1.1, (p[1] - 0.5) * 1.1
        ax, ay = 0.08 + 0.35 * p[2], 0.08 + 0.35 * p[3]
        th = math.pi * p[4]
        amp = 0.15 + 0.5 * p[5]
        xr = (xx - cx) * math.cos(th) + (yy - cy) * math.sin(th)
        yr = -(xx - cx) * math.sin(th) + (yy - cy) * math.cos(th)
        d = (xr / ax) ** 2 + (yr / ay) ** 2
        img += amp * np.clip((1.0 - d) * 10.0, 0.0, 1.0) * np.clip((1.0 - body) * 12.0, 0.0, 1.0)
    return np.clip(img / max(img.max(), 1e-9), 0.0, 1.0)


def _gauss(seed: int, stream: int, count: int) -> np.ndarray:
    u1 = (hash_uniform(seed, stream, count).astype(np.float64) + 1.0) * 0.5
    u2 = (hash_uniform(seed, stream + 1, count).astype(np.float64) + 1.0) * 0.5
    u1 = np.maximum(u1, 2.0 ** -25)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def make_problem(n: int, h: int, w: int, accel: float = 4.0, sigma_n: float = 10.0 / 255.0,
                 seed: int = 1234, first_slice: int = 0) -> Dict[str, np.ndarray]:
    """Collated-batch dict with the `.mat` keys the reference's `PnPEnv.reset` reads
    (env.py:57-71): x0, y0, ATy0 float32 [n,1,h,w,2]; mask bool [h,w]; gt float32 [n,1,h,w]; plus x0_raw [n,1,h,w].
    Slice i depends only on (seed, first_slice + i), so shards of one job agree with the
    unsharded job."""
    mask = radial_mask(h, w, accel)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    x0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    y0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        noise = (_gauss(s, 9001, h * w) + 1j * _gauss(s, 9003, h * w)).reshape(h, w) * sigma_n
        y = mask * (fft2c_np(g) + noise)
        a = ifft2c_np(y)
        gt[i, 0] = g
        y0[i, 0, ..., 0], y0[i, 0, ..., 1] = y.real, y.imag
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
        x0[i, 0] = np.clip(aty0[i, 0], 0.0, None)           # datasets.py:160
    # x0_raw: the UNclipped real part of the zero-filled reconstruction - the policy's first state token in the reference
    # (datasets.py:162,201 read mat['x0'][..., 0], which the clip at :160,199 does not touch)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "mask": mask, "gt": gt, "x0_raw": aty0[..., 0].copy()}


def ndft_np(traj: np.ndarray, x: np.ndarray, adjoint_shape=None) -> np.ndarray:
    """The exact non-Cartesian operator of include/pnpadmm.h in float64: (A x)_m = (1 / sqrt(h w)) sum_q x[q] exp(-2 pi i (ky qy + kx qx)),
    q centred; x [..., h, w] -> [..., M].  With adjoint_shape = (h, w): A^H, x [..., M] -> [..., h, w].  O(M h w): small sizes only."""
    traj = np.asarray(traj, dtype=np.float64)
    h, w = adjoint_shape if adjoint_shape is not None else x.shape[-2:]
    sgn = 2j if adjoint_shape is not None else -2j
    ey = np.exp(sgn * math.pi * traj[:, 0:1] * (np.arange(h) - h // 2))
    ex = np.exp(sgn * math.pi * traj[:, 1:2] * (np.arange(w) - w // 2))
    x = np.asarray(x, dtype=np.complex128)
    if adjoint_shape is not None:
        return np.einsum("my,...m,mx->...yx", ey, x, ex, optimize=True) / math.sqrt(h * w)
    return np.einsum("my,...yx,mx->...m", ey, x, ex, optimize=True) / math.sqrt(h * w)


def make_problem_nc(n: int, h: int, w: int, traj: np.ndarray, dcf: np.ndarray = None, sigma_n: float = 10.0 / 255.0, seed: int = 1234,
                    first_slice: int = 0) -> Dict[str, np.ndarray]:
    """`make_problem` for a non-Cartesian trajectory, by the exact NDFT in float64 (meant for small sizes): y0 float32 [n,1,M,2] with
    y = A gt + sigma_n noise (the counter hash of `make_problem` indexed by the sample m), ATy0 = A^H (dcf y) and x0 = its clip at 0,
    float32 [n,1,h,w,2]; gt, x0_raw as in `make_problem`; traj float64 [M,2], dcf float32 [M] or None."""
    traj = np.asarray(traj, dtype=np.float64)
    m = traj.shape[0]
    d = None if dcf is None else np.asarray(dcf, dtype=np.float32)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    y0 = np.empty((n, 1, m, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        y = ndft_np(traj, g) + (_gauss(s, 9001, m) + 1j * _gauss(s, 9003, m)) * sigma_n
        a = ndft_np(traj, y if d is None else y * d.astype(np.float64), adjoint_shape=(h, w))
        gt[i, 0] = g
        y0[i, 0, :, 0], y0[i, 0, :, 1] = y.real, y.imag
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
    x0 = np.clip(aty0, 0.0, None)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "gt": gt, "x0_raw": aty0[..., 0].copy(), "traj": traj, "dcf": d}


def field_map(h: int, w: int, max_hz: float, seed: int = 0) -> np.ndarray:
    """float64 [h,w] in Hz: a smooth main-field inhomogeneity map, a second-order polynomial plus one Gaussian lobe (an air-tissue
    interface), scaled so that max |f| = max_hz.  Multiply by 2 pi for the rad/s of include/pnpadmm_offres.h."""
    u = hash_uniform(seed, 7101, 12).astype(np.float64)       # [-1, 1)
    yy, xx = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing="ij")
    f = u[0] * xx + u[1] * yy + u[2] * xx * yy + u[3] * (xx * xx - 0.5) + u[4] * (yy * yy - 0.5)
    cx, cy, s = 0.6 * u[5], 0.6 * u[6], 0.25 + 0.1 * (u[7] + 1.0)
    f = f + (1.5 if u[8] >= 0 else -1.5) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * s * s))
    return f * (float(max_hz) / max(float(np.abs(f).max()), 1e-30))


def offres_ndft_np(traj: np.ndarray, times: np.ndarray, omega: np.ndarray, x: np.ndarray, adjoint_shape=None) -> np.ndarray:
    """`ndft_np` under a field map, exact in float64: (A x)_m = (1 / sqrt(h w)) sum_q x[q] exp(-i omega[q] t_m) exp(-2 pi i k_m . q); with
    adjoint_shape = (h, w): A^H.  x [h,w] -> [M] (or [M] -> [h,w]): one slice; omega [h,w] rad/s, times [M] s.  O(M h w)."""
    traj = np.asarray(traj, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    om = np.asarray(omega, dtype=np.float64)
    h, w = om.shape
    sgn = 1.0 if adjoint_shape is not None else -1.0
    ey = np.exp(sgn * 2j * math.pi * traj[:, 0:1] * (np.arange(h) - h // 2))
    ex = np.exp(sgn * 2j * math.pi * traj[:, 1:2] * (np.arange(w) - w // 2))
    x = np.asarray(x, dtype=np.complex128)
    out = np.zeros((h, w), dtype=np.complex128) if adjoint_shape is not None else np.empty(t.size, dtype=np.complex128)
    for m0 in range(0, t.size, 256):
        sl = slice(m0, m0 + 256)
        ph = np.exp(sgn * 1j * om[None] * t[sl, None, None])
        if adjoint_shape is not None:
            out += np.einsum("my,m,mx,myx->yx", ey[sl], x[sl], ex[sl], ph, optimize=True)
        else:
            out[sl] = np.einsum("my,myx,mx->m", ey[sl], ph * x[None], ex[sl], optimize=True)
    return out / math.sqrt(h * w)


def make_problem_ncb0(n: int, h: int, w: int, traj: np.ndarray, times: np.ndarray, omega: np.ndarray, dcf: np.ndarray = None,
                      sigma_n: float = 10.0 / 255.0, seed: int = 1234, first_slice: int = 0) -> Dict[str, np.ndarray]:
    """`make_problem_nc` under main-field inhomogeneity, by the exact operator in float64 (small sizes): y = A_exact gt + noise with the
    sample times `times` float64 [M] (seconds) and the field map `omega` float32 [h,w] (shared) or [n,h,w] in rad/s; ATy0 = A_exact^H (dcf y).
    The dict carries `omega` and `times` beside `traj` and `dcf`."""
    traj = np.asarray(traj, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    m = traj.shape[0]
    om = np.asarray(omega, dtype=np.float32)
    d = None if dcf is None else np.asarray(dcf, dtype=np.float32)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    y0 = np.empty((n, 1, m, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        oi = om if om.ndim == 2 else om[i]
        y = offres_ndft_np(traj, t, oi, g) + (_gauss(s, 9001, m) + 1j * _gauss(s, 9003, m)) * sigma_n
        a = offres_ndft_np(traj, t, oi, y if d is None else y * d.astype(np.float64), adjoint_shape=(h, w))
        gt[i, 0] = g
        y0[i, 0, :, 0], y0[i, 0, :, 1] = y.real, y.imag
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
    x0 = np.clip(aty0, 0.0, None)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "gt": gt, "x0_raw": aty0[..., 0].copy(), "traj": traj, "dcf": d, "omega": om, "times": t}


def param_table(n: int, iters: int, seed: int = 77):
    """Seeded per-slice (mu_t, sigma_t) schedule standing in for DT-chosen parameters at
    sizes the 128x128-only policy cannot see: mu in (0.05,0.6), sigma_d
    decaying 50/255 -> 5/255 with per-slice jitter.  float32 [n,iters] each."""
    u = (hash_uniform(seed, 31, n * iters).astype(np.float64).reshape(n, iters) + 1.0) * 0.5
    v = (hash_uniform(seed, 32, n * iters).astype(np.float64).reshape(n, iters) + 1.0) * 0.5
    mu = 0.05 + 0.55 * u
    t = np.arange(iters) / max(iters - 1, 1)
    sig = (50.0 * (5.0 / 50.0) ** t)[None, :] * (0.9 + 0.2 * v) / 255.0
    return mu.astype(np.float32), sig.astype(np.float32)


# ---- multi-coil (SENSE) problems ------------------------------------------------------------------------------------------------------

def coil_maps(c: int, h: int, w: int, radius: float = 1.3, width: float = 1.1) -> np.ndarray:
    """complex128 [c,h,w]: analytic coil sensitivity maps, normalised to unit root-sum-of-squares at every pixel.  Coil k sits at angle
    2 pi k / c on a ring of `radius` (outside the field of view, in the phantom's [-1,1] coordinates); its magnitude is the Gaussian
    exp(-d^2 / (2 width^2)) of the distance d to the coil and its phase is linear, pi/2 (x cos + y sin) along the coil's direction.
    radius 1.3, width 1.1: RSS = 1 to 1e-15 and min |S| = 0.035 at 8 coils."""
    if c < 1:
        raise ValueError(f"coil_maps: need c >= 1, got {c}")
    yy, xx = np.meshgrid((np.arange(h) + 0.5) / h * 2 - 1, (np.arange(w) + 0.5) / w * 2 - 1, indexing="ij")
    out = np.empty((c, h, w), dtype=np.complex128)
    for k in range(c):
        th = 2.0 * math.pi * k / c
        d2 = (xx - radius * math.cos(th)) ** 2 + (yy - radius * math.sin(th)) ** 2
        out[k] = np.exp(-d2 / (2.0 * width ** 2)) * np.exp(0.5j * math.pi * (xx * math.cos(th) + yy * math.sin(th)))
    return out / np.sqrt((np.abs(out) ** 2).sum(axis=0, keepdims=True))


def noise_cov_model(c: int, rho: float = 0.4, gains=1.0, seed: int = 0) -> np.ndarray:
    """complex128 [c,c]: a channel noise covariance with unequal gains and correlated neighbours,
        Psi[a][b] = g_a g_b rho^|a-b| e^{i phi_(a-b)},   phi_d = d theta,  theta = pi hash_uniform(seed, 9201, 1)   (phi_-d = -phi_d: Hermitian).
    gains: the c gains g_a > 0, or one number s >= 1, the gain spread: g_a = s^(a / (c - 1)), a geometric ramp from 1 to s.  0 <= rho < 1.
    Psi = D R D^H with D = diag(g_a e^{i a theta}) and R the real AR(1) matrix rho^|a-b|, which is positive definite for every rho in
    [0, 1): so is Psi, with a condition number of at most (g_max / g_min)^2 (1 + rho) / (1 - rho).  Plain float64 arithmetic on a
    counter hash: the same bits on every machine."""
    if c < 1:
        raise ValueError(f"noise_cov_model: need c >= 1, got {c}")
    if not 0.0 <= rho < 1.0:
        raise ValueError(f"noise_cov_model: rho must be in [0, 1), got {rho}")
    if np.ndim(gains) == 0:
        if not float(gains) >= 1.0 or not math.isfinite(float(gains)):
            raise ValueError(f"noise_cov_model: a gain spread must be finite and >= 1, got {gains}")
        g = float(gains) ** (np.arange(c) / max(c - 1, 1))
    else:
        g = np.asarray(gains, dtype=np.float64)
        if g.shape != (c,) or not (g > 0).all() or not np.isfinite(g).all():
            raise ValueError(f"noise_cov_model: gains must be {c} finite positive numbers, got {gains!r}")
    theta = math.pi * float(hash_uniform(seed, 9201, 1)[0])
    d = np.arange(c)[:, None] - np.arange(c)[None, :]
    psi = (g[:, None] * g[None, :]) * float(rho) ** np.abs(d) * np.exp(1j * theta * d)
    psi[np.arange(c), np.arange(c)] = g * g                  # an exactly real diagonal
    return np.tril(psi) + np.tril(psi, -1).conj().T          # exactly Hermitian


def make_problem_mc(n: int, h: int, w: int, coils: int, accel: float = 4.0, sigma_n: float = 10.0 / 255.0, seed: int = 1234,
                    first_slice: int = 0, mask: np.ndarray = None) -> Dict[str, np.ndarray]:
    """`make_problem` for `coils` coils with the maps of `coil_maps`: y0 float32 [n,coils,h,w,2] with
    y_c = mask * (fft_c(S_c gt) + sigma_n noise_c), noise_c = the counter hash with the streams 9001 + 4 c / 9003 + 4 c (coil 0 draws
    `make_problem`'s noise); ATy0 = sum_c conj(S_c) ifft_c(y_c) and x0 = its clip at 0, float32 [n,1,h,w,2]; sens complex64 [coils,h,w];
    mask, gt, x0_raw as in `make_problem`."""
    mask = radial_mask(h, w, accel) if mask is None else np.asarray(mask).astype(bool)
    sens = coil_maps(coils, h, w)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    x0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    y0 = np.empty((n, coils, h, w, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        noise = np.stack([(_gauss(s, 9001 + 4 * c, h * w) + 1j * _gauss(s, 9003 + 4 * c, h * w)).reshape(h, w) for c in range(coils)])
        y = mask * (fft2c_np(sens * g) + sigma_n * noise)
        a = (np.conj(sens) * ifft2c_np(y)).sum(axis=0)
        gt[i, 0] = g
        y0[i, ..., 0], y0[i, ..., 1] = y.real, y.imag
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
        x0[i, 0] = np.clip(aty0[i, 0], 0.0, None)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "mask": mask, "gt": gt, "x0_raw": aty0[..., 0].copy(), "sens": sens.astype(np.complex64)}


def make_problem_ncmc(n: int, h: int, w: int, coils: int, traj: np.ndarray, dcf: np.ndarray = None, sigma_n: float = 10.0 / 255.0,
                      seed: int = 1234, first_slice: int = 0, sens: np.ndarray = None) -> Dict[str, np.ndarray]:
    """`make_problem_nc` for `coils` coils (non-Cartesian SENSE), by the exact NDFT in float64 (meant for small sizes): y0 float32
    [n,coils,M,2] with y_c = A (S_c gt) + sigma_n noise_c, noise_c = the counter hash indexed by the sample m with the streams 9001 + 4 c /
    9003 + 4 c (`make_problem_mc`'s) ; ATy0 = sum_c conj(S_c) A^H (dcf y_c) and x0 = its clip at 0, float32 [n,1,h,w,2]; sens complex64
    [coils,h,w] (`coil_maps` unless given); gt, x0_raw, traj, dcf as in `make_problem_nc`."""
    traj = np.asarray(traj, dtype=np.float64)
    m = traj.shape[0]
    d = None if dcf is None else np.asarray(dcf, dtype=np.float32)
    sens = (coil_maps(coils, h, w) if sens is None else np.asarray(sens)).astype(np.complex64)
    s64 = sens.astype(np.complex128)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    y0 = np.empty((n, coils, m, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        noise = np.stack([_gauss(s, 9001 + 4 * c, m) + 1j * _gauss(s, 9003 + 4 * c, m) for c in range(coils)])
        y = ndft_np(traj, s64 * g) + sigma_n * noise
        a = (np.conj(s64) * ndft_np(traj, y if d is None else y * d.astype(np.float64), adjoint_shape=(h, w))).sum(axis=0)
        gt[i, 0] = g
        y0[i, ..., 0], y0[i, ..., 1] = y.real, y.imag
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
    x0 = np.clip(aty0, 0.0, None)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "gt": gt, "x0_raw": aty0[..., 0].copy(), "traj": traj, "dcf": d, "sens": sens}


def make_problem_ncmcb0(n: int, h: int, w: int, coils: int, traj: np.ndarray, times: np.ndarray, omega: np.ndarray, dcf: np.ndarray = None,
                        sigma_n: float = 10.0 / 255.0, seed: int = 1234, first_slice: int = 0, sens: np.ndarray = None) -> Dict[str, np.ndarray]:
    """`make_problem_ncb0` for `coils` coils (off-resonance correction for multi-coil data, include/pnpadmm_offres_mc.h), by the exact
    operator in float64 (small sizes): y0 float32 [n,coils,M,2] with y_c = A_exact (S_c gt) + sigma_n noise_c under the field map `omega`
    (float32 [h,w] or [n,h,w], rad/s) at the sample times `times`, noise_c as in `make_problem_ncmc`; ATy0 = sum_c conj(S_c) A_exact^H (dcf y_c)
    and x0 = its clip at 0.  The dict carries `omega`, `times` and `sens` (complex64 [coils,h,w]: `coil_maps` unless given) beside `traj` and `dcf`."""
    traj = np.asarray(traj, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    m = traj.shape[0]
    om = np.asarray(omega, dtype=np.float32)
    d = None if dcf is None else np.asarray(dcf, dtype=np.float32)
    sens = (coil_maps(coils, h, w) if sens is None else np.asarray(sens)).astype(np.complex64)
    s64 = sens.astype(np.complex128)
    gt = np.empty((n, 1, h, w), dtype=np.float32)
    y0 = np.empty((n, coils, m, 2), dtype=np.float32)
    aty0 = np.empty((n, 1, h, w, 2), dtype=np.float32)
    for i in range(n):
        s = seed + first_slice + i
        g = phantom(h, w, s)
        oi = om if om.ndim == 2 else om[i]
        a = np.zeros((h, w), dtype=np.complex128)
        for c in range(coils):
            y = offres_ndft_np(traj, t, oi, s64[c] * g) + (_gauss(s, 9001 + 4 * c, m) + 1j * _gauss(s, 9003 + 4 * c, m)) * sigma_n
            a += np.conj(s64[c]) * offres_ndft_np(traj, t, oi, y if d is None else y * d.astype(np.float64), adjoint_shape=(h, w))
            y0[i, c, :, 0], y0[i, c, :, 1] = y.real, y.imag
        gt[i, 0] = g
        aty0[i, 0, ..., 0], aty0[i, 0, ..., 1] = a.real, a.imag
    x0 = np.clip(aty0, 0.0, None)
    return {"x0": x0, "y0": y0, "ATy0": aty0, "gt": gt, "x0_raw": aty0[..., 0].copy(), "traj": traj, "dcf": d, "omega": om, "times": t,
            "sens": sens}
