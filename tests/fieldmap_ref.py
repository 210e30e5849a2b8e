"""Numpy restatement of the field map fit of include/pnpadmm_fieldmap.h: in float64, and in float32 in the header's expression order (an fma
is formed in float64 and rounded once more: the product of two float32 values is exact in float64, the sum is then rounded twice, which
differs from a true fma in rare last-bit cases only - tests/tv_ref.py's convention).  The cost Psi, and the fixture `ESTIMATES` the host and
the GPU tests share: the two-echo scan of tests/offres_ref.py's `corrects_problem()`.

    s = sum_c x1_c conj(x2_c),  m = |s|,  phi = arg s,  w = m / max m
    Psi(theta) = sum_j w_j (1 - cos(theta_j - phi_j)) + (beta / 2) sum over 4-neighbour pairs (theta_j - theta_k)^2
    theta <- theta - (w sin(theta - phi) + beta lap) / (w + 2 beta nn),   all pixels at once, from theta = phi

x1, x2 complex [N,C,H,W]; omega [N,H,W] rad/s (float64 values whatever the arithmetic)."""
import math

import numpy as np

import offres_ref as OR

FUSE_T = 10                                                   # sweeps per launch of the fused kernel (PNP_FIELDMAP_T)


def _fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def neighbours(h, w):
    """[H,W]: the number of 4-neighbours inside the image, 2..4"""
    nn = np.full((h, w), 4.0)
    nn[0, :] -= 1
    nn[-1, :] -= 1
    nn[:, 0] -= 1
    nn[:, -1] -= 1
    return nn


def products32(x1, x2):
    """(s.x, s.y) float32 [N,H,W]: the header's fma chains over ascending coils, from +0"""
    a, b = np.asarray(x1, dtype=np.complex64), np.asarray(x2, dtype=np.complex64)
    n, c, h, w = a.shape
    sx, sy = np.zeros((n, h, w), np.float32), np.zeros((n, h, w), np.float32)
    for k in range(c):
        ar, ai, br, bi = a[:, k].real, a[:, k].imag, b[:, k].real, b[:, k].imag
        sx = _fma32(ar, br, sx)
        sx = _fma32(ai, bi, sx)
        sy = _fma32(ai, br, sy)
        sy = _fma32(-ar, bi, sy)
    return sx, sy


def prepare(x1, x2, f32=False):
    """(phi, w) [N,H,W] of the echo images, in the arithmetic asked for"""
    if not f32:
        s = (np.asarray(x1, dtype=np.complex128) * np.conj(np.asarray(x2, dtype=np.complex128))).sum(axis=1)
        m = np.abs(s)
        mx = m.reshape(m.shape[0], -1).max(axis=1)
        ri = np.where(mx > 0, 1.0 / np.where(mx > 0, mx, 1.0), 0.0)
        return np.arctan2(s.imag, s.real), m * ri[:, None, None]
    sx, sy = products32(x1, x2)
    n = sx.shape[0]
    m = np.sqrt(_fma32(sx, sx, sy * sy))
    phi = np.arctan2(sy.astype(np.float64), sx.astype(np.float64)).astype(np.float32)
    mx = m.reshape(n, -1).max(axis=1)
    ri = np.where(mx > 0, np.float32(1) / np.where(mx > 0, mx, np.float32(1)), np.float32(0)).astype(np.float32)
    return phi, m * ri[:, None, None]


def _shifted(t):
    """(up, down, left, right) of t [N,H,W]; an absent neighbour reads t itself"""
    up, dn, lf, rt = t.copy(), t.copy(), t.copy(), t.copy()
    up[:, 1:, :] = t[:, :-1, :]
    dn[:, :-1, :] = t[:, 1:, :]
    lf[:, :, 1:] = t[:, :, :-1]
    rt[:, :, :-1] = t[:, :, 1:]
    return up, dn, lf, rt


def sweep(t, phi, w, rd, beta, f32=False):
    up, dn, lf, rt = _shifted(t)
    sn = np.sin(t - phi)
    lap = ((t - up) + (t - dn)) + ((t - lf) + (t - rt))
    if f32:
        g = _fma32(np.float32(beta), lap, w * sn)
        return _fma32(-g, rd, t)
    return t - (beta * lap + w * sn) * rd


def estimate(x1, x2, dte, beta, iters, f32=False, trace=None):
    """omega [N,H,W] (float64 values).  trace: a list that receives theta (float64 values) before the first sweep and after every sweep"""
    phi, w = prepare(x1, x2, f32)
    nn = neighbours(*phi.shape[-2:])
    if f32:
        beta = np.float32(beta)
        rd = np.float32(1) / _fma32(np.float32(2) * beta, nn.astype(np.float32), w)
    else:
        rd = 1.0 / (w + 2.0 * float(np.float32(beta)) * nn)
        beta = float(np.float32(beta))                         # the library takes beta as float32
    t = phi.copy()
    if trace is not None:
        trace.append(t.astype(np.float64))
    for _ in range(iters):
        t = sweep(t, phi, w, rd, beta, f32)
        if trace is not None:
            trace.append(t.astype(np.float64))
    return t.astype(np.float64) / float(dte)


def psi_theta(theta, phi, w, beta):
    """Psi per slice [N] in float64 at theta [N,H,W]"""
    theta, phi, w = (np.asarray(v, dtype=np.float64) for v in (theta, phi, w))
    data = (w * (1.0 - np.cos(theta - phi))).reshape(theta.shape[0], -1).sum(axis=1)
    dr = (theta[:, :, :-1] - theta[:, :, 1:]) ** 2
    dd = (theta[:, :-1, :] - theta[:, 1:, :]) ** 2
    return data + 0.5 * float(np.float32(beta)) * (dr.reshape(theta.shape[0], -1).sum(axis=1) + dd.reshape(theta.shape[0], -1).sum(axis=1))


def cost(x1, x2, dte, beta, omega):
    """pnp_fieldmap_cost in float64: Psi at theta = float32(omega dte), the library's theta"""
    phi, w = prepare(x1, x2)
    theta = (np.asarray(omega, dtype=np.float64) * float(dte)).astype(np.float32)
    return psi_theta(theta, phi, w, beta)


# ---- the cases the GPU test runs and the CPU test measures (float32 against float64) ------------------------------------------------------
SHAPES = ((1, 16, 16), (1, 32, 32), (1, 160, 80), (2, 256, 256))      # (N, H, W)
ITERS = (0, 1, FUSE_T - 1, FUSE_T, FUSE_T + 1, 3 * FUSE_T + 2)
COILS = (1, 3, 8)
CASE_DTE, CASE_BETA, CASE_HZ, CASE_NOISE = 2e-3, 0.05, 150.0, 5.0 / 255.0
_case_cache = {}


def case(n, h, w, coils, seed=0):
    """(x1, x2 complex64 [N,C,H,W], omega_true [N,H,W]) of a phantom under a smooth map of at most CASE_HZ, analytic coil maps for C > 1"""
    key = (n, h, w, coils, seed)
    if key not in _case_cache:
        from dt4image_restoration_amd import acquisition, synthetic
        gt = np.stack([synthetic.phantom(h, w, seed + 3 + i) for i in range(n)])
        om = np.stack([2.0 * math.pi * synthetic.field_map(h, w, CASE_HZ, seed + i) for i in range(n)])
        sens = synthetic.coil_maps(coils, h, w) if coils > 1 else None
        x1, x2 = acquisition.field_map_scan(gt, om, 1e-3, CASE_DTE, CASE_NOISE, seed + 40, sens=sens)
        _case_cache[key] = (x1, x2, om)
    return _case_cache[key]


# ---- "the estimate helps": the fixture the host and the GPU tests share ----------------------------------------------------------------------
# the two-echo scan of offres_ref.corrects_problem() (32 x 32, omega_max = 150 Hz: omega_max dte = 0.6 pi), then offres_ref.corrects_admm under
# the estimated map
ESTIMATES = dict(dte=2e-3, te=1e-3, noise=5.0 / 255.0, beta=0.05, iters=200, seed=21)
# PSNR in dB of the float64 restatement (tests/test_fieldmap_host.py produces them): the regularised estimate, the raw phase difference;
# offres_ref.CORRECTS_PSNR holds the other two (true map, no map)
ESTIMATES_PSNR = (28.415, 20.223)
# ... and how far the same float64 run moves when it is given the map of the FLOAT32 restatement instead (that map differs by 1.25e-05 Hz), dB
ESTIMATES_F32_GAP = 2.64e-07
_est_cache = {}


def estimates_scan():
    """(x1, x2 complex64 [1,1,h,w]) of the fixture"""
    if "scan" not in _est_cache:
        from dt4image_restoration_amd import acquisition
        e = ESTIMATES
        _, _, omega, gt, _, _ = estimates_problem()
        _est_cache["scan"] = acquisition.field_map_scan(gt[None], omega, e["te"], e["dte"], e["noise"], e["seed"])
    return _est_cache["scan"]


def estimates_problem():
    if "problem" not in _est_cache:
        _est_cache["problem"] = OR.corrects_problem()
    return _est_cache["problem"]


def estimates_psnr(omega_est):
    """PSNR of offres_ref.corrects_admm in float64 under the map omega_est [h,w]: the segments and the data are the true map's"""
    import dcf_ref
    import nufft_ref as NR
    c = OR.CORRECTS
    traj, t, _, gt, y, L = estimates_problem()
    if "plan" not in _est_cache:
        P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
        _est_cache["plan"] = (P, dcf_ref.pipe(P, 30)[0], OR.plan(t, L))
    P, dcf, Q = _est_cache["plan"]
    E = OR.maps(np.asarray(omega_est, dtype=np.float32).astype(np.float64), Q).astype(np.complex64).astype(np.complex128)
    return OR.corrects_admm(P, lambda p: OR.model_forward(P, Q, E, p), lambda q: OR.model_adjoint(P, Q, E, q, dcf), y, gt, dcf)[0]
