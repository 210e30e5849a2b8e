"""Float64 restatement of the Toeplitz normal operator (include/pnpadmm_toeplitz.h): the spectrum K by the real rank-1 Dirichlet sum (and, as
its check, by the transform of the directly summed T), its per-entry rounding bound, the application on the 2H x 2W grid, the single- and
multi-coil normal operators, the K-step CG of the two non-Cartesian stages on them, the cases the host and GPU tests share and the
end-to-end constants.

    K[j, l] = (1 / (H W)) sum_m w_m D_H(ky_m - (j - H) / 2H) D_W(kx_m - (l - W) / 2W)        q = crop(ifft2c(K . fft2c(pad(p))))

The right-hand side of the stages, aty = A^H W y, stays on the NUFFT model of tests/nufft_ref.py, as it does in the library."""
import math

import numpy as np

import ncsense_ref as SR
import nufft_ref as NR

# (N, H, W): after the five of nufft_ref.CASES (indices 0..4), the mixed-radix family at 160 and the thin shapes that reach every row and
# column length up to 1024 of the power-of-two family, all on nufft_ref.SPOKES golden-angle spokes
EXTRA_SHAPES = ((1, 80, 80), (1, 64, 80), (1, 128, 16), (1, 256, 16), (1, 512, 16), (1, 16, 128), (1, 16, 256), (1, 16, 512))
N_CASES = len(NR.CASES) + len(EXTRA_SHAPES)


def case_shape(i):
    return NR.CASES[i][:3] if i < len(NR.CASES) else EXTRA_SHAPES[i - len(NR.CASES)]


def case_traj(i):
    if i < len(NR.CASES):
        return NR.case_traj(i)
    n, h, w = case_shape(i)
    return NR.radial(h, w, NR.SPOKES)


def case_image(i, seed=0):
    n, h, w = case_shape(i)
    rng = np.random.default_rng(1000 + 17 * i + seed)
    return rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))


def case_weights(i):
    """float32 [M] in [0.25, 1.75): non-trivial, positive"""
    m = case_traj(i).shape[0]
    return np.random.default_rng(7 + i).uniform(0.25, 1.75, m).astype(np.float32)


# ---- the spectrum ----------------------------------------------------------------------------------------------------------------------------
def dirichlet(t, n):
    """D_n(t) = sum_{d = -(n-1)}^{n-1} exp(2 pi i d t), real; t is reduced to t - rint(t) first and t == 0 takes the limit 2n - 1 (a sample at
    k = +-0.5 against the bin -0.5 gives the integer 1, where sin(pi t) is 1e-16 and the quotient garbage)"""
    t = np.asarray(t, dtype=np.float64)
    t = t - np.rint(t)
    zero = t == 0.0
    return np.where(zero, 2.0 * n - 1.0, np.sin((2 * n - 1) * math.pi * t) / np.where(zero, 1.0, np.sin(math.pi * t)))


def _dirichlets(traj, h, w):
    traj = np.asarray(traj, dtype=np.float64)
    j = (np.arange(2 * h) - h) / (2.0 * h)
    l = (np.arange(2 * w) - w) / (2.0 * w)
    return dirichlet(traj[:, 0:1] - j[None, :], h), dirichlet(traj[:, 1:2] - l[None, :], w)      # [M, 2H], [M, 2W]


def spectrum(traj, h, w, wgt=None):
    """float64 [2H, 2W], centred"""
    dy, dx = _dirichlets(traj, h, w)
    wgt = np.ones(dy.shape[0]) if wgt is None else np.asarray(wgt, dtype=np.float64)
    return np.einsum("m,mj,ml->jl", wgt, dy, dx, optimize=True) / (h * w)


def spectrum_bound(traj, h, w, wgt=None):
    """B[j, l] = M 2^-52 sum_m w_m |D_H| |D_W| / (H W): the rounding of an M-term float64 sum, whatever its order"""
    dy, dx = _dirichlets(traj, h, w)
    wgt = np.ones(dy.shape[0]) if wgt is None else np.abs(np.asarray(wgt, dtype=np.float64))
    return dy.shape[0] * 2.0 ** -52 * np.einsum("m,mj,ml->jl", wgt, np.abs(dy), np.abs(dx), optimize=True) / (h * w)


def spectrum_by_lags(traj, h, w, wgt=None):
    """complex128 [2H, 2W]: the centred unnormalised DFT of the directly summed T (the lags -H and -W left out); its real part is `spectrum`"""
    traj = np.asarray(traj, dtype=np.float64)
    wgt = np.ones(traj.shape[0]) if wgt is None else np.asarray(wgt, dtype=np.float64)
    ey = np.exp(2j * math.pi * traj[:, 0:1] * np.arange(-h, h))
    ex = np.exp(2j * math.pi * traj[:, 1:2] * np.arange(-w, w))
    ey[:, 0] = 0
    ex[:, 0] = 0
    T = np.einsum("m,my,mx->yx", wgt, ey, ex, optimize=True) / (h * w)                          # lag 0 at index (h, w)
    return np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(T)))


# ---- the application ---------------------------------------------------------------------------------------------------------------------------
def apply(K, p, stage=None):
    """crop(ifft2c(K . fft2c(pad(p)))), [N,H,W]; stage: a rounding applied after each of the four steps (the float32 restatement)"""
    p = np.asarray(p, dtype=np.complex128)
    h, w = p.shape[-2:]
    p = p.reshape(-1, h, w)
    r = stage or (lambda a: a)
    g = np.zeros((p.shape[0], 2 * h, 2 * w), dtype=np.complex128)
    g[:, h // 2:h // 2 + h, w // 2:w // 2 + w] = p
    G = r(r(NR.fft2c(g)) * np.asarray(K, dtype=np.float64))
    return r(NR.ifft2c(G))[:, h // 2:h // 2 + h, w // 2:w // 2 + w]


def _c64(a):
    return a.astype(np.complex64).astype(np.complex128)


def apply_f32(K, p):
    """the float32 restatement: K rounded to float32, the input and every stage's result rounded to complex64, float64 transforms in between"""
    return apply(np.asarray(K).astype(np.float32), _c64(np.asarray(p)), stage=_c64)


def normal(K, p, mu):
    return apply(K, p) + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * np.asarray(p).reshape(-1, *np.asarray(p).shape[-2:])


def apply_mc(K, p, S):
    """sum_c conj(S_c) . Toep(S_c . p); S [C,H,W] or [N,C,H,W]"""
    p = np.asarray(p, dtype=np.complex128)
    p = p.reshape(-1, *p.shape[-2:])
    S4 = SR._maps4(S, p.shape[0])
    out = np.zeros_like(p)
    for c in range(S4.shape[1]):
        out += np.conj(S4[:, c]) * apply(K, S4[:, c] * p)
    return out


def normal_mc(K, p, S, mu):
    p = np.asarray(p, dtype=np.complex128)
    p = p.reshape(-1, *p.shape[-2:])
    return apply_mc(K, p, S) + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * p


# ---- the data-fidelity stages: the CG of tests/ncsense_ref.py (nufft_ref.cg_solve word for word, with a replaceable operator) --------------------
def cg_solve(K, z0, x, u, aty, mu, iters, S=None):
    """K-step CG on the Toeplitz Nop (single-coil, or multi-coil with maps S); aty is the caller's (the NUFFT model's A^H W y)"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    op = (lambda p: normal(K, p, mu)) if S is None else (lambda p: normal_mc(K, p, S, mu))
    return SR.cg_solve(None, z0, x, u, aty, None, mu, iters, op=op)


def prox_dual(K, x, z, u, aty, mu, iters, S=None):
    zn, res = cg_solve(K, z, x, u, aty, mu, iters, S)
    return zn, u + x - zn, res


# ---- end to end: the two fixtures of nufft_ref / ncsense_ref with the Toeplitz operator inside the CG ------------------------------------------
# (x0, final) PSNR of the float64 restatements below, dB; produced by tests/test_toeplitz_host.py
FIXTURE_PSNR = (16.572, 36.812)
FIXTURE_PSNR_MC = (17.493, 32.399)


def admm_tv_nc(d, P, mu, sigma, cg_iters, tv_scale, tv_iters):
    """nufft_ref.admm_tv_nc with the Toeplitz operator of (the plan's trajectory, the problem's dcf) inside the CG"""
    import tv_ref
    x0 = tv_ref.cplx(d["x0"])[:, 0]
    y = tv_ref.cplx(d["y0"])[:, 0]
    gt = d["gt"][:, 0].astype(np.float64)
    wgt = None if d.get("dcf") is None else d["dcf"].astype(np.float64)
    n = x0.shape[0]
    K = spectrum(np.asarray(d["traj"], dtype=np.float64), P["h"], P["w"], wgt)
    aty = NR.adjoint(P, y, wgt)
    x, z, u = x0.real.copy(), x0.copy(), np.zeros_like(x0)
    p0 = tv_ref.psnr(x, gt)
    for k in range(len(sigma)):
        lam = np.full(n, float(np.float32(tv_scale)) * float(np.float32(sigma[k])))
        x = tv_ref.tv((z - u).real, lam, tv_iters)
        z, u, _ = prox_dual(K, x, z, u, aty, np.full(n, float(np.float32(mu[k]))), cg_iters)
    return x, p0, tv_ref.psnr(x, gt)


def admm_tv_ncmc(d, P, mu, sigma, cg_iters, tv_scale, tv_iters):
    """ncsense_ref.admm_tv with the Toeplitz operator inside the CG"""
    import tv_ref
    x0 = tv_ref.cplx(d["x0"])[:, 0]
    y = tv_ref.cplx(d["y0"])
    S = np.asarray(d["sens"]).astype(np.complex128)
    gt = d["gt"][:, 0].astype(np.float64)
    wgt = None if d.get("dcf") is None else d["dcf"].astype(np.float64)
    n = x0.shape[0]
    K = spectrum(np.asarray(d["traj"], dtype=np.float64), P["h"], P["w"], wgt)
    aty = SR.AH(P, y, S, wgt)
    x, z, u = x0.real.copy(), x0.copy(), np.zeros_like(x0)
    p0 = tv_ref.psnr(x, gt)
    for k in range(len(sigma)):
        lam = np.full(n, float(np.float32(tv_scale)) * float(np.float32(sigma[k])))
        x = tv_ref.tv((z - u).real, lam, tv_iters)
        z, u, _ = prox_dual(K, x, z, u, aty, np.full(n, float(np.float32(mu[k]))), cg_iters, S)
    return x, p0, tv_ref.psnr(x, gt)
