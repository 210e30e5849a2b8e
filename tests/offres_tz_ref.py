"""Float64 restatement of the Toeplitz form of the off-resonance normal operator (include/pnpadmm_offres_tz.h); no tests in here.

    A = sum_l diag(B[l]) F diag(E_l)           A^H W A p = sum_l conj(E_l) . sum_l' Toep[u_ll'](E_l' . p),   u_ll' = w B[l] B[l']
    K_ll'[j, k] = (1 / (H W)) sum_m u_ll'(m) D_H(ky_m - (j - H) / 2H) D_W(kx_m - (k - W) / 2W)
    X_l' = fft2c(pad(E_l' . p))     Y_l = sum_l' K_ll' . X_l'     q = sum_l conj(E_l) . crop(ifft2c(Y_l))

B [L, M] is the table of the STORED float32 coefficients as float64 (tests/offres_ref.py: weights(plan) for the linear interpolator, the
device's table for least squares), E [L,H,W] or [N,L,H,W] the segment maps the caller hands in (the tests hand in the device's own).  Four
restatements: the dense operator by NDFT matrices (dense_normal), the spectra by direct Dirichlet sums (spectra), the FFT form (apply) and
the FFT form with every stage rounded to complex64 (apply_f32), plus the CG stage on the FFT form."""
import numpy as np

import ncsense_ref as NS
import nufft_ref as NR
import offres_ls_ref as LS
import toeplitz_ref as T


def pairs(kind, L):
    """the pair order of pnp_offres_tz_spectrum: kind "linear" - (l, l), (l, l+1) interleaved; "ls" - the upper triangle row by row"""
    if kind == "linear":
        out = []
        for l in range(L):
            out.append((l, l))
            if l + 1 < L:
                out.append((l, l + 1))
        return out
    return [(l, r) for l in range(L) for r in range(l, L)]


def pair_weights(B, wgt=None):
    """u [L, L, M] float64 = w B[l] B[l']"""
    B = np.asarray(B, dtype=np.float64)
    w = np.ones(B.shape[1]) if wgt is None else np.asarray(wgt, dtype=np.float64)
    return w[None, None, :] * B[:, None, :] * B[None, :, :]


def nonzero_blocks(B, wgt=None):
    """the (l, l') with a sample that carries weight in both: the structure of A^H W A"""
    u = pair_weights(B, wgt)
    return [(l, r) for l in range(u.shape[0]) for r in range(u.shape[1]) if np.any(u[l, r] != 0.0)]


def spectra(traj, h, w, B, kind, wgt=None):
    """float64 [P, 2H, 2W] in the header's pair order, each by toeplitz_ref.spectrum's direct Dirichlet sum"""
    u = pair_weights(B, wgt)
    return np.stack([T.spectrum(traj, h, w, u[l, r]) for l, r in pairs(kind, u.shape[0])])


def spectra_bound(traj, h, w, B, kind, wgt=None):
    """[P, 2H, 2W]: M 2^-52 sum_m |u| |D_H| |D_W| / (H W) per pair - to which the test adds 2^-24 |K|, the one rounding to float32"""
    u = np.abs(pair_weights(B, wgt))
    return np.stack([T.spectrum_bound(traj, h, w, u[l, r]) for l, r in pairs(kind, u.shape[0])])


def full_matrix(K, kind, L):
    """[L, L, 2H, 2W] symmetric from the stored spectra [P, 2H, 2W]; zeros outside the band of a linear plan"""
    K = np.asarray(K, dtype=np.float64)
    full = np.zeros((L, L) + K.shape[-2:])
    for p, (l, r) in enumerate(pairs(kind, L)):
        full[l, r] = K[p]
        full[r, l] = K[p]
    return full


def _maps4(E, n):
    E = np.asarray(E, dtype=np.complex128)
    return np.broadcast_to(E, (n,) + E.shape[-3:])


def apply(Kfull, E, p, stage=None):
    """the FFT form, [N,H,W]; stage: a rounding applied to the segment images, both transforms' results, the mix and the result"""
    p = np.asarray(p, dtype=np.complex128)
    h, w = p.shape[-2:]
    p = p.reshape(-1, h, w)
    n, L = p.shape[0], Kfull.shape[0]
    E4 = _maps4(E, n)
    r = stage or (lambda a: a)
    g = np.zeros((n, L, 2 * h, 2 * w), dtype=np.complex128)
    g[:, :, h // 2:h // 2 + h, w // 2:w // 2 + w] = r(E4 * p[:, None])
    X = r(NR.fft2c(g.reshape(n * L, 2 * h, 2 * w))).reshape(n, L, 2 * h, 2 * w)
    Y = r(np.einsum("lrjk,nrjk->nljk", np.asarray(Kfull, dtype=np.float64), X, optimize=True))
    y = r(NR.ifft2c(Y.reshape(n * L, 2 * h, 2 * w))).reshape(n, L, 2 * h, 2 * w)[:, :, h // 2:h // 2 + h, w // 2:w // 2 + w]
    return r((np.conj(E4) * y).sum(axis=1))


def _c64(a):
    return a.astype(np.complex64).astype(np.complex128)


def apply_f32(Kfull, E, p):
    """the float32 restatement: the spectra rounded to float32, the input, the maps and every stage's result rounded to complex64, float64
    arithmetic in between"""
    return apply(np.asarray(Kfull).astype(np.float32).astype(np.float64), _c64(np.asarray(E)), _c64(np.asarray(p)), stage=_c64)


def dense_normal(traj, B, E, p, wgt=None):
    """A^H W A p with dense NDFT matrices for F: the operator the spectra must reproduce"""
    p = np.asarray(p, dtype=np.complex128)
    h, w = p.shape[-2:]
    B = np.asarray(B, dtype=np.float64)
    f = LS.segmented_forward(traj, None, B, None, p, E=E)
    return LS.segmented_adjoint(traj, None, B, None, f, h, w, wgt, E=E)


def apply_mc(Kfull, E, S, p):
    """sum_c conj(S_c) . apply(S_c . p); S [C,H,W] or [N,C,H,W]"""
    p = np.asarray(p, dtype=np.complex128)
    p = p.reshape(-1, *p.shape[-2:])
    S4 = NS._maps4(S, p.shape[0])
    out = np.zeros_like(p)
    for c in range(S4.shape[1]):
        out += np.conj(S4[:, c]) * apply(Kfull, E, S4[:, c] * p)
    return out


def apply_mc_f32(Kfull, E, S, p):
    p = _c64(np.asarray(p, dtype=np.complex128).reshape(-1, *np.asarray(p).shape[-2:]))
    S4 = _c64(np.asarray(NS._maps4(S, p.shape[0])))
    out = np.zeros_like(p)
    for c in range(S4.shape[1]):
        out = _c64(out + np.conj(S4[:, c]) * apply_f32(Kfull, E, _c64(S4[:, c] * p)))
    return out


def dense_normal_mc(traj, B, E, S, p, wgt=None):
    p = np.asarray(p, dtype=np.complex128)
    p = p.reshape(-1, *p.shape[-2:])
    S4 = NS._maps4(S, p.shape[0])
    out = np.zeros_like(p)
    for c in range(S4.shape[1]):
        out += np.conj(S4[:, c]) * dense_normal(traj, B, E, S4[:, c] * p, wgt)
    return out


def normal(Kfull, E, p, mu, S=None):
    p = np.asarray(p, dtype=np.complex128)
    p = p.reshape(-1, *p.shape[-2:])
    q = apply(Kfull, E, p) if S is None else apply_mc(Kfull, E, S, p)
    return q + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * p


def corrects_psnr(Kfull, E, aty, gt, S=None):
    """tests/offres_ref.py's CORRECTS fixture run as the stage runs it: TV-ADMM in float64 from x0 = aty (the gridding model's A^H W y, the
    caller's) with the K-step CG on the Toeplitz operator; the final PSNR in dB"""
    import offres_ref as OR
    import tv_ref
    c = OR.CORRECTS
    x, z, u = aty.real.copy(), aty.copy(), np.zeros_like(aty)
    mu = np.full(1, c["mu"])
    for s in OR.corrects_schedule():
        x = tv_ref.tv((z - u).real, np.full(1, float(s)), c["tv_iters"])
        z, u, _ = prox_dual(Kfull, E, x, z, u, aty, mu, c["K"], S)
    return float(tv_ref.psnr(x, gt[None])[0])


def prox_dual(Kfull, E, x, z, u, aty, mu, iters, S=None):
    """tests/ncsense_ref.py's K-step CG on the Toeplitz operator; aty is the caller's (the gridding model's A^H W y).  (z, u, cg_res)"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    zn, res = NS.cg_solve(None, z, x, u, aty, None, mu, iters, op=lambda p: normal(Kfull, E, p, mu, S))
    return zn, u + x - zn, res
