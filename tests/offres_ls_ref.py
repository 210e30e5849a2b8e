"""Float64 restatement of the off-resonance operator with the least-squares temporal interpolator of include/pnpadmm_offres_ls.h.  The plan
(centres, G, Cholesky, coefficients) is `acquisition.offres_ls_coeffs`; here are the model error, the operators with a coefficient table
B [L, M] in the place of tests/offres_ref.py's two weights per sample, and the figures of the shared fixture.

    A p   = [ sum_l B[l, m] F(E_l . p)_m ]_m,   E_l = exp(-i omega tau_l)
    A^H q = sum_l conj(E_l) . F^H(w . B[l] . q)

F is the dense DFT (segmented_*) or the float64 NUFFT model on the plan (model_*).  B is whatever the caller hands in: the tests hand in the
float32 table the device or the stand-alone program produced, so the model runs on the numbers the library multiplies with."""
import math

import numpy as np

import ncsense_ref as NS
import nufft_ref as NR
import offres_ref as OR

RIDGE = 1e-10

# worst model error over the band and a 10 ms span, float32 coefficients: the table of the issue this feature answers (omega_max span / pi, L)
TABLE = {(2, 6): 6.0e-3, (2, 8): 1.2e-4, (2, 10): 3.8e-5, (2, 12): 1.8e-5,
         (3, 6): 6.5e-2, (3, 8): 2.8e-3, (3, 10): 1.0e-4, (3, 12): 4.8e-5,
         (6, 12): 4.2e-3, (6, 16): 1.5e-4, (6, 24): 3.0e-5, (6, 32): 1.4e-5}

# tests/offres_ref.py's CORRECTS fixture with the least-squares interpolator at L = 8 through corrects_admm, float64 NUFFT model:
# (PSNR dB, weighted misfit at x = gt); produced by tests/test_offres_ls_host.py
CORRECTS_LS_L = 8
CORRECTS_LS = (50.573, 4.38e-3)
LINEAR_L32_MISFIT = 2.33e-2                                   # the linear interpolator at L = 32 on the same fixture (tests/test_gpu_offres.py)


def centres(times, L):
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    return OR.plan(t, L)["tau"]                               # exactly plan_offres' centres (the CPU suite compares their bits)


def plan_like(times, L):
    """the part of offres_ref.plan's dict that `offres_ref.maps` reads"""
    return dict(L=L, tau=centres(times, L))


def model_error(times, tau, B, omegas):
    """max over the given frequencies and times of |exp(-i omega t) - sum_l B[l] exp(-i omega tau_l)|, float64"""
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    B = np.asarray(B, dtype=np.float64)
    worst = 0.0
    om = np.asarray(omegas, dtype=np.float64).reshape(-1)
    for k0 in range(0, om.size, 256):
        o = om[k0:k0 + 256]
        fit = (np.exp(-1j * o[:, None, None] * np.asarray(tau)[None, :, None]) * B[None]).sum(axis=1)
        worst = max(worst, float(np.abs(np.exp(-1j * o[:, None] * t[None]) - fit).max()))
    return worst


def band(omega_max, L):
    return np.linspace(-omega_max, omega_max, max(16 * L + 1, 257))


def segmented_forward(traj, tau, B, omega, x, E=None):
    x = np.asarray(x, dtype=np.complex128)
    h, w = x.shape[-2:]
    x = x.reshape(-1, h, w)
    E = OR.maps(omega, dict(tau=np.asarray(tau))) if E is None else np.asarray(E, dtype=np.complex128)
    E = np.broadcast_to(E, (x.shape[0],) + E.shape[-3:])
    out = np.zeros((x.shape[0], B.shape[1]), dtype=np.complex128)
    for l in range(B.shape[0]):
        out += B[l] * NR.ndft(traj, E[:, l] * x)
    return out


def segmented_adjoint(traj, tau, B, omega, y, h, w, wgt=None, E=None):
    y = np.asarray(y, dtype=np.complex128).reshape(-1, B.shape[1])
    E = OR.maps(omega, dict(tau=np.asarray(tau))) if E is None else np.asarray(E, dtype=np.complex128)
    E = np.broadcast_to(E, (y.shape[0],) + E.shape[-3:])
    out = np.zeros((y.shape[0], h, w), dtype=np.complex128)
    for l in range(B.shape[0]):
        out += np.conj(E[:, l]) * NR.ndft_adjoint(traj, B[l] * y, h, w, wgt)
    return out


def model_forward(P, B, E, x):
    x = np.asarray(x, dtype=np.complex128).reshape(-1, P["h"], P["w"])
    E = np.broadcast_to(np.asarray(E, dtype=np.complex128), (x.shape[0],) + np.asarray(E).shape[-3:])
    out = np.zeros((x.shape[0], P["m"]), dtype=np.complex128)
    for l in range(B.shape[0]):
        out += B[l] * NR.forward(P, E[:, l] * x)
    return out


def model_adjoint(P, B, E, y, wgt=None):
    y = np.asarray(y, dtype=np.complex128).reshape(-1, P["m"])
    E = np.broadcast_to(np.asarray(E, dtype=np.complex128), (y.shape[0],) + np.asarray(E).shape[-3:])
    out = np.zeros((y.shape[0], P["h"], P["w"]), dtype=np.complex128)
    for l in range(B.shape[0]):
        out += np.conj(E[:, l]) * NR.adjoint(P, B[l] * y, wgt)
    return out


def model_normal(P, B, E, p, mu, wgt=None):
    return model_adjoint(P, B, E, model_forward(P, B, E, p), wgt) + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * p


def prox_dual(P, B, E, x, z, u, aty, mu, iters, wgt=None):
    zn, res = NS.cg_solve(P, z, x, u, aty, None, mu, iters, wgt, op=lambda p: model_normal(P, B, E, p, mu, wgt))
    return zn, u + x - zn, res


def dc_misfit(P, B, E, x, y, wgt=None):
    d = np.abs(model_forward(P, B, E, x) - y) ** 2
    d = d if wgt is None else d * np.asarray(wgt, dtype=np.float64)
    return np.sqrt(d.sum(axis=1))
