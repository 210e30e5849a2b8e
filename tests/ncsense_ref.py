"""Float64 restatement of the non-Cartesian SENSE stage (include/pnpadmm_ncsense.h), composed from tests/nufft_ref.py (the NUFFT model: the
plan's float32-rounded weights and factors, float64 arithmetic) and the coil maps: the operators A, A^H, Nop, the K-step CG of the
data-fidelity stage, the misfit, the exact acquisition, the operator norm, the cases the host and GPU tests share and the end-to-end fixture.

    A p   = [ F_nu(S_c . p) ]_c          A^H q = sum_c conj(S_c) . F_nu^H(w . q_c)          Nop(p) = A^H W A p + mu p

Maps: S [C,H,W] (shared) or [N,C,H,W]; samples [N,C,M]; images [N,H,W]."""
import math

import numpy as np

import nufft_ref as NR

from dt4image_restoration_amd import synthetic
from dt4image_restoration_amd.weights import hash_uniform

# (index into nufft_ref.CASES, coils): the five small grids 16 x 16 .. 64 x 64 with 1, 3, 5 and 9 coils between them - 9 crosses the default
# block of 8 raggedly - and one 16 x 16 case at the largest coil count
CASES = ((0, 3), (1, 5), (2, 9), (3, 1), (4, 9), (0, 32))


def _maps4(S, n):
    S = np.asarray(S, dtype=np.complex128)
    return np.broadcast_to(S, (n,) + S.shape) if S.ndim == 3 else S


def case_maps(k, per_slice=False):
    """complex128 maps of CASES[k], rounded to complex64: synthetic.coil_maps (sum_c |S_c|^2 = 1) times a per-coil phase and, per slice, a
    smooth modulation that differs from slice to slice"""
    i, c = CASES[k]
    n, h, w = NR.CASES[i][:3]
    S = synthetic.coil_maps(c, h, w).astype(np.complex128)
    ph = hash_uniform(700 + k, 3, c).astype(np.float64) * math.pi
    S = S * np.exp(1j * ph)[:, None, None]
    if per_slice:
        yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
        S = np.stack([S * np.exp(0.3j * (j + 1) * (yy - 0.5 * xx)) * (1.0 - 0.1 * j * xx) for j in range(n)])
    return S.astype(np.complex64).astype(np.complex128)


def case_samples(k, m, seed=0):
    i, c = CASES[k]
    n = NR.CASES[i][0]
    rng = np.random.default_rng(3000 + 17 * k + seed)
    return rng.standard_normal((n, c, m)) + 1j * rng.standard_normal((n, c, m))


# ---- the operators ---------------------------------------------------------------------------------------------------------------------------
def A(P, x, S):
    """[N,C,M]"""
    x = np.asarray(x, dtype=np.complex128).reshape(-1, P["h"], P["w"])
    S4 = _maps4(S, x.shape[0])
    return np.stack([NR.forward(P, S4[:, c] * x) for c in range(S4.shape[1])], axis=1)


def AH(P, y, S, wgt=None):
    """[N,H,W]"""
    y = np.asarray(y, dtype=np.complex128)
    S4 = _maps4(S, y.shape[0])
    out = np.zeros((y.shape[0], P["h"], P["w"]), dtype=np.complex128)
    for c in range(S4.shape[1]):
        out += np.conj(S4[:, c]) * NR.adjoint(P, y[:, c], wgt)
    return out


def normal(P, p, S, mu, wgt=None):
    return AH(P, A(P, p, S), S, wgt) + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * p


def _dot(a, b):
    return (a.real * b.real + a.imag * b.imag).reshape(a.shape[0], -1).sum(axis=1)


def cg_solve(P, z0, x, u, aty, S, mu, iters, wgt=None, op=None):
    """the multi-coil section's K-step CG on Nop; returns (z, cg_res [N]).  op: another normal operator (cg_solve_f32)"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    m3 = mu.reshape(-1, 1, 1)
    nop = op or (lambda p: normal(P, p, S, mu, wgt))
    b = aty + m3 * (x + u)
    z = np.array(z0, dtype=np.complex128)
    r = b - nop(z)
    p = r.copy()
    rs, bb = _dot(r, r), _dot(b, b)
    for _ in range(iters):
        q = nop(p)
        pq = _dot(p, q)
        ok = (rs > 0) & (pq > 0)
        alpha = np.where(ok, rs / np.where(ok, pq, 1.0), 0.0)
        z = z + alpha.reshape(-1, 1, 1) * p
        r = r - alpha.reshape(-1, 1, 1) * q
        rs2 = _dot(r, r)
        beta = np.where(ok, rs2 / np.where(ok, rs, 1.0), 0.0)
        p = r + beta.reshape(-1, 1, 1) * p
        rs = rs2
    return z, np.where(bb > 0, np.sqrt(rs / np.where(bb > 0, bb, 1.0)), 0.0)


def prox_dual(P, x, z, u, aty, S, mu, iters, wgt=None):
    zn, res = cg_solve(P, z, x, u, aty, S, mu, iters, wgt)
    return zn, u + x - zn, res


def dc_misfit(P, x, y, S, wgt=None):
    d = np.abs(A(P, x, S) - y) ** 2
    d = d if wgt is None else d * np.asarray(wgt, dtype=np.float64)
    return np.sqrt(d.sum(axis=(1, 2)))


def acquire(traj, gt, S, sigma_n, seed, first_slice=0):
    """y [N,C,M] by the exact NDFT of S_c gt plus the counter-hash noise of pnp_acquire_ncsense (streams 9001 + 4 c / 9003 + 4 c, seed + n)"""
    gt = np.asarray(gt, dtype=np.float64)
    gt = gt.reshape(-1, gt.shape[-2], gt.shape[-1])
    S4 = _maps4(S, gt.shape[0])
    m = np.asarray(traj).shape[0]
    y = np.stack([NR.ndft(traj, S4[:, c] * gt) for c in range(S4.shape[1])], axis=1)
    if sigma_n:
        for j in range(gt.shape[0]):
            for c in range(S4.shape[1]):
                y[j, c] += sigma_n * (synthetic._gauss(seed + first_slice + j, 9001 + 4 * c, m)
                                      + 1j * synthetic._gauss(seed + first_slice + j, 9003 + 4 * c, m))
    return y


def op_norm(P, S, iters=30):
    """||A|| of the model by power iteration on A^H A (one slice: S [C,H,W])"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, P["h"], P["w"])) + 1j * rng.standard_normal((1, P["h"], P["w"]))
    s = 0.0
    for _ in range(iters):
        x /= np.linalg.norm(x)
        x = AH(P, A(P, x, S), S)
        s = math.sqrt(np.linalg.norm(x))
    return s


# ---- the end-to-end fixture (tests/test_gpu_ncsense.py; the CPU run that sets its inputs: tests/test_ncsense_host.py) ------------------------
# one 64 x 64 phantom, 4 coils of synthetic.coil_maps, 12 golden-angle spokes (ramp dcf), the noise level of the single-coil fixture, TV prior
FIXTURE = dict(n=1, h=64, w=64, coils=4, spokes=12, sigma_n=5.0 / 255.0, seed=1234, mu=0.3, sigma_start=50.0 / 255.0, sigma_end=5.0 / 255.0,
               iters=20, cg_iters=8, width=6, tv_scale=1.0, tv_iters=20)
FIXTURE_PSNR = (17.493, 32.399)                                # (x0, final) of the float64 restatement, dB


def fixture_problem():
    """(synthetic.make_problem_ncmc dict by the exact NDFT in float64, plan of the restatement)"""
    from dt4image_restoration_amd import acquisition
    t = FIXTURE
    traj = acquisition.radial_trajectory(t["h"], t["w"], t["spokes"])
    d = synthetic.make_problem_ncmc(t["n"], t["h"], t["w"], t["coils"], traj, dcf=acquisition.radial_dcf(traj, t["h"], t["w"]),
                                    sigma_n=t["sigma_n"], seed=t["seed"])
    return d, NR.plan(t["h"], t["w"], 0, 0, t["width"], traj)


def fixture_schedules():
    t = FIXTURE
    s = np.arange(t["iters"]) / max(t["iters"] - 1, 1)
    return np.full(t["iters"], t["mu"], dtype=np.float32), (t["sigma_start"] * (t["sigma_end"] / t["sigma_start"]) ** s).astype(np.float32)


def admm_tv(d, P, mu, sigma, cg_iters, tv_scale, tv_iters):
    """TV-ADMM on a `synthetic.make_problem_ncmc` dict in float64: x = Re x0, z = x0, u = 0, then per column k of the schedules
    x = TV(Re(z - u), tv_scale * sigma[k], tv_iters) (tests/tv_ref.py) and z, u = `prox_dual` with the model operator, aty = A^H W y.
    Returns (x [N,H,W], psnr of x0 [N], psnr of the final x [N])."""
    import tv_ref
    x0 = tv_ref.cplx(d["x0"])[:, 0]
    y = tv_ref.cplx(d["y0"])
    S = np.asarray(d["sens"]).astype(np.complex128)
    gt = d["gt"][:, 0].astype(np.float64)
    wgt = None if d.get("dcf") is None else d["dcf"].astype(np.float64)
    n = x0.shape[0]
    aty = AH(P, y, S, wgt)
    x, z, u = x0.real.copy(), x0.copy(), np.zeros_like(x0)
    p0 = tv_ref.psnr(x, gt)
    for k in range(len(sigma)):
        lam = np.full(n, float(np.float32(tv_scale)) * float(np.float32(sigma[k])))
        x = tv_ref.tv((z - u).real, lam, tv_iters)
        z, u, _ = prox_dual(P, x, z, u, aty, S, np.full(n, float(np.float32(mu[k]))), cg_iters, wgt)
    return x, p0, tv_ref.psnr(x, gt)
