"""Float64 restatement of the non-Cartesian stage (include/pnpadmm.h, "non-Cartesian sampling"): the plan (footprint starts, kernel
weights, deconvolution factors), the forward / adjoint MODELS built from the plan's float32-rounded weights and factors but evaluated in
float64, the exact NDFT, the K-step CG of the data-fidelity stage, and the cases the host and GPU tests share.

The plan's float64 expressions are written operation by operation as csrc/nufft_plan.hip writes them (math.exp / math.sqrt are the C
library's, as std::exp / std::sqrt there), so both round the same float64 values to float32: tests/nufft_plan_host.cpp compares bits."""
import math

import numpy as np

from dt4image_restoration_amd.weights import hash_uniform

SIDES = (16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024)
QUAD_NODES = 128
TILE = 16

# (N, H, W, gh, gw, J); the first four on 13 golden-angle spokes of 2 max(H, W) samples (r = -0.5 included: it wraps), the fifth on 300
# hash-drawn samples plus the corners, the centre, a coordinate one grid ulp inside the edge and a duplicated pair (wrap, ties, duplicates)
CASES = ((2, 16, 16, 32, 32, 6), (1, 64, 64, 80, 80, 6), (2, 32, 16, 64, 32, 4), (1, 64, 32, 80, 64, 8), (3, 16, 16, 32, 32, 8))
SPOKES = 13


def default_grid(side):
    for g in SIDES:
        if 4 * g >= 5 * side:
            return g
    return 0


def radial(h, w, spokes, readout=None, golden=True):
    """[spokes * R, 2] float64 (ky, kx): spoke s at angle s pi (sqrt 5 - 1) / 2 (or s pi / spokes), r_j = (j - R/2) / R"""
    R = 2 * max(h, w) if readout is None else int(readout)
    r = (np.arange(R, dtype=np.float64) - R / 2) / R
    out = np.empty((spokes, R, 2))
    for s in range(spokes):
        a = s * math.pi * (math.sqrt(5.0) - 1.0) / 2.0 if golden else s * math.pi / spokes
        out[s, :, 0] = r * math.sin(a)
        out[s, :, 1] = r * math.cos(a)
    return out.reshape(-1, 2)


def case_traj(i):
    n, h, w, gh, gw, j = CASES[i]
    if i < 4:
        return radial(h, w, SPOKES)
    u = hash_uniform(515, 61, 600).astype(np.float64).reshape(300, 2) * 0.5           # [-0.5, 0.5)
    extra = np.array([[-0.5, -0.5], [0.0, 0.0], [0.5, 0.5], [0.5 - 2.0 ** -20, 0.0], [0.123, -0.321], [0.123, -0.321]])
    return np.concatenate([u, extra])


def case_image(i, seed=0):
    """complex128 [N,H,W], Gaussian: energy up to the image edge, the worst case for the kernel's aliasing error"""
    n, h, w = CASES[i][:3]
    rng = np.random.default_rng(1000 + 17 * i + seed)
    return rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w))


def case_samples(i, m, seed=0):
    n = CASES[i][0]
    rng = np.random.default_rng(2000 + 17 * i + seed)
    return rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
def beta_of(J, g, side):
    if g == 2 * side:
        return 2.30 * J
    return 0.97 * math.pi * J * (1.0 - side / (2.0 * g))


def phi(t, J, beta):
    z = 2.0 * t / J
    if not abs(z) < 1.0:
        return 0.0
    a = 1.0 - z * z
    return math.exp(beta * (math.sqrt(a) - 1.0))


def phihat(q, J, g, beta, nodes=QUAD_NODES):
    """2 int_0^{J/2} phi(t) cos(2 pi q t / g) dt, Gauss-Legendre; q: array"""
    x, wq = np.polynomial.legendre.leggauss(nodes)
    half = 0.25 * J
    t = half * (x + 1.0)
    ph = np.array([phi(tt, J, beta) for tt in t])
    q = np.asarray(q, dtype=np.float64)
    return 2.0 * half * (wq * ph * np.cos(2.0 * math.pi * q[..., None] * t / g)).sum(axis=-1)


def plan(h, w, gh, gw, J, traj, nodes=QUAD_NODES):
    traj = np.asarray(traj, dtype=np.float64)
    m = traj.shape[0]
    gh = gh or default_grid(h)
    gw = gw or default_grid(w)
    i0 = np.empty((2, m), dtype=np.int64)
    wts = np.empty((2 * J, m), dtype=np.float32)
    for a, (g, side) in enumerate(((gh, h), (gw, w))):
        beta = beta_of(J, g, side)
        for s in range(m):
            kg = float(traj[s, a]) * g
            u = kg + 0.5 * g
            i = int(math.ceil(u - 0.5 * J))
            i0[a, s] = i
            for j in range(J):
                wts[a * J + j, s] = np.float32(phi(u - float(i + j), J, beta))
    c = []
    for g, side in ((gh, h), (gw, w)):
        beta = beta_of(J, g, side)
        c.append((math.sqrt(g / side) / phihat(np.arange(side) - side // 2, J, g, beta, nodes)).astype(np.float32))
    return dict(h=h, w=w, gh=gh, gw=gw, J=J, m=m, i0=i0, wts=wts, cy=c[0], cx=c[1])


def tiles_of(P, s):
    """the set of (tile row, tile column) the periodic footprint of sample s meets"""
    J = P["J"]
    ty = {((int(P["i0"][0, s]) + j) % P["gh"]) // TILE for j in range(J)}
    tx = {((int(P["i0"][1, s]) + j) % P["gw"]) // TILE for j in range(J)}
    return {(a, b) for a in ty for b in tx}


def chain_lengths(P):
    """int [gh, gw]: samples whose footprint contains each grid point (the length of its fma chain)"""
    J = P["J"]
    cnt = np.zeros((P["gh"], P["gw"]), dtype=np.int64)
    rows = (P["i0"][0][:, None] + np.arange(J)) % P["gh"]
    cols = (P["i0"][1][:, None] + np.arange(J)) % P["gw"]
    for a in range(J):
        for b in range(J):
            np.add.at(cnt, (rows[:, a], cols[:, b]), 1)
    return cnt


# ---- the models: the plan's float32 numbers, float64 arithmetic --------------------------------------------------------------------------------
def fft2c(a):
    return np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def ifft2c(a):
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def _factors(P):
    return (P["cy"][:, None] * P["cx"][None, :]).astype(np.float64)             # the float32 product the kernels form


def _foot(P):
    J = P["J"]
    rows = (P["i0"][0][:, None] + np.arange(J)) % P["gh"]
    cols = (P["i0"][1][:, None] + np.arange(J)) % P["gw"]
    return rows, cols, P["wts"][:J].T.astype(np.float64), P["wts"][J:].T.astype(np.float64)      # [M, J] each


def grid_of(P, x):
    """the padded, deconvolved and transformed grid [N, gh, gw] of the forward"""
    x = np.asarray(x, dtype=np.complex128).reshape(-1, P["h"], P["w"])
    g = np.zeros((x.shape[0], P["gh"], P["gw"]), dtype=np.complex128)
    oy, ox = P["gh"] // 2 - P["h"] // 2, P["gw"] // 2 - P["w"] // 2
    g[:, oy:oy + P["h"], ox:ox + P["w"]] = x * _factors(P)
    return fft2c(g)


def gather(P, X, absolute=False):
    rows, cols, wy, wx = _foot(P)
    X = np.abs(X) if absolute else X
    out = np.zeros((X.shape[0], P["m"]), dtype=X.dtype)
    for a in range(P["J"]):
        for b in range(P["J"]):
            out += (wy[:, a] * wx[:, b]) * X[:, rows[:, a], cols[:, b]]
    return out


def forward(P, x):
    return gather(P, grid_of(P, x))


def spread(P, y, wgt=None, absolute=False):
    rows, cols, wy, wx = _foot(P)
    y = np.asarray(y, dtype=np.complex128).reshape(-1, P["m"])
    v = y if wgt is None else y * np.asarray(wgt, dtype=np.float64)
    v = np.abs(v) if absolute else v
    g = np.zeros((y.shape[0], P["gh"], P["gw"]), dtype=v.dtype)
    for n in range(y.shape[0]):
        for a in range(P["J"]):
            for b in range(P["J"]):
                np.add.at(g[n], (rows[:, a], cols[:, b]), v[n] * wy[:, a] * wx[:, b])
    return g


def adjoint(P, y, wgt=None):
    g = ifft2c(spread(P, y, wgt))
    oy, ox = P["gh"] // 2 - P["h"] // 2, P["gw"] // 2 - P["w"] // 2
    return g[:, oy:oy + P["h"], ox:ox + P["w"]] * _factors(P)


def ndft(traj, x):
    """the exact operator: (A x)_m = (1 / sqrt(H W)) sum_q x[q] exp(-2 pi i (ky qy + kx qx))"""
    x = np.asarray(x, dtype=np.complex128)
    h, w = x.shape[-2:]
    x = x.reshape(-1, h, w)
    traj = np.asarray(traj, dtype=np.float64)
    ey = np.exp(-2j * math.pi * traj[:, 0:1] * (np.arange(h) - h // 2))
    ex = np.exp(-2j * math.pi * traj[:, 1:2] * (np.arange(w) - w // 2))
    return np.einsum("my,nyx,mx->nm", ey, x, ex, optimize=True) / math.sqrt(h * w)


def ndft_adjoint(traj, y, h, w, wgt=None):
    y = np.asarray(y, dtype=np.complex128)
    y = y if wgt is None else y * np.asarray(wgt, dtype=np.float64)
    traj = np.asarray(traj, dtype=np.float64)
    ey = np.exp(2j * math.pi * traj[:, 0:1] * (np.arange(h) - h // 2))
    ex = np.exp(2j * math.pi * traj[:, 1:2] * (np.arange(w) - w // 2))
    return np.einsum("my,nm,mx->nyx", ey, y.reshape(-1, traj.shape[0]), ex, optimize=True) / math.sqrt(h * w)


def op_norm(P, iters=30, wgt=None):
    """||A|| of the model by power iteration on A^H A"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, P["h"], P["w"])) + 1j * rng.standard_normal((1, P["h"], P["w"]))
    s = 0.0
    for _ in range(iters):
        x /= np.linalg.norm(x)
        x = adjoint(P, forward(P, x))
        s = math.sqrt(np.linalg.norm(x))
    return s


# ---- the data-fidelity stage -----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a.real * b.real + a.imag * b.imag).reshape(a.shape[0], -1).sum(axis=1)


def normal(P, p, mu, wgt=None):
    return adjoint(P, forward(P, p), wgt) + np.asarray(mu, dtype=np.float64).reshape(-1, 1, 1) * p


def cg_solve(P, z0, x, u, aty, mu, iters, wgt=None):
    """the multi-coil section's K-step CG on Nop(p) = A^H W A p + mu p; returns (z, cg_res [N])"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    m3 = mu.reshape(-1, 1, 1)
    b = aty + m3 * (x + u)
    z = np.array(z0, dtype=np.complex128)
    r = b - normal(P, z, mu, wgt)
    p = r.copy()
    rs, bb = _dot(r, r), _dot(b, b)
    for _ in range(iters):
        q = normal(P, p, mu, wgt)
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


def prox_dual(P, x, z, u, aty, mu, iters, wgt=None):
    zn, res = cg_solve(P, z, x, u, aty, mu, iters, wgt)
    return zn, u + x - zn, res


def dc_misfit(P, x, y, wgt=None):
    d = np.abs(forward(P, x) - y) ** 2
    d = d if wgt is None else d * np.asarray(wgt, dtype=np.float64)
    return np.sqrt(d.sum(axis=1))


def mask_traj(mask):
    """the Cartesian-bin trajectory of a centred mask: bin (j, l) -> ((j - H/2) / H, (l - W/2) / W), row-major over the sampled bins"""
    mask = np.asarray(mask).astype(bool)
    h, w = mask.shape
    j, l = np.nonzero(mask)
    return np.stack([(j - h // 2) / h, (l - w // 2) / w], axis=1).astype(np.float64), (j, l)


# ---- the end-to-end fixture (tests/test_gpu_nufft.py; the CPU run that sets its inputs: tests/test_nufft_host.py) -----------------------------
# one 64 x 64 phantom, golden radial, the noise level of the GRAPPA fixture, TV prior, a fixed (mu, sigma_d) schedule
FIXTURE = dict(n=1, h=64, w=64, spokes=24, sigma_n=5.0 / 255.0, seed=1234, mu=0.3, sigma_start=50.0 / 255.0, sigma_end=5.0 / 255.0, iters=20,
               cg_iters=8, width=6, tv_scale=1.0, tv_iters=20)
FIXTURE_PSNR = (16.572, 36.812)                                 # (x0, final) of the float64 restatement, dB


def fixture_problem():
    """(make_problem_nc dict by the exact NDFT in float64, plan of the restatement)"""
    from dt4image_restoration_amd import acquisition, synthetic
    t = FIXTURE
    traj = acquisition.radial_trajectory(t["h"], t["w"], t["spokes"])
    d = synthetic.make_problem_nc(t["n"], t["h"], t["w"], traj, dcf=acquisition.radial_dcf(traj, t["h"], t["w"]), sigma_n=t["sigma_n"], seed=t["seed"])
    return d, plan(t["h"], t["w"], 0, 0, t["width"], traj)


def fixture_schedules():
    t = FIXTURE
    s = np.arange(t["iters"]) / max(t["iters"] - 1, 1)
    return np.full(t["iters"], t["mu"], dtype=np.float32), (t["sigma_start"] * (t["sigma_end"] / t["sigma_start"]) ** s).astype(np.float32)


def admm_tv_nc(d, P, mu, sigma, cg_iters, tv_scale, tv_iters):
    """TV-ADMM on a `synthetic.make_problem_nc` dict in float64: x = Re x0, z = x0, u = 0, then per column k of the schedules
    x = TV(Re(z - u), tv_scale * sigma[k], tv_iters) (tests/tv_ref.py) and z, u = `prox_dual` with the model operator, aty = A^H W y.
    Returns (x [N,H,W], psnr of x0 [N], psnr of the final x [N])."""
    import tv_ref
    x0 = tv_ref.cplx(d["x0"])[:, 0]
    y = tv_ref.cplx(d["y0"])[:, 0]
    gt = d["gt"][:, 0].astype(np.float64)
    wgt = None if d.get("dcf") is None else d["dcf"].astype(np.float64)
    n = x0.shape[0]
    aty = adjoint(P, y, wgt)
    x, z, u = x0.real.copy(), x0.copy(), np.zeros_like(x0)
    p0 = tv_ref.psnr(x, gt)
    for k in range(len(sigma)):
        lam = np.full(n, float(np.float32(tv_scale)) * float(np.float32(sigma[k])))
        x = tv_ref.tv((z - u).real, lam, tv_iters)
        z, u, _ = prox_dual(P, x, z, u, aty, np.full(n, float(np.float32(mu[k]))), cg_iters, wgt)
    return x, p0, tv_ref.psnr(x, gt)
