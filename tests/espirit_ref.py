"""NumPy restatement of the ESPIRiT coil map estimate (include/pnpadmm.h, pnp_espirit_sens) in float64, a float32 restatement of its
per-pixel part that SETS the tolerances of the GPU checks, and the cases of those checks.  TEST INFRASTRUCTURE ONLY.

Per slice, with the centred acs_h x acs_w block B of pnp_estimate_sens, kernel side k, C coils, n = C k^2, D = 2 k - 1:

    A[(wy, wx)][(a, iy, ix)] = B[a][wy + iy][wx + ix]          all (acs_h - k + 1)(acs_w - k + 1) windows, column = a k^2 + iy k + ix
    G = A^H A = V diag(lambda) V^H                             float64
    kept columns {j : lambda_j > sv_thresh^2 max lambda},  P = V_kept V_kept^H
    R[a][b][d] = (1 / k^2) sum over {i - j = d} of conj(P[(a, i), (b, j)])        float64, rounded to complex64 once
    G_q[a][b]  = sum_d R[a][b][d] exp(+2 pi i (dy qy / H + dx qx / W)),  qy = py - H/2, qx = px - W/2
    v <- G_q v / ||G_q v||, `iters` times from l / rss (l, rss: the low-resolution coil images of pnp_estimate_sens and their root-sum-of-squares)
    lambda = Re(v^H G_q v);   p = sum_c conj(v_c) l_c;   S_c = v_c p / |p|   (p == 0: S_c = v_c)
    S_c kept where lambda > float32(crop) and rss > 0 and rss > float32(thresh) smax, else 0

`espirit(..., f32=False)` keeps everything in float64 except the stated roundings of the INPUTS of each stage (the float32 window, R as
complex64, float32 crop / thresh).  `espirit(..., f32=True)` is what a float32 implementation of the per-pixel part can be expected to give:
l from a float32 transform, the twiddles rounded to float32, G_q, the power steps, the quotient and the phase in float32; the Gram matrix, its
eigen-decomposition and R stay float64 as on the device.  The projector comes from numpy.linalg.eigh; `jacobi_kern` restates the device's
solver and the host test shows that both give the same R.

Layouts: y [N,C,H,W] complex; maps [N,C,H,W]; eval [N,H,W]; kern [N,C,C,D,D]; nkept [N].
"""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coilcomp_ref as CC  # noqa: E402
import coilmap_ref as CM  # noqa: E402

from dt4image_restoration_amd.synthetic import ifft2c_np  # noqa: E402

MAX_COILS, MAX_KSIZE, MAX_N = 16, 8, 512
SWEEPS = 40            # the device's cap
LAMBDA_BAND = 1e-4     # pixels with |lambda_ref - crop| <= LAMBDA_BAND may fall on either side of the crop
BAND_SHARE = 1e-3      # ... and are at most this share of a slice
SV_GAP = 1e-6          # no Gram eigenvalue within this (relative) of sv_thresh^2 lambda_0
P_FLOOR = 1e-2         # with thresh = 0 the maps themselves are compared where |p| >= P_FLOOR smax
P_SHARE = 0.15         # ... which may leave out at most this share of a slice


def windows(acs, k):
    return (acs[0] - k + 1) * (acs[1] - k + 1)


def calib_matrix(yn, acs, k):
    """complex128 [windows, C k^2]: the sliding k x k x C windows of the centred block of yn [C,H,W], window-major in row-major order."""
    b = np.asarray(CC.block(np.asarray(yn), acs), dtype=np.complex128)
    c = b.shape[0]
    w = np.lib.stride_tricks.sliding_window_view(b, (k, k), axis=(1, 2))          # [C, wy, wx, iy, ix]
    return np.ascontiguousarray(w.transpose(1, 2, 0, 3, 4)).reshape(-1, c * k * k)


def gram(yn, acs, k):
    """complex128 [n,n]: G = A^H A, exactly Hermitian with a real diagonal."""
    a = calib_matrix(yn, acs, k)
    g = a.conj().T @ a
    g = 0.5 * (g + g.conj().T)
    i = np.arange(g.shape[0])
    g[i, i] = g[i, i].real
    return g


def kern_of(vecs, lam, sv_thresh, c, k):
    """(R complex128 [C,C,D,D] (not yet rounded), nkept) from eigenvectors in the columns of `vecs` and their eigenvalues `lam` (any order)."""
    keep = lam > (sv_thresh * sv_thresh) * lam.max()
    vk = vecs[:, keep]
    p4 = (vk @ vk.conj().T).conj().reshape(c, k, k, c, k, k)                    # conj(P)[a, iy, ix, b, jy, jx]
    d = 2 * k - 1
    r = np.zeros((c, c, d, d), dtype=np.complex128)
    for iy in range(k):
        for jy in range(k):
            for ix in range(k):
                for jx in range(k):
                    r[:, :, iy - jy + k - 1, ix - jx + k - 1] += p4[:, iy, ix, :, jy, jx]
    return r / (k * k), int(keep.sum())


def eigh_kern(g, sv_thresh, c, k):
    lam, vecs = np.linalg.eigh(g)
    return kern_of(vecs, lam, sv_thresh, c, k) + (lam[::-1].copy(),)


def jacobi(g, sweeps=SWEEPS, eps=CC.EPS):
    """The device's solver on one Hermitian matrix, float64: cyclic Jacobi with coilcomp_ref's rotation, round-robin pairs and stop rule,
    each round applied as column and row operations.  Returns (vectors in columns, eigenvalues (unsorted), sweeps run)."""
    n = g.shape[0]
    npad = (n + 1) & ~1
    G = np.zeros((npad, npad), dtype=np.complex128)
    G[:n, :n] = g
    V = np.eye(npad, dtype=np.complex128)
    trace = G.diagonal().real.sum()
    ran = 0
    for _ in range(sweeps):
        if (np.abs(G - np.diag(G.diagonal())) ** 2).sum() <= (eps * trace) ** 2:
            break
        ran += 1
        for r in range(npad - 1):
            p, q = CC.pairs(r, npad)
            t, cs, sg, ab, on = CC.rotation(G[p, p].real, G[q, q].real, G[p, q])
            dp, dq = G[p, p].real - t * ab, G[q, q].real + t * ab
            gp, gq = G[:, p].copy(), G[:, q].copy()                              # G J
            G[:, p], G[:, q] = gp * cs - gq * sg.conj(), gp * sg + gq * cs
            gp, gq = G[p, :].copy(), G[q, :].copy()                              # J^H (G J)
            G[p, :], G[q, :] = cs[:, None] * gp - sg[:, None] * gq, sg.conj()[:, None] * gp + cs[:, None] * gq
            G = 0.5 * (G + G.conj().T)
            G[p, q], G[q, p] = 0.0, 0.0
            G[p, p], G[q, q] = np.where(on, dp, G[p, p].real), np.where(on, dq, G[q, q].real)
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = vp * cs - vq * sg.conj(), vp * sg + vq * cs
    return V[:n, :n], G.diagonal().real[:n].copy(), ran


def jacobi_kern(g, sv_thresh, c, k):
    """(R, nkept, eigenvalues, sweeps) from the restated cyclic Jacobi solver of the device."""
    vecs, lam, ran = jacobi(g)
    return kern_of(vecs, lam, sv_thresh, c, k) + (lam, ran)


def round_c64(a):
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def twiddles(length, k, dtype=np.complex128):
    """[length, D]: exp(+2 pi i d q / length), q = p - length/2, d = -(k-1) .. k-1; the argument reduced exactly in integers."""
    q = np.arange(length) - length // 2
    d = np.arange(-(k - 1), k)
    m = np.mod(np.outer(q, d), length)
    return np.exp(2j * math.pi * m / length).astype(dtype)


def pixel_matrices(r, h, w, k, f32=False):
    """G_q [C,C,H,W] from R [C,C,D,D] (complex64 values), evaluated separably: d_y first."""
    ct = np.complex64 if f32 else np.complex128
    t = np.einsum("abyx,py->abpx", r.astype(ct), twiddles(h, k, ct))
    return np.einsum("abpx,qx->abpq", t, twiddles(w, k, ct))


def lowres(y, acs, kind, f32=False):
    """(l [N,C,H,W], rss [N,H,W], smax [N]) of pnp_estimate_sens: float64, or float32 as coilmap_ref.estimate_f32 forms them."""
    n, c, h, w = y.shape
    win = CM.window(h, w, acs[0], acs[1], kind)
    if not f32:
        l = ifft2c_np(win * np.asarray(y, dtype=np.complex128))
        rss = np.sqrt((l.real ** 2 + l.imag ** 2).sum(axis=1))
        return l, rss, rss.reshape(n, -1).max(axis=1)
    import torch
    yt = torch.from_numpy(np.array(y, dtype=np.complex64))
    kk = torch.view_as_complex(torch.view_as_real(yt) * torch.from_numpy(win).float()[..., None])
    l = torch.fft.fftshift(torch.fft.ifftn(torch.fft.ifftshift(kk, dim=(-2, -1)), dim=(-2, -1), norm="ortho"), dim=(-2, -1)).numpy()
    acc = np.zeros((n, h, w))
    for i in range(c):
        acc = acc + (l[:, i].real.astype(np.float64) ** 2 + l[:, i].imag.astype(np.float64) ** 2)
    rss = np.sqrt(acc).astype(np.float32)
    return l, rss, rss.reshape(n, -1).max(axis=1)


def power(gq, v0, iters):
    """`iters` steps v <- G_q v / ||G_q v|| (a zero product gives v = 0), then lambda = Re(v^H G_q v): (v [C,H,W], lambda [H,W])."""
    v = v0
    rt = v0.real.dtype
    for _ in range(iters):
        wv = np.einsum("abpq,bpq->apq", gq, v)
        nrm = np.sqrt((wv.real ** 2 + wv.imag ** 2).sum(axis=0)).astype(rt)
        v = np.where(nrm > 0, wv / np.where(nrm > 0, nrm, 1), 0).astype(v0.dtype)
    wv = np.einsum("abpq,bpq->apq", gq, v)
    return v, (v.conj() * wv).sum(axis=0).real.astype(rt)


def espirit(y, acs, k=6, sv_thresh=0.02, crop=0.9, iters=16, kind="hann", thresh=0.0, f32=False, kern=None):
    """dict(maps, eval, kern (complex64 values), nkept, kept, pabs (|p| [N,H,W]), rss, smax, lam (Gram eigenvalues, descending, [N,n]), gq).
    kern: reuse the (kern, nkept, lam) of an earlier call on the same data (they do not depend on iters, crop, thresh or f32)."""
    y = np.asarray(y)
    n, c, h, w = y.shape
    l, rss, smax = lowres(y, acs, kind, f32)
    ct, rt = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    out = dict(maps=np.zeros((n, c, h, w), dtype=ct), eval=np.zeros((n, h, w), dtype=rt), kept=np.zeros((n, h, w), dtype=bool),
               pabs=np.zeros((n, h, w)), rss=rss, smax=smax, kern=[], nkept=[], lam=[], gq=[])
    for i in range(n):
        if kern is None:
            r, nk, lam = eigh_kern(gram(y[i], acs, k), sv_thresh, c, k)
            r = round_c64(r)
        else:
            r, nk, lam = kern[0][i], kern[1][i], kern[2][i]
        gq = pixel_matrices(r, h, w, k, f32)
        ok = rss[i] > 0
        v0 = np.where(ok, l[i] / np.where(ok, rss[i], 1), 0).astype(ct)
        v, lam_q = power(gq, v0, iters)
        p = (v.conj() * l[i].astype(ct)).sum(axis=0)
        pa = np.hypot(p.real, p.imag)
        phi = np.where(pa > 0, p / np.where(pa > 0, pa, 1), 1).astype(ct)
        keep = (lam_q > rt(np.float32(crop))) & ok & (rss[i] > rt(np.float32(thresh)) * smax[i])
        out["maps"][i] = np.where(keep, v * phi, 0)
        out["eval"][i], out["kept"][i], out["pabs"][i] = lam_q, keep, pa
        out["kern"].append(r); out["nkept"].append(nk); out["lam"].append(lam); out["gq"].append(gq)
    out["kern"], out["nkept"], out["lam"] = np.stack(out["kern"]), np.array(out["nkept"]), np.stack(out["lam"])
    return out


def eigh_maps(gq, l):
    """The dominant eigenvector of every G_q by numpy.linalg.eigh, with the phase rule of the estimate: (maps [C,H,W], lambda [H,W])."""
    lam, vec = np.linalg.eigh(np.ascontiguousarray(gq.transpose(2, 3, 0, 1)))
    v = vec[..., -1].transpose(2, 0, 1)
    p = (v.conj() * l).sum(axis=0)
    pa = np.abs(p)
    return v * np.where(pa > 0, p / np.where(pa > 0, pa, 1), 1), lam[..., -1]


def sv_gap(lam, sv_thresh):
    """The smallest relative distance of a Gram eigenvalue from the cut sv_thresh^2 lambda_0."""
    cut = sv_thresh * sv_thresh * lam.max(axis=-1, keepdims=True)
    return float((np.abs(lam - cut) / cut).min())


def band(ref, crop, thresh):
    """bool [N,H,W]: the pixels that may fall on either side of a cut (|lambda - crop| <= LAMBDA_BAND, or rss near the threshold as in
    coilmap_ref)."""
    s3 = ref["smax"][:, None, None].astype(np.float64)
    near = np.abs(ref["eval"].astype(np.float64) - np.float64(np.float32(crop))) <= LAMBDA_BAND
    return near | (np.abs(ref["rss"].astype(np.float64) - np.float64(np.float32(thresh)) * s3) <= CM.NEAR_CUT * s3)


def compare(maps, ev, kern, nkept, ref, crop, thresh):
    """Figures of one estimate against `ref = espirit(...)` in float64 (see the GPU test's header)."""
    maps, ev = np.asarray(maps).astype(np.complex128), np.asarray(ev).astype(np.float64)
    n = maps.shape[0]
    near = band(ref, crop, thresh)
    use, kept64 = ~near, ref["kept"]
    power_ = (np.abs(maps) ** 2).sum(axis=1)
    kept = power_ > 0.5
    both = use & kept64
    s3 = ref["smax"][:, None, None]
    prod = lambda m: m[:, :, None] * m[:, None, :].conj()
    dprod = np.abs(prod(maps) - prod(ref["maps"])).max(axis=(1, 2))
    dmap = np.abs(maps - ref["maps"]).max(axis=1)
    strong = kept64 & kept & (ref["pabs"] >= P_FLOOR * s3)
    return dict(nkept=bool(np.array_equal(np.asarray(nkept), ref["nkept"])),
                kern=float(np.abs(np.asarray(kern).astype(np.complex128) - ref["kern"]).max() / np.abs(ref["kern"]).max()),
                eval=float(np.abs(ev - ref["eval"])[use].max()),
                flips=int(((kept != kept64) & use).sum()),
                off_zero=bool(not maps[np.broadcast_to((use & ~kept64)[:, None], maps.shape)].any()),
                unit=float(np.abs(power_ - 1.0)[both].max()) if both.any() else 0.0,
                prod=float(dprod[kept64 & kept].max()) if (kept64 & kept).any() else 0.0,
                maps_all=float(dmap[kept64 & kept].max()) if (kept64 & kept).any() else 0.0,
                maps=float(dmap[strong].max()) if strong.any() else 0.0,
                left_out=float((kept64 & ~(ref["pabs"] >= P_FLOOR * s3)).reshape(n, -1).mean(axis=1).max()),
                near=float(near.reshape(n, -1).mean(axis=1).max()),
                finite=bool(np.isfinite(maps.view(np.float64)).all() and np.isfinite(ev).all()))


# ---- the cases of the GPU checks (shared with the CPU measurement that sets their bounds) -------------------------------------------------

SV, CROP, ITERS = 0.02, 0.9, 16
#        N, C, H,  W,   block,    k, sigma_n
CASES = ((3, 4, 64, 64, (24, 24), 4, 1.0 / 255.0),          # n = 64
         (1, 5, 80, 64, (20, 24), 4, 1.0 / 255.0),          # n = 80: an odd coil count, a 2^a 5^b side, just past 64
         (2, 8, 64, 80, (24, 24), 5, 1.0 / 255.0),          # n = 200: odd k
         (2, 8, 128, 128, (24, 24), 6, 10.0 / 255.0),       # n = 288: the default configuration
         (1, 12, 64, 64, (24, 24), 4, 1.0 / 255.0))         # n = 192: more than 8 coils (the 16-coil instantiation of the pixel kernel)
THRESHES = (0.05, 0.0)


@functools.lru_cache(maxsize=None)
def case_y(n, c, h, w, sigma_n, seed=11, mask_key=None):
    """complex64 [n,c,h,w]: noisy multi-coil k-space of `make_problem_mc` (all-ones mask unless mask_key = (kind, accel))."""
    from dt4image_restoration_amd import acquisition, synthetic
    mask = np.ones((h, w), dtype=bool) if mask_key is None else acquisition.make_mask(h, w, mask_key[1], mask_key[0])
    d = synthetic.make_problem_mc(n, h, w, c, sigma_n=sigma_n, seed=seed, mask=mask)
    y = (d["y0"][..., 0] + 1j * d["y0"][..., 1]).astype(np.complex64)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def case_ref(i, thresh=0.05, f32=False):
    """(y complex64, ref) of CASES[i] with the default parameters, computed once; the Gram part is shared between the variants."""
    n, c, h, w, acs, k, sigma_n = CASES[i]
    y = case_y(n, c, h, w, sigma_n, 11 + i)
    base = None if (thresh, f32) == (THRESHES[0], False) else case_ref(i)[1]
    kern = None if base is None else (base["kern"], base["nkept"], base["lam"])
    ref = espirit(y, acs, k, SV, CROP, ITERS, "hann", thresh, f32=f32, kern=kern)
    ref.pop("gq")
    return y, ref


# ---- the chain check: ESPIRiT maps, then the multi-coil data fidelity -----------------------------------------------------------------------

CHAIN = dict(n=2, c=4, h=64, w=64, accel=4, mu=0.3, K=8, ksize=2, thresh=0.05, cal=(24, 24))


@functools.lru_cache(maxsize=None)
def chain_problem():
    """dict(y complex64 [n,c,h,w], mask, acs (the mask's block cropped to `cal`), x0 complex64 [n,h,w]) of `make_problem_mc` under
    cartesian_mask(64, 64, 4)."""
    from dt4image_restoration_amd import acquisition, synthetic
    t = CHAIN
    mask = acquisition.cartesian_mask(t["h"], t["w"], t["accel"])
    d = synthetic.make_problem_mc(t["n"], t["h"], t["w"], t["c"], seed=11, mask=mask)
    y = (d["y0"][..., 0] + 1j * d["y0"][..., 1]).astype(np.complex64)
    x0 = (d["x0"][:, 0, ..., 0] + 1j * d["x0"][:, 0, ..., 1]).astype(np.complex64)
    acs = tuple(min(a, c) for a, c in zip(acquisition.acs_block(mask), t["cal"]))
    return dict(y=y, mask=mask, acs=acs, x0=x0)


@functools.lru_cache(maxsize=None)
def chain_reference(f32=False):
    """(ref = espirit(...), z, u, cg_res) of one prox_dual from (x, z, u) = (Re x0, x0, 0) with the estimate's maps: float64 with
    sense_ref.prox_dual, or the float32 restatement (espirit f32, coilcomp_ref.aty_f32, sense_ref.cg_solve_f32)."""
    import sense_ref as SR
    q, t = chain_problem(), CHAIN
    ref = espirit(q["y"], q["acs"], t["ksize"], SV, CROP, ITERS, "hann", t["thresh"], f32=f32)
    ref.pop("gq")
    x, z0, u0 = q["x0"].real, q["x0"], np.zeros_like(q["x0"])
    if not f32:
        mu = np.full(t["n"], np.float64(np.float32(t["mu"])))
        z, u, res = SR.prox_dual(x.astype(np.float64), z0.astype(np.complex128), u0.astype(np.complex128), q["y"].astype(np.complex128),
                                 ref["maps"], q["mask"], mu, t["K"])
        return ref, z, u, res
    aty = CC.aty_f32(q["y"], ref["maps"], q["mask"])
    z, res, _, _ = SR.cg_solve_f32(z0, x, u0, aty, ref["maps"], q["mask"], np.full(t["n"], np.float32(t["mu"])), t["K"])
    return ref, z, u0 + x - z, res
