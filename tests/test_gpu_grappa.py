"""GRAPPA (pnp_grappa_weights, pnp_grappa_apply) on the MI355X, through the C ABI, against the float64 restatement of tests/grappa_ref.py.
Every caller-owned buffer of the two entry points' own tests comes from tests/guard_bands.py (`weights` / `fill` below: the outputs between
bands of a fixed pattern, the inputs frozen at their bits); the end-to-end and command-line tests go through the Python functions
(`acquisition.grappa`, `PnPEngine.grappa_*`), which allocate plain torch tensors themselves: plumbing around calls the guarded tests cover.
Every figure is printed before it is asserted.

The cases (grappa_ref.CASES) are (N, C, H, W, R, offset, by x bx, acs_w) with acs_h = H; the data is `synthetic.make_problem_mc` on the
case's comb with noise 2/255, and lam = 1e-3 (grappa_ref.case_data).

BOUNDS (none of them measured on the device).
  gram       bit for bit: the terms are exact float64 products and the order of the additions is fixed (grappa_ref.gram_one).
  weights    |wts - X_ref| <= (2^-23 + 16 ns kappa 2^-53) max |X_ref|: one complex64 rounding plus the forward error of a float64 Cholesky
             solve, kappa = numpy's condition number of the regularised Gram matrix.  The test asserts kappa ns <= 3e7 for its inputs, so
             the second term stays below 2^-24 x 0.9 (measured on the CPU: kappa ns <= 2e6 on all six cases).
  geometry   bit for bit: a weight 1 + 0i at one (t, s) copies that source plane, shifted (a -0 component comes out as +0).
  apply      |out - float64| <= gamma_{4 ns} sum_s (|a.re| + |a.im|)(|x.re| + |x.im|), gamma_k = k 2^-24 / (1 - k 2^-24), bin by bin.
  end to end grappa_ref.FIXTURE (1 x 64 x 64, 8 coils, R 2, 5 x 4 kernel, 12 centre columns, noise 5/255, lam 1e-2, phantom seed 7).  Measured
             on the CPU in float64: 32.514 dB map-combined from the GRAPPA-filled k-space, 30.740 dB for ATy0: +1.774 dB (a condition on the
             input, >= 1 dB; it depends on the phantom).  The device's PSNR is asserted within 0.01 dB of the reference's.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402
import grappa_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = range(len(R.CASES))


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


def weights(e, y, acs_h, acs_w, r, by, bx, lam=R.CASE_LAM, with_gram=True):
    """pnp_grappa_weights on guarded buffers: y complex64 ndarray [N,C,H,W] -> (wts [N,nt,ns], info [N], gram [N,ns,ns+nt] or None)"""
    n, c = y.shape[:2]
    ns, nt = R.sizes(c, r, by, bx)
    x = g_in(y, torch.complex64, "y0")
    wts = G.guarded((n, nt, ns), torch.complex64, DEV, name="wts")
    info = G.guarded((n,), torch.int32, DEV, name="info")
    gram = G.guarded((n, ns, ns + nt), torch.complex128, DEV, name="gram") if with_gram else None
    with G.watch(outputs={"wts": wts, "info": info, "gram": gram}, inputs={"y0": x}):
        _lib.check(e.lib.pnp_grappa_weights(e._h, x.data_ptr(), c, acs_h, acs_w, r, by, bx, float(lam), 0, wts.data_ptr(), info.data_ptr(),
                                            gram.data_ptr() if with_gram else None, _stream()), "pnp_grappa_weights")
    return wts, info, gram


def fill(e, y, mask, wts, r, off, by, bx):
    """pnp_grappa_apply on guarded buffers: y [N,C,H,W], mask bool [H,W] or [N,H,W], wts complex64 [nt,ns] or [N,nt,ns] -> out tensor"""
    n, c, h, w = y.shape
    ns, nt = R.sizes(c, r, by, bx)
    wts = np.asarray(wts, dtype=np.complex64)
    wn = 1 if wts.ndim == 2 else wts.shape[0]
    mask = np.asarray(mask)
    mn = 1 if mask.ndim == 2 else mask.shape[0]
    x = g_in(y, torch.complex64, "y0")
    m = g_in(mask.astype(np.uint8).reshape(mn, h, w), torch.uint8, "mask")
    wt = g_in(wts.reshape(wn, nt, ns), torch.complex64, "wts")
    out = G.guarded((n, c, h, w), torch.complex64, DEV, name="out")
    with G.watch(outputs={"out": out}, inputs={"y0": x, "mask": m, "wts": wt}):
        _lib.check(e.lib.pnp_grappa_apply(e._h, x.data_ptr(), c, m.data_ptr(), mn, r, off, by, bx, wt.data_ptr(), wn, out.data_ptr(), _stream()),
                   "pnp_grappa_apply")
    return out


_CACHE = {}


def case(i):
    """The case's data, reference Gram, float64 weights and condition numbers, computed once and left unchanged"""
    if i not in _CACHE:
        n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
        y, mask = R.case_data(i)
        gram = R.gram(y, h, acs_w, r, by, bx)
        sol = [R.weights_one(m, R.CASE_LAM) for m in gram]
        d = dict(y=y, mask=mask, gram=gram, wts=np.stack([s[0] for s in sol]), kappa=[s[1] for s in sol])
        _CACHE[i] = d
    return _CACHE[i]


def both(e, i, y=None, mask=None):
    """weights then apply of case i (or of other data of its shape) on the device: (wts, info, out)"""
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    y = case(i)["y"] if y is None else y
    mask = case(i)["mask"] if mask is None else mask
    wts, info, _ = weights(e, y, h, acs_w, r, by, bx, with_gram=False)
    return wts, info, fill(e, y, mask, wts.cpu().numpy(), r, off, by, bx)


# ---- 1, 2: calibration -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", ALL)
def test_gram_is_the_reference_bit_for_bit_and_the_weights_are_within_the_solve_bound(i):
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    ns, nt = R.sizes(c, r, by, bx)
    d = case(i)
    e = _engine(n, h, w)
    wts, info, gram = weights(e, d["y"], h, acs_w, r, by, bx)
    assert info.tolist() == [0] * n
    g = gram.cpu().numpy()
    diff = int((g.view(np.int64) != d["gram"].view(np.int64)).sum())
    print(f"case {i} {R.CASES[i]}: ns {ns} nt {nt}, gram words that differ {diff}")
    assert g.shape == (n, ns, ns + nt) and diff == 0
    for k in range(n):
        kappa, ref = d["kappa"][k], d["wts"][k]
        assert kappa * ns <= 3e7
        bound = (2.0 ** -23 + 16 * ns * kappa * 2.0 ** -53) * np.abs(ref).max()
        err = float(np.abs(_np(wts[k]) - ref).max())
        print(f"  slice {k}: kappa {kappa:.3e} kappa ns {kappa * ns:.3e}  max |wts - X_ref| {err:.3e} / {bound:.3e}  max |X_ref| {np.abs(ref).max():.3e}")
        assert err <= bound
    again, _, none = weights(e, d["y"], h, acs_w, r, by, bx, with_gram=False)
    assert none is None and _same(again, wts)                                    # gram = NULL changes nothing


# ---- 3: the apply kernel's geometry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", ALL)
def test_a_one_hot_weight_copies_its_source_plane_shifted_bit_for_bit(i):
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    ns, nt = R.sizes(c, r, by, bx)
    e = _engine(n, h, w)
    rng = np.random.default_rng(100 + i)
    y = (rng.standard_normal((n, c, h, w)) + 1j * rng.standard_normal((n, c, h, w))).astype(np.complex64)
    y[0, 0, 0, off] = np.complex64(complex(-0.0, 1.0))                           # a -0 component comes out as +0
    yt = torch.from_numpy(y).to(DEV)
    none = np.zeros((h, w), dtype=bool)                                          # nothing measured beside the comb: every other bin is synthesised
    cs, ct = 0, c - 1                                                            # source coil != target coil
    comb = torch.arange(off, w, r, device=DEV)
    for ti in range(by):
        for tj in range(bx):
            k = 1 + (ti * bx + tj) % (r - 1)
            hot = np.zeros((nt, ns), dtype=np.complex64)
            hot[ct * (r - 1) + (k - 1), (cs * by + ti) * bx + tj] = 1
            out = fill(e, y, none, hot, r, off, by, bx)
            # out[y][xa + k] = src[y + ti - by/2][xa + (tj - (bx/2 - 1)) R], indices periodic
            want = torch.roll(yt[:, cs], shifts=(-(ti - by // 2), k - (tj - (bx // 2 - 1)) * r), dims=(1, 2)) + 0.0
            cols = (comb + k) % w
            assert _same(out[:, ct][:, :, cols], want[:, :, cols]), (ti, tj, k)
            # rows 0 and H - 1 and the first and last comb columns, spelled out: the wrap in both axes
            for row in (0, h - 1):
                for q in (0, w // r - 1):
                    xa = off + q * r
                    src = yt[0, cs, (row + ti - by // 2) % h, (xa + (tj - (bx // 2 - 1)) * r) % w] + 0.0
                    assert _same(out[0, ct, row, (xa + k) % w], src), (ti, tj, row, q)
            assert _same(out[:, :, :, comb], yt[:, :, :, comb])                   # the comb is a copy
            rest = torch.ones((c, w), dtype=torch.bool, device=DEV)
            rest[:, comb] = False
            rest[ct, cols] = False
            assert not bool(_bits(out.permute(1, 3, 0, 2)[rest]).any())           # every other target is +0


# ---- 4, 5: the apply kernel's arithmetic and what it copies -------------------------------------------------------------------------------

@pytest.mark.parametrize("i", ALL)
def test_apply_against_float64_and_the_measured_bins_are_copies(i):
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    d = case(i)
    e = _engine(n, h, w)
    wts = R.rounded(d["wts"])
    out = fill(e, d["y"], d["mask"], wts, r, off, by, bx)
    ref = R.apply(d["y"], d["mask"], wts, r, off, by, bx)
    bound = np.stack([R.apply_bound_one(d["y"][k], d["mask"], wts[k], r, off, by, bx) for k in range(n)])
    err = np.abs(_np(out) - ref)
    miss = R.missing(d["mask"], r, off)
    worst = float((err[:, :, miss] / bound[:, :, miss]).max())
    print(f"case {i} {R.CASES[i]}: max |out - float64| {err.max():.3e}, largest |d| / bound {worst:.3e}, synthesised bins {int(miss.sum())} of {h * w}")
    assert (err <= bound).all() and miss.any()
    yt = torch.from_numpy(d["y"]).to(DEV)
    kept = torch.from_numpy(~miss).to(DEV)
    assert _same(out[:, :, kept], yt[:, :, kept])
    # one mask per slice, the centres of different widths: the bins of each slice's own mask are copies, the others are what the comb alone gives
    masks = np.stack([R.comb_mask(h, w, r, off, acs_w + 4 * (k % 2) - 2 * (k // 2)) for k in range(n)])
    y2 = d["y"] * masks[:, None] if n > 1 else d["y"]
    per = fill(e, y2, masks, wts, r, off, by, bx)
    bare = fill(e, y2, np.zeros((h, w), dtype=bool), wts, r, off, by, bx)
    mt = torch.from_numpy(masks).to(DEV)[:, None].expand(n, c, h, w)
    assert _same(per[mt], torch.from_numpy(np.ascontiguousarray(y2)).to(DEV)[mt]) and _same(per[~mt], bare[~mt])
    # wts_n = 1 against the same matrix repeated
    assert _same(fill(e, d["y"], d["mask"], wts[0], r, off, by, bx), fill(e, d["y"], d["mask"], np.stack([wts[0]] * n), r, off, by, bx))


# ---- 6, 7: a slice's bits are its own ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", ALL)
def test_an_all_zero_slice_is_flagged_stays_zero_and_leaves_its_neighbours_alone(i):
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    d = case(i)
    wts, info, out = both(_engine(n, h, w), i)
    y = np.concatenate([d["y"][:1], np.zeros_like(d["y"][:1]), d["y"][1:]])
    wz, iz, oz = both(_engine(n + 1, h, w), i, y=y)
    print(f"case {i}: info {iz.tolist()}")
    assert iz.tolist() == [0, 1] + [0] * (n - 1) and info.tolist() == [0] * n
    assert not bool(_bits(wz[1]).any()) and not bool(_bits(oz[1]).any())          # +0 weights; out = y0 = 0
    keep = [0] + list(range(2, n + 1))
    assert _same(wz[keep], wts) and _same(oz[keep], out)
    assert bool(torch.isfinite(torch.view_as_real(wz)).all()) and bool(torch.isfinite(torch.view_as_real(oz)).all())


@pytest.mark.parametrize("i", ALL)
def test_bits_do_not_depend_on_the_batch_the_call_the_stream_or_the_handle(i):
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    ns, nt = R.sizes(c, r, by, bx)
    d = case(i)
    e = _engine(n, h, w)
    ws0 = e.workspace_bytes
    wts, info, out = both(e, i)
    ws1 = e.workspace_bytes
    print(f"case {i}: workspace {ws0} -> {ws1}: + {ws1 - ws0} (documented 16 n ns (ns + nt) = {R.workspace_bytes(n, c, r, by, bx)})")
    assert ws1 - ws0 == R.workspace_bytes(n, c, r, by, bx) == 16 * n * ns * (ns + nt)
    again = both(e, i)
    assert _same(again[0], wts) and _same(again[2], out) and e.workspace_bytes == ws1 and e.coils == 0    # the first call only; the mode is untouched
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = both(e, i)
    side.synchronize()
    assert _same(on_side[0], wts) and _same(on_side[2], out)
    # a slice alone, and inside a batch of another size and order
    e1 = _engine(1, h, w, denoiser=(i == 0))                                     # (a denoiser handle)
    for k in range(n):
        w1, i1, o1 = both(e1, i, y=d["y"][k:k + 1])
        assert _same(w1[0], wts[k]) and _same(o1[0], out[k]) and int(i1[0]) == 0
    e3 = _engine(3, h, w, denoiser=(i == 1), **({"bf16_convs": True} if i == 1 else {}))    # (a bf16 handle)
    y3 = np.stack([d["y"][0] * np.float32(2), d["y"][n - 1], d["y"][0]])
    w3, _, o3 = both(e3, i, y=y3)
    assert _same(w3[1], wts[n - 1]) and _same(o3[1], out[n - 1]) and _same(w3[2], wts[0]) and _same(o3[2], out[0])


# ---- 8: the handle ------------------------------------------------------------------------------------------------------------------------------

def test_a_multi_coil_handle_steps_to_the_same_bits_before_and_after_a_grappa_call():
    i = 3
    n, c, h, w, r, off, (by, bx), acs_w = R.CASES[i]
    d = case(i)
    sens = torch.from_numpy(synthetic.coil_maps(c, h, w).astype(np.complex64)).to(DEV)
    y = torch.from_numpy(d["y"]).to(DEV)
    mask = torch.from_numpy(d["mask"]).to(DEV)
    x0 = (sens.conj()[None] * torch.fft.fftshift(torch.fft.ifft2(torch.fft.ifftshift(y, dim=(-2, -1)), norm="ortho"), dim=(-2, -1))).sum(
        dim=1, keepdim=True).contiguous()

    def run(with_grappa):
        e = _engine(n, h, w)
        e.set_prior("tv", 1.0, 8)
        x, z, u = e.reset(x0, y, mask, sens=sens, cg_iters=4)
        mu, sig = torch.full((n,), 0.3, device=DEV), torch.full((n,), 0.05, device=DEV)
        e.step(x, z, u, mu, sig)
        if with_grappa:
            wts, info = e.grappa_weights(y, (h, acs_w), r, kernel=(by, bx), lam=R.CASE_LAM)
            filled = e.grappa_apply(y, wts, mask, r, off, kernel=(by, bx))
            assert e.coils == c and info.tolist() == [0] * n and bool(torch.isfinite(torch.view_as_real(filled)).all())
        e.step(x, z, u, mu, sig)
        e.step(x, z, u, mu, sig)
        return x.clone(), z.clone(), u.clone()
    a, b = run(False), run(True)
    assert all(_same(p, q) for p, q in zip(a, b)) and bool(torch.isfinite(a[0]).all())


def test_argument_errors_that_need_the_handle_are_refused_with_the_outputs_untouched():
    e = _engine(2, 16, 80)
    c = 2
    y = G.guarded((2, c, 16, 80), torch.complex64, DEV, fill=1.0, name="y0")
    out = G.guarded((2, c, 16, 80), torch.complex64, DEV, name="out")
    wts = G.guarded((2, 7 * c, 4 * c), torch.complex64, DEV, name="wts")
    info = G.guarded((2,), torch.int32, DEV, name="info")
    mask = G.guarded((2, 16, 80), torch.uint8, DEV, fill=0, name="mask")
    before = {k: G.snapshot(v) for k, v in (("y0", y), ("out", out), ("wts", wts), ("info", info), ("mask", mask))}
    wcall = lambda acs_h, acs_w, r: e.lib.pnp_grappa_weights(e._h, y.data_ptr(), c, acs_h, acs_w, r, 1, 2, 1e-3, 0, wts.data_ptr(), info.data_ptr(),
                                                             None, None)
    acall = lambda r, mn, wn, o=None, yy=None: e.lib.pnp_grappa_apply(e._h, yy or y.data_ptr(), c, mask.data_ptr(), mn, r, 0, 1, 2, wts.data_ptr(), wn,
                                                                      o or out.data_ptr(), None)
    for args, what in (((16, 8, 3), b"accel"), ((16, 8, 6), b"accel"), ((18, 8, 2), b"acs_h"), ((16, 82, 2), b"acs_w")):
        assert wcall(*args) == -1 and what in e.lib.pnp_last_error() and b"pnp_grappa_weights" in e.lib.pnp_last_error(), e.lib.pnp_last_error()
    assert acall(3, 1, 1) == -1 and b"accel" in e.lib.pnp_last_error()
    assert acall(2, 3, 1) == -1 and b"mask_n" in e.lib.pnp_last_error()
    assert acall(2, 1, 3) == -1 and b"wts_n" in e.lib.pnp_last_error()
    assert acall(2, 1, 1, o=y.data_ptr() + 2 * c * 16 * 80 * 8 - 8) == -1 and b"overlap" in e.lib.pnp_last_error()
    # partial overlap among the buffers of the weights call: wts inside y0, info inside wts, gram reaching into wts
    part = lambda wp, ip, gp: e.lib.pnp_grappa_weights(e._h, y.data_ptr(), c, 16, 8, 2, 1, 2, 1e-3, 0, wp, ip, gp, None)
    for wp, ip, gp in ((y.data_ptr() + 64, info.data_ptr(), None), (wts.data_ptr(), wts.data_ptr() + 8, None),
                       (wts.data_ptr(), info.data_ptr(), wts.data_ptr() - 16), (wts.data_ptr(), info.data_ptr(), y.data_ptr() + 2 * c * 16 * 80 * 8 - 16)):
        assert part(wp, ip, gp) == -1 and b"alias" in e.lib.pnp_last_error(), e.lib.pnp_last_error()
    big = _engine(4096, 16, 16)
    assert big.lib.pnp_grappa_weights(big._h, y.data_ptr(), 16, 16, 8, 2, 1, 2, 1e-3, 0, wts.data_ptr(), info.data_ptr(), None, None) == -1
    assert b"n * coils" in big.lib.pnp_last_error()
    assert big.lib.pnp_grappa_apply(big._h, y.data_ptr(), 16, mask.data_ptr(), 1, 2, 0, 1, 2, wts.data_ptr(), 1, out.data_ptr(), None) == -1
    assert b"n * coils" in big.lib.pnp_last_error()
    G.check({"y0": y, "out": out, "wts": wts, "info": info, "mask": mask}, before)
    assert wcall(16, 8, 2) == 0 and acall(2, 2, 2) == 0                           # the valid calls go through
    G.check({"y0": y, "out": out, "wts": wts, "info": info, "mask": mask}, {k: before[k] for k in ("y0", "mask")})


# ---- 10: end to end -------------------------------------------------------------------------------------------------------------------------------

def test_acquisition_grappa_against_the_float64_pipeline_and_its_gain_over_aty0():
    f, p = R.FIXTURE, R.fixture()
    xr, pg, pa = R.pipeline(p)
    gain_ref = float((pg - pa)[0])
    print(f"reference: {pg[0]:.4f} dB from the GRAPPA-filled k-space, {pa[0]:.4f} dB ATy0, gain {gain_ref:.4f} dB (recorded {R.FIXTURE_GAIN_DB})")
    assert gain_ref >= 1.0 and abs(gain_ref - R.FIXTURE_GAIN_DB) <= 2e-3
    e = _engine(f["n"], f["h"], f["w"])
    r = acquisition.grappa(e, p["y0"], p["mask"], kernel=f["kernel"], lam=f["lam"], sens=p["sens"])
    assert r["info"].tolist() == [0] and r["x0"].shape == (1, 1, f["h"], f["w"]) and r["x0"].dtype == torch.float32
    assert r["y0"].shape == (1, f["coils"], f["h"], f["w"]) and r["rss"].shape == (1, f["h"], f["w"]) and r["wts"].shape == (1, 8, 160)
    xd = _np(r["x0"])[:, 0]
    pd = R.psnr(xd, p["gt"])
    gt = torch.from_numpy(p["gt"]).to(DEV)
    on_device = float(e.psnr(r["x0"].contiguous(), gt)[0])
    print(f"device: {pd[0]:.4f} dB (pnp_psnr {on_device:.4f}), |dPSNR| {abs(pd[0] - pg[0]):.3e} dB, max |dx| {np.abs(xd - xr).max():.3e}")
    assert abs(pd[0] - pg[0]) <= 0.01 and abs(on_device - pg[0]) <= 0.01
    mt = torch.from_numpy(p["mask"]).to(DEV)
    assert _same(r["y0"][:, :, mt], torch.from_numpy(p["y"]).to(DEV)[:, :, mt])
    rss_ref = np.sqrt((np.abs(synthetic.ifft2c_np(_np(r["y0"]))) ** 2).sum(axis=1))
    assert np.abs(_np(r["rss"]) - rss_ref).max() <= 1e-5 * rss_ref.max()


def test_cli_grappa_runs_and_starts_from_the_grappa_image(tmp_path):
    from dt4image_restoration_amd import cli
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5)]).astype(np.float32))
    with pytest.raises(SystemExit, match="--mask uniform: task 3x_10"):            # 64 columns hold no comb of every third
        cli.main(["--block_size", "6", "--n_embeds", "9", "--coils", "8", "--gt", str(gtd), "--tasks", "3x_10", "--mask", "uniform", "--grappa",
                  "--prior", "tv", "fixed", "--max_iter", "2"])
    base = ["--block_size", "6", "--n_embeds", "9", "--size", "64", "--limit", "2", "--coils", "8", "--mask", "uniform", "--prior", "tv", "--seed", "3"]
    mode = ["fixed", "--max_iter", "4"]

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = cli.main(base + extra + mode)
        return out, [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
    out, lines = run(["--grappa"])
    print(lines)
    assert len(lines) == 2 and [l["psnr"] for l in lines] == [o["psnr"] for o in out] and all(np.isfinite(l["psnr"]) for l in lines)
    small, _ = run(["--grappa", "--grappa-kernel", "3", "2", "--grappa-lambda", "0.1"])
    plain, _ = run([])
    # the start differs (x0 from the GRAPPA-filled k-space), the measurements do not: the initial PSNR moves, the run completes either way
    i0 = [o["psnr"] - o["psnr_increment"] for o in out]
    i1 = [o["psnr"] - o["psnr_increment"] for o in plain]
    print("initial psnr with --grappa", i0, "without", i1)
    assert all(abs(a - b) > 1e-3 for a, b in zip(i0, i1)) and all(np.isfinite(o["psnr"]) for o in small + plain)
