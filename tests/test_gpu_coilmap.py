"""The coil map estimate (pnp_estimate_sens) on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against the float64
restatement of tests/coilmap_ref.py computed from the float32 k-space the device is handed.  Every figure is printed and attached with
record_property before it is asserted.

BOUNDS.  Ten times what the float32 restatement of the estimator (coilmap_ref.estimate_f32: torch CPU complex64, whose FFT is truly
float32) measures against the float64 one on the CPU, per case, the margin the suite gives its FFT and solve checks.  Measured on the CPU
(rss = max |d rss| / max rss_ref; maps = max |dS| over the pixels with rss_ref > 1e-3 smax_ref; unit = max |sum_c |S_c|^2 - 1| on the kept
set; near = the largest share of a slice within 1e-5 smax_ref of the threshold; flips = kept pixels that differ AWAY from the threshold):

      N  C   H    W    block     window thresh   rss         maps        unit        near      flips
      1  1   16   16   2 x 2     box    0        8.446e-08   1.389e-07   1.440e-07   0         0
      2  3   32   80   16 x 16   hann   0.05     8.971e-08   6.744e-07   1.680e-07   0         0
      2  8   64   64   24 x 24   hann   0.05     8.425e-08   6.457e-07   1.722e-07   0         0
      2  8   64   64   64 x 64   box    0        7.782e-08   3.607e-07   1.562e-07   0         0
      3  2   128  160  24 x 160  hann   0.1      1.628e-07   5.900e-07   1.891e-07   4.9e-05   0
      1  32  64   80   64 x 6    hann   0.05     8.691e-08   4.358e-07   1.321e-07   0         0

The kept set may differ from the reference's only on pixels near the threshold (|rss_ref - thresh smax_ref| <= 1e-5 smax_ref); those are left
out of the comparison and may be at most 0.5 % of a slice.  Off the kept set the maps are exact zeros.

Chain (2 x 64 x 64, 4 coils, cartesian_mask(64, 64, 4), block 64 x 4 from the mask, Hann, thresh 0.05, then pnp_reset_mc and one
pnp_prox_dual at mu = 0.3, K = 8): z against sense_ref.prox_dual in float64 fed the REFERENCE's estimated maps.  The float32 restatement of
the whole chain (estimate_f32, then sense_ref.cg_solve_f32) measured max |dz| / max |z_ref| = 4.657e-07 and ||dz|| / ||z_ref|| = 2.459e-07 on
the CPU; the bounds are ten times that.  No pixel of that problem is near the threshold (asserted on the reference), so the kept sets agree.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coilmap_ref as R  # noqa: E402
import sense_ref as SR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0
F32 = [  # (rss, maps, unit) of the float32 restatement per case of coilmap_ref.CASES, from the table above
    (8.446e-08, 1.389e-07, 1.440e-07), (8.971e-08, 6.744e-07, 1.680e-07), (8.425e-08, 6.457e-07, 1.722e-07),
    (7.782e-08, 3.607e-07, 1.562e-07), (1.628e-07, 5.900e-07, 1.891e-07), (8.691e-08, 4.358e-07, 1.321e-07)]
CHAIN_F32 = (4.657e-07, 2.459e-07)
DEV = "cuda"


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=kw.pop("denoiser", False), **kw)


def c64(a):
    return torch.from_numpy(np.array(a, dtype=np.complex64)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.complex128 if t.is_complex() else np.float64)


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_estimate_against_float64(i, record_property):
    n, c, h, w, acs, kind, thresh = R.CASES[i]
    y, ref = R.case_ref(i)
    e = _engine(n, h, w)
    maps, rss = e.estimate_sens(c64(y), acs, window=kind, thresh=thresh, return_rss=True)
    assert maps.shape == (n, c, h, w) and maps.dtype == torch.complex64 and rss.shape == (n, h, w) and rss.dtype == torch.float32
    f = R.compare(_np(maps), _np(rss), ref, thresh)
    brss, bmaps, bunit = (MARGIN * v for v in F32[i])
    print(f"{n}x{c}x{h}x{w} block {acs} {kind} thresh {thresh}: rss {f['rss']:.3e} / {brss:.2e}  maps {f['maps']:.3e} / {bmaps:.2e}  "
          f"unit {f['unit']:.3e} / {bunit:.2e}  near {f['near']:.2e}  flips {f['flips']}  off_zero {f['off_zero']}  finite {f['finite']}")
    for k, v in f.items():
        record_property(k, v)
    assert f["finite"]
    assert f["near"] <= R.NEAR_SHARE and f["flips"] == 0
    assert f["off_zero"]
    assert f["rss"] <= brss and f["maps"] <= bmaps and f["unit"] <= bunit
    assert e.coils == 0                                                            # an estimate does not change the handle's mode


def _case(i=2):
    n, c, h, w, acs, kind, thresh = R.CASES[i]
    return c64(R.case_ref(i)[0]), acs, kind, thresh, (n, c, h, w)


def test_without_an_rss_output_the_maps_have_the_same_bits():
    y, acs, kind, thresh, (n, c, h, w) = _case()
    e = _engine(n, h, w)
    with_rss = e.estimate_sens(y, acs, window=kind, thresh=thresh, return_rss=True)[0]
    assert _same(e.estimate_sens(y, acs, window=kind, thresh=thresh), with_rss)


def test_two_calls_give_the_same_bits():
    y, acs, kind, thresh, (n, c, h, w) = _case(4)
    e = _engine(n, h, w)
    a, ra = e.estimate_sens(y, acs, window=kind, thresh=thresh, return_rss=True)
    b, rb = e.estimate_sens(y, acs, window=kind, thresh=thresh, return_rss=True)
    assert _same(a, b) and _same(ra, rb)


def test_a_slice_gives_the_same_bits_alone_at_every_place_of_a_batch_on_a_side_stream_and_on_every_handle_kind():
    c, h, w, acs, kind, thresh = 3, 32, 80, (16, 16), "hann", 0.05
    y = c64(R.case_y(3, c, h, w, 31))
    e3 = _engine(3, h, w)
    maps, rss = e3.estimate_sens(y, acs, window=kind, thresh=thresh, return_rss=True)
    assert not _same(maps[0], maps[1]) and not _same(maps[1], maps[2])
    e1 = _engine(1, h, w)
    for i in range(3):                                                             # alone
        m1, r1 = e1.estimate_sens(y[i:i + 1].clone(), acs, window=kind, thresh=thresh, return_rss=True)
        assert _same(m1[0], maps[i]) and _same(r1[0], rss[i]), i
    for shift in (1, 2):                                                           # at the two other places
        perm = [(i + shift) % 3 for i in range(3)]
        mp, rp = e3.estimate_sens(y[perm].contiguous(), acs, window=kind, thresh=thresh, return_rss=True)
        for j, i in enumerate(perm):
            assert _same(mp[j], maps[i]) and _same(rp[j], rss[i]), (shift, j)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ms, rs = e3.estimate_sens(y, acs, window=kind, thresh=thresh, return_rss=True)
    side.synchronize()
    assert _same(ms, maps) and _same(rs, rss)
    for kw in (dict(denoiser=True), dict(denoiser=True, bf16_convs=True)):         # handles with a denoiser, f32 and bf16
        mk = _engine(3, h, w, **kw).estimate_sens(y, acs, window=kind, thresh=thresh)
        assert _same(mk, maps), kw


def test_a_closed_form_handle_steps_bit_for_bit_as_before_after_an_estimate():
    n, h, w = 2, 64, 64
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=9)
    x0, y0 = c64(d["x0"][..., 0] + 1j * d["x0"][..., 1]), c64(d["y0"][..., 0] + 1j * d["y0"][..., 1])
    mask = torch.from_numpy(d["mask"]).to(DEV)
    mu = torch.tensor([0.1, 0.4], device=DEV)
    ymc = c64(R.case_y(n, 8, h, w, 13))
    used, fresh = _engine(n, h, w), _engine(n, h, w)
    out = []
    for e in (used, fresh):
        x, z, u = e.reset(x0, y0, mask)
        e.prox_dual(x, z, u, mu)
        if e is used:
            e.estimate_sens(ymc, (24, 24))
            e.estimate_sens(ymc, (64, 64), window="box", return_rss=True)
            assert e.coils == 0
        e.prox_dual(x, z, u, mu)
        out.append((x, z, u, e.residuals(x, z, u, dc=True)))
    for a, b in zip(*out):
        assert _same(a, b)


def test_a_multi_coil_handle_keeps_its_mode_and_its_next_prox_dual_bits():
    n, h, w, coils = 2, 64, 64, 4
    cs = SR.solve_case(h, w, coils, False, "radial", 4)
    mask = torch.from_numpy(cs["mask"]).to(DEV)
    mu = torch.tensor([0.05, 0.3], device=DEV)
    iterate = lambda: (torch.from_numpy(cs["x"]).float().to(DEV).reshape(n, 1, h, w), c64(cs["z0"]).reshape(n, 1, h, w),
                       c64(cs["u"]).reshape(n, 1, h, w))
    used, fresh = _engine(n, h, w), _engine(n, h, w)
    out = []
    for e in (used, fresh):
        e.set_kspace(c64(cs["y"]), mask, sens=c64(cs["sens"]), cg_iters=4)
        x, z, u = iterate()
        e.prox_dual(x, z, u, mu)
        if e is used:
            e.estimate_sens(c64(R.case_y(n, 8, h, w, 13)), (24, 24), thresh=0.05)   # another coil count than the installed one
            assert e.coils == coils
        e.prox_dual(x, z, u, mu)
        out.append((z, u, e.cg_residual()))
    for a, b in zip(*out):
        assert _same(a, b)


def test_workspace_grows_by_the_documented_bytes_once():
    n, c, h, w = 2, 3, 32, 80
    y = c64(R.case_y(n, c, h, w, 12))
    e = _engine(n, h, w)
    chunks = -(-h * w // 2048)
    ws0 = e.workspace_bytes
    e.estimate_sens(y, (16, 16), return_rss=True)
    ws1 = e.workspace_bytes
    assert ws1 - ws0 == 4 * n * chunks + 4 * n
    e.estimate_sens(y, (16, 16), return_rss=True)
    assert e.workspace_bytes == ws1
    e.estimate_sens(y, (16, 16))                                                   # no rss output: the handle's own plane
    ws2 = e.workspace_bytes
    assert ws2 - ws1 == 4 * n * h * w
    e.estimate_sens(y, (8, 8), window="box")
    e.estimate_sens(y, (16, 16), return_rss=True)
    assert e.workspace_bytes == ws2


def test_errors_that_need_a_handle_leave_the_output_untouched():
    n, c, h, w = 1, 2, 32, 80
    e = _engine(n, h, w)
    y = c64(R.case_y(n, c, h, w, 12))
    sens = torch.full((n, c, h, w), 7.0 + 0j, dtype=torch.complex64, device=DEV)
    call = lambda eng, ah, aw: eng.lib.pnp_estimate_sens(eng._h, y.data_ptr(), c, ah, aw, _lib.PNP_SENS_HANN, 0.05, 0, sens.data_ptr(), None, None)
    for ah, aw, what in ((34, 16, b"acs_h"), (16, 82, b"acs_w"), (64, 160, b"acs_h")):
        assert call(e, ah, aw) == -1 and what in e.lib.pnp_last_error(), (ah, aw)
    odd = _engine(1, 48, 48)                                                        # a size the k-space stage refuses
    assert call(odd, 16, 16) == -1 and b"k-space stage" in odd.lib.pnp_last_error()
    torch.cuda.synchronize()
    assert bool((sens == 7.0).all())
    assert call(e, 32, 80) == 0                                                     # block = plane is accepted
    with pytest.raises(ValueError, match="window"):
        e.estimate_sens(y, (16, 16), window="hamming")


def test_acquisition_estimate_sens_takes_the_block_from_the_mask():
    n, c, h, w = 2, 4, 64, 64
    mask = acquisition.cartesian_mask(h, w, 4)
    d = synthetic.make_problem_mc(n, h, w, c, seed=11, mask=mask)
    e = _engine(n, h, w)
    auto = acquisition.estimate_sens(e, d["y0"], mask=mask)                         # the real view [N,C,H,W,2] of the batch dict
    acs = acquisition.acs_block(mask)
    assert acs == (64, 4)
    want = e.estimate_sens(c64(d["y0"][..., 0] + 1j * d["y0"][..., 1]), acs, window="hann", thresh=0.05)
    assert auto.shape == (n, c, h, w) and auto.dtype == torch.complex64 and auto.is_cuda and _same(auto, want)
    assert _same(acquisition.estimate_sens(e, torch.from_numpy(d["y0"]).to(DEV), mask=torch.from_numpy(mask).to(DEV), acs=acs), want)
    with pytest.raises(ValueError):
        acquisition.estimate_sens(e, d["y0"])                                       # neither a block nor a mask


def test_chain_estimate_then_reset_mc_then_prox_dual_against_float64(record_property):
    n, c, h, w, K = 2, 4, 64, 64, 8
    mask = acquisition.cartesian_mask(h, w, 4)
    d = synthetic.make_problem_mc(n, h, w, c, seed=11, mask=mask)
    y = (d["y0"][..., 0] + 1j * d["y0"][..., 1]).astype(np.complex64)
    x0 = (d["x0"][:, 0, ..., 0] + 1j * d["x0"][:, 0, ..., 1]).astype(np.complex64)
    acs = acquisition.acs_block(mask)
    ref = R.estimate(y, acs, "hann", 0.05)
    assert not (np.abs(ref[1] - np.float64(np.float32(0.05)) * ref[3][:, None, None]) <= R.NEAR_CUT * ref[3][:, None, None]).any()
    mu64 = np.full(n, np.float64(np.float32(0.3)))
    zr, ur, rr = SR.prox_dual(x0.real.astype(np.float64), x0.astype(np.complex128), np.zeros((n, h, w), dtype=np.complex128),
                              y.astype(np.complex128), ref[0], mask, mu64, K)
    e = _engine(n, h, w)
    maps = acquisition.estimate_sens(e, c64(y), mask=mask)
    f = R.compare(_np(maps), ref[1], ref, 0.05)                                     # (rss is not an output here: the reference's own)
    assert f["flips"] == 0 and f["off_zero"]
    x, z, u = e.reset(c64(x0).reshape(n, 1, h, w), c64(y), torch.from_numpy(mask).to(DEV), sens=maps, cg_iters=K)
    assert e.coils == c
    e.prox_dual(x, z, u, torch.full((n,), 0.3, dtype=torch.float32, device=DEV))
    emax, erms = SR.solve_errors(_np(z)[:, 0], zr)
    umax = float(np.abs(_np(u)[:, 0] - ur).max() / np.abs(zr).max())
    bmax, brms = (MARGIN * v for v in CHAIN_F32)
    print(f"chain: maps {f['maps']:.3e}; z err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  u {umax:.3e}; "
          f"cg_res {e.cg_residual().cpu().numpy()} ref {rr}")
    record_property("err_max", emax); record_property("err_rms", erms); record_property("u_max", umax)
    assert emax <= bmax and erms <= brms and umax <= 2 * bmax
