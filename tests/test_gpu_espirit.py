"""The ESPIRiT coil map estimate (pnp_espirit_sens) on the MI355X, through the C ABI (PnPEngine is the ctypes binding), against the float64
restatement of tests/espirit_ref.py computed from the float32 k-space the device is handed.  Every figure is printed and attached with
record_property before it is asserted.

CASES (espirit_ref.CASES; data of make_problem_mc with a full mask, sv_thresh 0.02, crop 0.9, 16 power steps, Hann window; each at
thresh 0.05 and thresh 0):

      N  C   H    W    block    k  sigma_n  n    covers
      3  4   64   64   24 x 24  4  1/255    64   a matrix the coil-compression solver would hold on chip
      1  5   80   64   20 x 24  4  1/255    80   an odd coil count, a 2^a 5^b side, a non-square plane, n just past 64
      2  8   64   80   24 x 24  5  1/255    200  odd k
      2  8   128  128  24 x 24  6  10/255   288  the default configuration
      1  12  64   64   24 x 24  4  1/255    192  more than 8 coils: the 16-coil instantiation of the pixel kernel

BOUNDS.  nkept is equal.  kern is within 2^-22 max |R|: one float32 rounding on each side with a fourfold margin.  Every other bound is ten
times what the float32 restatement of the per-pixel part (espirit_ref.espirit(f32=True): float32 transform, twiddles, G_q, power steps,
quotient and phase) measures against the float64 one on the CPU (eval = max |d lambda|; unit = max |sum_c |S_c|^2 - 1| on the kept set;
prod = max |S_a conj(S_b) - ref| on the kept set, phase-free; maps = max |dS| on the kept set - with thresh = 0 only where the
reference's |p| >= 1e-2 smax, which may leave out at most 15 % of a slice (left = the share of a slice that is kept and left out):

      case thresh   eval        unit        prod        maps        left     near      gap of the Gram eigenvalues from the cut
      0    0.05     1.015e-05   4.287e-07   3.476e-07   5.055e-07   -        4.9e-04   4.1e-02
      0    0        1.015e-05   4.287e-07   2.593e-05   1.989e-06   0.108    2.4e-04
      1    0.05     4.934e-06   3.749e-07   3.262e-07   6.763e-07   -        3.9e-04   1.4e-01
      1    0        4.934e-06   3.749e-07   1.305e-05   2.043e-06   0.077    3.9e-04
      2    0.05     1.541e-05   4.324e-07   2.305e-07   2.087e-07   -        2.0e-04   3.7e-02
      2    0        1.541e-05   4.324e-07   4.433e-06   1.715e-06   0.061    2.0e-04
      3    0.05     1.325e-06   4.636e-07   2.471e-07   3.313e-07   -        3.1e-04   2.2e-03
      3    0        1.325e-06   4.636e-07   2.282e-06   1.394e-06   0.036    3.1e-04
      4    0.05     1.318e-06   4.981e-07   1.307e-07   1.478e-07   -        0         4.0e-02
      4    0        1.318e-06   4.981e-07   3.562e-06   1.120e-06   0.084    0

Pixels within 1e-4 of the crop (or within 1e-5 smax of the rss threshold, as in test_gpu_coilmap.py) may fall on either side; they are left
out of eval / unit / the kept-set comparison and are at most 1e-3 of a slice (near, asserted on the reference).  Off the kept set the maps
are exact zeros.

Chain (2 x 64 x 64, 4 coils, cartesian_mask(64, 64, 4), block 24 x 4 = the mask's 64 x 4 cropped to 24 x 24, 2 x 2 kernels: 69 windows for
n = 16; thresh 0.05; then pnp_reset_mc and one pnp_prox_dual at mu = 0.3, K = 8): z against sense_ref.prox_dual in float64 fed the
REFERENCE's ESPIRiT maps.  The float32 restatement of the whole chain measured max |dz| / max |z_ref| = 4.284e-07 and ||dz|| / ||z_ref|| = 2.925e-07
on the CPU; the bounds are ten times that.  No pixel of that problem is in a band (asserted on the reference), so the kept sets agree.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import espirit_ref as R  # noqa: E402
import guard_bands as GB  # noqa: E402
import sense_ref as SR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 10.0
KERN_BOUND = 2.0 ** -22
#      (eval, unit, prod, maps) of the float32 restatement per (case, thresh), from the table above
F32 = {(0, 0.05): (1.015e-05, 4.287e-07, 3.476e-07, 5.055e-07), (0, 0.0): (1.015e-05, 4.287e-07, 2.593e-05, 1.989e-06),
       (1, 0.05): (4.934e-06, 3.749e-07, 3.262e-07, 6.763e-07), (1, 0.0): (4.934e-06, 3.749e-07, 1.305e-05, 2.043e-06),
       (2, 0.05): (1.541e-05, 4.324e-07, 2.305e-07, 2.087e-07), (2, 0.0): (1.541e-05, 4.324e-07, 4.433e-06, 1.715e-06),
       (3, 0.05): (1.325e-06, 4.636e-07, 2.471e-07, 3.313e-07), (3, 0.0): (1.325e-06, 4.636e-07, 2.282e-06, 1.394e-06),
       (4, 0.05): (1.318e-06, 4.981e-07, 1.307e-07, 1.478e-07), (4, 0.0): (1.318e-06, 4.981e-07, 3.562e-06, 1.120e-06)}
CHAIN_F32 = (4.284e-07, 2.925e-07)
DEV = "cuda"
C64, F32T, I32 = torch.complex64, torch.float32, torch.int32


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
    return all(bool(torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b)) if isinstance(a, tuple) else bool(torch.equal(_bits(a), _bits(b)))


def _run(e, y, acs, k, thresh=0.05, **kw):
    """(maps, eval, kern, nkept) with the cases' parameters."""
    return e.espirit_sens(y, acs, ksize=k, sv_thresh=R.SV, crop=R.CROP, iters=R.ITERS, window="hann", thresh=thresh, return_eval=True,
                          return_kernels=True, **kw)


def _fixture_conditions(ref, acs, k, c, crop, thresh):
    """The conditions under which the device and the reference must agree, asserted on the reference."""
    assert R.windows(acs, k) >= c * k * k
    assert R.sv_gap(ref["lam"], R.SV) > R.SV_GAP
    near = R.band(ref, crop, thresh)
    assert near.reshape(near.shape[0], -1).mean(axis=1).max() <= R.BAND_SHARE


@pytest.mark.parametrize("thresh", R.THRESHES)
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_espirit_against_float64(i, thresh, record_property):
    n, c, h, w, acs, k, _ = R.CASES[i]
    y, ref = R.case_ref(i, thresh)
    _fixture_conditions(ref, acs, k, c, R.CROP, thresh)
    e = _engine(n, h, w)
    maps, ev, kern, nkept = _run(e, c64(y), acs, k, thresh)
    d = 2 * k - 1
    assert maps.shape == (n, c, h, w) and maps.dtype == C64 and ev.shape == (n, h, w) and ev.dtype == F32T
    assert kern.shape == (n, c, c, d, d) and kern.dtype == C64 and nkept.shape == (n,) and nkept.dtype == I32
    f = R.compare(_np(maps), _np(ev), _np(kern), nkept.cpu().numpy(), ref, R.CROP, thresh)
    beval, bunit, bprod, bmaps = (MARGIN * v for v in F32[(i, thresh)])
    got_maps = f["maps_all"] if thresh > 0 else f["maps"]
    print(f"case {i} {n}x{c}x{h}x{w} block {acs} k {k} thresh {thresh}: nkept {nkept.tolist()} ref {ref['nkept'].tolist()}  kern {f['kern']:.3e} / "
          f"{KERN_BOUND:.2e}  eval {f['eval']:.3e} / {beval:.2e}  unit {f['unit']:.3e} / {bunit:.2e}  prod {f['prod']:.3e} / {bprod:.2e}  "
          f"maps {got_maps:.3e} / {bmaps:.2e} (all kept: {f['maps_all']:.3e})  left_out {f['left_out']:.3f}  near {f['near']:.2e}  "
          f"flips {f['flips']}  off_zero {f['off_zero']}  finite {f['finite']}")
    for key, v in f.items():
        record_property(key, v)
    assert f["finite"]
    assert f["nkept"]
    assert f["kern"] <= KERN_BOUND
    assert f["flips"] == 0 and f["off_zero"]
    assert f["eval"] <= beval and f["unit"] <= bunit and f["prod"] <= bprod
    if thresh == 0:
        assert f["left_out"] <= R.P_SHARE
    assert got_maps <= bmaps
    assert e.coils == 0                                                            # an estimate does not change the handle's mode


def test_a_slice_gives_the_same_bits_alone_at_every_place_of_a_batch_on_a_side_stream_and_twice_in_a_row():
    n, c, h, w, acs, k, _ = R.CASES[0]
    y = c64(R.case_ref(0)[0])
    e3 = _engine(n, h, w)
    base = _run(e3, y, acs, k)
    assert _same(_run(e3, y, acs, k), base)                                        # two calls in a row
    assert not _same(base[0][0], base[0][1]) and not _same(base[0][1], base[0][2])
    e1 = _engine(1, h, w)
    for i in range(n):                                                             # alone
        one = _run(e1, y[i:i + 1].clone(), acs, k)
        assert all(_same(o[0], b[i]) for o, b in zip(one, base)), i
    for shift in (1, 2):                                                           # at the two other places
        perm = [(i + shift) % n for i in range(n)]
        got = _run(e3, y[perm].contiguous(), acs, k)
        for j, i in enumerate(perm):
            assert all(_same(g[j], b[i]) for g, b in zip(got, base)), (shift, j)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = _run(e3, y, acs, k)
    side.synchronize()
    assert _same(got, base)
    assert _same(_engine(n, h, w, denoiser=True).espirit_sens(y, acs, ksize=k, thresh=0.05), base[0])   # a handle with a denoiser
    assert _same(e3.espirit_sens(y, acs, ksize=k, thresh=0.05), base[0])           # without the optional outputs


def test_chain_espirit_then_reset_mc_then_prox_dual_against_float64(record_property):
    t, q = R.CHAIN, R.chain_problem()
    n, c, h, w, K = t["n"], t["c"], t["h"], t["w"], t["K"]
    ref, zr, ur, rr = R.chain_reference()
    assert q["acs"] == (24, 4)
    _fixture_conditions(ref, q["acs"], t["ksize"], c, R.CROP, t["thresh"])
    assert not R.band(ref, R.CROP, t["thresh"]).any()
    e = _engine(n, h, w)
    maps = acquisition.estimate_sens(e, c64(q["y"]), mask=q["mask"], method="espirit", ksize=t["ksize"], thresh=t["thresh"], cal=t["cal"])
    want = e.espirit_sens(c64(q["y"]), q["acs"], ksize=t["ksize"], thresh=t["thresh"])
    assert _same(maps, want)
    power = (np.abs(_np(maps)) ** 2).sum(axis=1)
    assert np.array_equal(power > 0.5, ref["kept"])
    x, z, u = e.reset(c64(q["x0"]).reshape(n, 1, h, w), c64(q["y"]), torch.from_numpy(q["mask"]).to(DEV), sens=maps, cg_iters=K)
    assert e.coils == c
    e.prox_dual(x, z, u, torch.full((n,), t["mu"], dtype=torch.float32, device=DEV))
    emax, erms = SR.solve_errors(_np(z)[:, 0], zr)
    umax = float(np.abs(_np(u)[:, 0] - ur).max() / np.abs(zr).max())
    bmax, brms = (MARGIN * v for v in CHAIN_F32)
    print(f"chain: maps {float(np.abs(_np(maps) - ref['maps']).max()):.3e}; z err_max {emax:.3e} / {bmax:.2e}  err_rms {erms:.3e} / {brms:.2e}  "
          f"u {umax:.3e}; cg_res {e.cg_residual().cpu().numpy()} ref {rr}")
    record_property("err_max", emax); record_property("err_rms", erms); record_property("u_max", umax)
    assert emax <= bmax and erms <= brms and umax <= 2 * bmax


def test_an_all_zero_block_gives_zero_maps_and_no_nan():
    n, c, h, w, acs, k = 2, 5, 64, 64, (20, 24), 4
    y = c64(R.case_y(n, c, h, w, 1.0 / 255.0, 17)).clone()
    y[1, :, h // 2 - 10:h // 2 + 10, w // 2 - 12:w // 2 + 12] = 0                   # slice 1: an empty block under a non-empty plane
    y[0] = 0
    maps, ev, kern, nkept = _run(_engine(n, h, w), y, acs, k, thresh=0.0)
    for t in (maps, ev, kern):
        v = torch.view_as_real(t) if t.is_complex() else t
        assert bool(torch.isfinite(v).all()) and not bool(v.any())
    assert nkept.tolist() == [0, 0]


def test_a_closed_form_handle_steps_bit_for_bit_as_before_after_an_estimate():
    n, h, w = 2, 64, 64
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=9)
    x0, y0 = c64(d["x0"][..., 0] + 1j * d["x0"][..., 1]), c64(d["y0"][..., 0] + 1j * d["y0"][..., 1])
    mask = torch.from_numpy(d["mask"]).to(DEV)
    mu = torch.tensor([0.1, 0.4], device=DEV)
    ymc = c64(R.case_y(n, 4, h, w, 1.0 / 255.0, 13))
    used, fresh = _engine(n, h, w), _engine(n, h, w)
    out = []
    for e in (used, fresh):
        x, z, u = e.reset(x0, y0, mask)
        e.prox_dual(x, z, u, mu)
        if e is used:
            e.espirit_sens(ymc, (24, 24), ksize=4)
            e.espirit_sens(ymc, (16, 20), ksize=3, window="box", return_eval=True, return_kernels=True)
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
            e.espirit_sens(c64(R.case_y(n, 5, h, w, 1.0 / 255.0, 13)), (24, 24), ksize=4, thresh=0.05)   # another coil count than the installed one
            assert e.coils == coils
        e.prox_dual(x, z, u, mu)
        out.append((z, u, e.cg_residual()))
    for a, b in zip(*out):
        assert _same(a, b)


def _es_bytes(n, c, k):
    npad = (c * k * k + 1) & ~1
    return n * (32 * npad * npad + 8 * c * c * (2 * k - 1) ** 2 + 8)


def test_workspace_grows_by_the_documented_bytes():
    n, c, h, w = 2, 5, 64, 64
    y = c64(R.case_y(n, c, h, w, 1.0 / 255.0, 12))
    e = _engine(n, h, w)
    chunks = -(-h * w // 2048)
    ws0 = e.workspace_bytes
    e.espirit_sens(y, (16, 16), ksize=3)                                           # n = 45, padded to 46
    ws1 = e.workspace_bytes
    assert ws1 - ws0 == 4 * n * chunks + 4 * n + 4 * n * h * w + _es_bytes(n, c, 3)
    e.espirit_sens(y, (16, 16), ksize=3, return_eval=True, return_kernels=True)
    e.espirit_sens(y, (8, 8), ksize=2)
    assert e.workspace_bytes == ws1
    e.espirit_sens(y, (16, 16), ksize=4)                                           # a larger matrix: the buffer is replaced by a larger one
    assert e.workspace_bytes - ws1 == _es_bytes(n, c, 4) - _es_bytes(n, c, 3)
    e.estimate_sens(y, (16, 16))                                                    # shares the coil map workspace: nothing new
    assert e.workspace_bytes - ws1 == _es_bytes(n, c, 4) - _es_bytes(n, c, 3)


@pytest.mark.parametrize("optional", [True, False], ids=["all-outputs", "null-outputs"])
@pytest.mark.parametrize("shape,c,k,acs", [((2, 64, 80), 5, 3, (16, 12)), ((1, 32, 32), 12, 2, (8, 8)), ((1, 16, 16), 1, 2, (16, 16))],
                         ids=["2x64x80-C5", "1x32x32-C12", "1x16x16-C1"])
def test_guard_bands_around_every_caller_buffer(shape, c, k, acs, optional):
    n, h, w = shape
    d = 2 * k - 1
    e = _engine(n, h, w)
    g = torch.Generator().manual_seed(5)
    y0 = GB.guarded((n, c, h, w), C64, DEV, fill=torch.view_as_complex(torch.randn((n, c, h, w, 2), generator=g)), name="y0")
    sens = GB.guarded((n, c, h, w), C64, DEV, name="sens")
    ev = GB.guarded((n, h, w), F32T, DEV, name="eval") if optional else None
    kern = GB.guarded((n, c, c, d, d), C64, DEV, name="kern") if optional else None
    nkept = GB.guarded((n,), I32, DEV, name="nkept") if optional else None
    ptr = lambda t: None if t is None else t.data_ptr()
    for window, thresh in ((_lib.PNP_SENS_HANN, 0.05), (_lib.PNP_SENS_BOX, 0.0)):
        with GB.watch(outputs={"sens": sens, "eval": ev, "kern": kern, "nkept": nkept}, inputs={"y0": y0}):
            rc = e.lib.pnp_espirit_sens(e._h, y0.data_ptr(), c, acs[0], acs[1], k, 0.02, 0.5, 4, window, thresh, 0, sens.data_ptr(), ptr(ev),
                                        ptr(kern), ptr(nkept), None)
            assert rc == 0, e.lib.pnp_last_error()
        assert bool(torch.isfinite(torch.view_as_real(sens)).all())
        if optional:
            assert bool(torch.isfinite(ev).all()) and bool(torch.isfinite(torch.view_as_real(kern)).all())
            assert all(0 <= v <= c * k * k for v in nkept.tolist())


def test_every_argument_error_is_invalid_and_leaves_the_outputs_untouched():
    n, c, h, w, k = 1, 2, 32, 80, 3
    e = _engine(n, h, w)
    y = c64(R.case_y(n, c, h, w, 1.0 / 255.0, 12))
    d = 2 * k - 1
    sens = torch.full((n, c, h, w), 7.0 + 0j, dtype=C64, device=DEV)
    ev = torch.full((n, h, w), 7.0, dtype=F32T, device=DEV)
    kern = torch.full((n, 16, 16, 15, 15), 7.0 + 0j, dtype=C64, device=DEV)        # large enough for every refused argument set
    nkept = torch.full((n,), 7, dtype=I32, device=DEV)
    good = dict(h=e._h, y0=y.data_ptr(), coils=c, acs_h=16, acs_w=16, ksize=k, sv=0.02, crop=0.9, iters=8, window=_lib.PNP_SENS_HANN, thresh=0.05,
                flags=0, sens=sens.data_ptr())

    def call(eng=e, **kw):
        a = dict(good, h=eng._h, **kw)
        return eng.lib.pnp_espirit_sens(a["h"], a["y0"], a["coils"], a["acs_h"], a["acs_w"], a["ksize"], a["sv"], a["crop"], a["iters"], a["window"],
                                        a["thresh"], a["flags"], a["sens"], ev.data_ptr(), kern.data_ptr(), nkept.data_ptr(), None)

    nan = float("nan")
    bad = [(dict(h=None), b"null handle"), (dict(y0=None), b"null y0"), (dict(sens=None), b"null sens"), (dict(sens=y.data_ptr()), b"alias"),
           (dict(coils=0), b"coils"), (dict(coils=17), b"coils"), (dict(ksize=1), b"ksize"), (dict(ksize=9), b"ksize"),
           (dict(coils=16, ksize=6), b"ksize^2"), (dict(acs_h=15), b"acs_h"), (dict(acs_w=2), b"acs_w"), (dict(acs_h=34), b"acs_h"),
           (dict(acs_w=82), b"acs_w"), (dict(sv=0.0), b"sv_thresh"), (dict(sv=1.0), b"sv_thresh"), (dict(sv=nan), b"sv_thresh"),
           (dict(crop=-0.1), b"crop"), (dict(crop=1.0), b"crop"), (dict(crop=nan), b"crop"), (dict(thresh=-0.5), b"thresh"),
           (dict(thresh=1.0), b"thresh"), (dict(thresh=nan), b"thresh"), (dict(iters=0), b"iters"), (dict(iters=65), b"iters"),
           (dict(window=2), b"window"), (dict(flags=4), b"flags")]
    for kw, what in bad:
        if kw.get("h", 1) is None:
            rc = e.lib.pnp_espirit_sens(None, good["y0"], c, 16, 16, k, 0.02, 0.9, 8, _lib.PNP_SENS_HANN, 0.05, 0, good["sens"], ev.data_ptr(),
                                        kern.data_ptr(), nkept.data_ptr(), None)
        else:
            rc = call(**kw)
        assert rc == -1 and what in e.lib.pnp_last_error(), (kw, e.lib.pnp_last_error())
    odd = _engine(1, 48, 48)                                                        # a size the k-space stage refuses
    assert call(odd) == -1 and b"k-space stage" in odd.lib.pnp_last_error()
    many = _engine(32768, 16, 16)                                                   # n * coils = 65536
    assert call(many, acs_h=8, acs_w=8) == -1 and b"65535" in many.lib.pnp_last_error()
    torch.cuda.synchronize()
    assert bool((sens == 7.0).all()) and bool((ev == 7.0).all()) and bool((kern == 7.0).all()) and bool((nkept == 7).all())
    assert call(acs_h=32, acs_w=80) == 0                                            # block = plane is accepted
    with pytest.raises(ValueError, match="window"):
        e.espirit_sens(y, (16, 16), window="hamming")
    with pytest.raises(ValueError, match="coils"):
        _engine(1, 16, 16).espirit_sens(torch.zeros((1, 17, 16, 16), dtype=C64, device=DEV), (8, 8))
