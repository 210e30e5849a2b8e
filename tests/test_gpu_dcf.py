"""GPU checks of the density compensation (include/pnpadmm_dcf.h): pnp_nufft_psi and pnp_nufft_dcf against the float64 restatement
tests/dcf_ref.py on its three cases (13 radial spokes at 16 x 16, J = 8: coincident centre samples, wrapping footprints; a 9-petal rosette of
1500 samples at 32 x 16, J = 4; a spiral of 3064 samples at 64 x 64, J = 6: M no multiple of the gather's 256 or the finish's 2048).

Tolerances.  The library evaluates the header's float64 expressions and rounds to float32 once: 2^-24 relative.  It differs from the
restatement in the order of the sums only, which tests/test_dcf_host.py measures by a permutation of the samples (2e-15 after 30 iterations,
asserted below 2^-40).  Every term is positive, so the bound holds entry by entry: |got - ref| <= 2^-23 |ref| for Psi w and for every weight;
info (a difference |d - 1| of float64 values near 1) gets the absolute 1e-12 on top.  sum w = H W: each weight is off by at most 2^-24 of
itself, so the float64 sum of the float32 weights is within 2^-24 H W (plus the restatement's own 1e-12).

Bits: two calls, a handle of 1 slice and one of 3, with and without info; a re-plan is followed.  Either call between two steps of a live
nc, ncsense or Toeplitz episode changes no bit of the episode.  Guard bands lie around out, w and info in every call made here.
End to end: dcf_ref.FIXTURE through FixedScheduleSolver with the device's own weights, within 0.01 dB of the recorded float64 value, with the
NUFFT and with the Toeplitz normal operator; one `cli --traj spiral ... fixed` run at 64 x 64."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcf_cases as DC  # noqa: E402
import dcf_ref as D  # noqa: E402
import guard_bands as GB  # noqa: E402
import handle_cases as HC  # noqa: E402
import nufft_ref as NR  # noqa: E402
import test_gpu_ncsense as TS  # noqa: E402  (its episodes and helpers; its tests are not collected from here)
import test_gpu_nufft as TN  # noqa: E402
import test_gpu_toeplitz as TT  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL = 2.0 ** -23
CASES = range(len(D.CASES))
_np = TN._np


def _engine(n, h, w):
    from dt4image_restoration_amd.engine import PnPEngine
    return PnPEngine(n, h, w, device=0, denoiser=False)


def planned(i, n=1):
    h, w, gh, gw, J, _ = D.CASES[i]
    e = _engine(n, h, w)
    e.nufft_plan(D.case_traj(i), grid=(gh, gw), width=J)
    return e


def raw_psi(e, w):
    """pnp_nufft_psi into a guarded output, the input frozen"""
    out = GB.guarded((e.nufft_samples,), torch.float32, DEV)
    with GB.watch(outputs={"out": out}, inputs={"w": w}):
        _lib.check(e.lib.pnp_nufft_psi(e._h, w.data_ptr(), out.data_ptr(), e._stream()), "pnp_nufft_psi")
    return out


def raw_dcf(e, iters, w0=None, info=True):
    """pnp_nufft_dcf into guarded outputs, the start frozen: (w, info or None)"""
    w = GB.guarded((e.nufft_samples,), torch.float32, DEV)
    inf = GB.guarded((iters + 1,), torch.float32, DEV) if info else None
    with GB.watch(outputs={"w": w, "info": inf}, inputs={"w0": w0}):
        _lib.check(e.lib.pnp_nufft_dcf(e._h, None if w0 is None else w0.data_ptr(), iters, 0, w.data_ptr(),
                                       None if inf is None else inf.data_ptr(), e._stream()), "pnp_nufft_dcf")
    return w, inf


def _rel(got, ref):
    return float((np.abs(got - ref) / np.abs(ref)).max())


# ---- against the float64 restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", CASES)
def test_nufft_psi_against_the_float64_restatement(i):
    e, P = planned(i), D.case_plan(i)
    for name, w in (("ones", np.ones(P["m"], dtype=np.float32)), ("start", D.case_start(i))):
        ref = D.psi(P, w)
        got = _np(raw_psi(e, TN.g_f32(w)))
        print(f"case {i} {D.CASES[i]} {name}: max |Psi w - ref| / ref {_rel(got, ref):.3e} (bound {REL:.3e}), Psi w in [{ref.min():.3f}, {ref.max():.3f}]")
        assert (np.abs(got - ref) <= REL * np.abs(ref)).all()
    w = TN.g_f32(D.case_start(i))                                                   # out may alias w; the engine's own call
    want = e.nufft_psi(w)
    _lib.check(e.lib.pnp_nufft_psi(e._h, w.data_ptr(), w.data_ptr(), e._stream()), "pnp_nufft_psi")
    GB.check({"w": w})
    assert HC.differing(w, want) == 0 and HC.differing(want, raw_psi(e, TN.g_f32(D.case_start(i)))) == 0


@pytest.mark.parametrize("start", (False, True))
@pytest.mark.parametrize("i", CASES)
def test_nufft_dcf_against_the_float64_restatement(i, start):
    e = planned(i)
    h, w_ = D.CASES[i][:2]
    w0 = TN.g_f32(D.case_start(i)) if start else None
    for iters in D.ITERS:
        ref, iref = D.case_ref(i, iters, start)
        w, info = raw_dcf(e, iters, w0)
        got, igot = _np(w), _np(info)
        total = float(got.sum())
        print(f"case {i} {D.CASES[i]} start {start} iters {iters}: max |w - ref| / ref {_rel(got, ref):.3e} (bound {REL:.3e}), "
              f"max |info - ref| {np.abs(igot - iref).max():.3e}, info {igot[0]:.4f} .. {igot[-1]:.5f}, sum w - H W {total - h * w_:.3e}")
        assert (np.abs(got - ref) <= REL * np.abs(ref)).all()
        assert (np.abs(igot - iref) <= REL * iref + 1e-12).all()
        assert abs(total - h * w_) <= 2.0 ** -24 * h * w_ + 1e-12 * h * w_
        w2, none = raw_dcf(e, iters, w0, info=False)                                # info is optional and changes no bit of the weights
        assert none is None and HC.differing(w2, w) == 0
    if start:                                                                       # w may alias w0
        buf = TN.g_f32(D.case_start(i))
        _lib.check(e.lib.pnp_nufft_dcf(e._h, buf.data_ptr(), 5, 0, buf.data_ptr(), None, e._stream()), "pnp_nufft_dcf")
        GB.check({"w": buf})
        assert HC.differing(buf, raw_dcf(e, 5, w0, info=False)[0]) == 0


# ---- bits, plans, errors, workspace -----------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_the_call_or_the_batch_and_follow_the_plan():
    i = 2
    e1, e3 = planned(i, 1), planned(i, 3)
    w0 = TN.g_f32(D.case_start(i))
    a = raw_dcf(e1, 5, w0)
    for label, other in (("a second call", raw_dcf(e1, 5, w0)), ("a handle of 3 slices", raw_dcf(e3, 5, w0))):
        assert HC.differing(a[0], other[0]) == 0 and HC.differing(a[1], other[1]) == 0, label
    assert HC.differing(raw_psi(e1, w0), raw_psi(e3, w0)) == 0
    w, info = e1.nufft_dcf(iters=5, w0=w0, return_info=True)                        # the engine's methods make the same calls
    assert HC.differing(w, a[0]) == 0 and HC.differing(info, a[1]) == 0 and HC.differing(e1.nufft_dcf(5, w0), a[0]) == 0
    # another trajectory on the same handle: the result is the new plan's
    h, w_, gh, gw, J, _ = D.CASES[i]
    other = acquisition.rosette_trajectory(h, w_, 7, readout=1234)
    e1.nufft_plan(other, grid=(gh, gw), width=8)
    b = raw_dcf(e1, 5)
    f = _engine(1, h, w_)
    f.nufft_plan(other, grid=(gh, gw), width=8)
    c = raw_dcf(f, 5)
    assert b[0].shape == (1234,) and HC.differing(b[0], c[0]) == 0 and HC.differing(b[1], c[1]) == 0
    ref, iref = D.pipe(NR.plan(h, w_, gh, gw, 8, other), 5)
    assert (np.abs(_np(b[0]) - ref) <= REL * ref).all() and (np.abs(_np(b[1]) - iref) <= REL * iref + 1e-12).all()
    assert HC.differing(acquisition.pipe_dcf(e3, other, iters=5, width=8, grid=(gh, gw)), b[0]) == 0      # plans, then iterates


def test_errors_the_start_that_is_not_positive_and_workspace_accounting():
    i = 1
    h, w_, gh, gw, J, _ = D.CASES[i]
    m = D.case_traj(i).shape[0]
    e = _engine(2, h, w_)
    lib, hd, st = e.lib, e._h, e._stream()
    w0 = TN.g_f32(D.case_start(i))
    out, info = GB.guarded((m,), torch.float32, DEV), GB.guarded((31,), torch.float32, DEV)
    ws0 = e.workspace_bytes
    with GB.watch(outputs={"out": out, "info": info}, inputs={"out": out, "info": info, "w0": w0}):
        # without a plan: PNP_ERR_INVALID, and the message names the plan
        assert lib.pnp_nufft_psi(hd, w0.data_ptr(), out.data_ptr(), st) == -1 and b"no NUFFT plan (pnp_nufft_plan)" in lib.pnp_last_error()
        assert lib.pnp_nufft_dcf(hd, w0.data_ptr(), 30, 0, out.data_ptr(), info.data_ptr(), st) == -1
        assert b"pnp_nufft_dcf: the handle has no NUFFT plan (pnp_nufft_plan)" in lib.pnp_last_error()
    for call in (lambda: e.nufft_psi(w0), lambda: e.nufft_dcf(3), lambda: e.nufft_dcf(3, w0, return_info=True)):
        with pytest.raises(_lib.PnPError, match="no NUFFT plan"):
            call()
    assert e.workspace_bytes == ws0
    e.nufft_plan(D.case_traj(i), grid=(gh, gw), width=J)
    ws0 = e.workspace_bytes
    bad = [(lambda: lib.pnp_nufft_dcf(hd, w0.data_ptr(), 0, 0, out.data_ptr(), info.data_ptr(), st), "iters"),
           (lambda: lib.pnp_nufft_dcf(hd, w0.data_ptr(), 257, 0, out.data_ptr(), info.data_ptr(), st), "iters"),
           (lambda: lib.pnp_nufft_dcf(hd, w0.data_ptr(), 30, 4, out.data_ptr(), info.data_ptr(), st), "flags"),
           (lambda: lib.pnp_nufft_dcf(hd, w0.data_ptr(), 30, 0, None, info.data_ptr(), st), "null w"),
           (lambda: lib.pnp_nufft_psi(hd, None, out.data_ptr(), st), "null w"),
           (lambda: lib.pnp_nufft_psi(hd, w0.data_ptr(), None, st), "null out")]
    with GB.watch(outputs={"out": out, "info": info}, inputs={"out": out, "info": info, "w0": w0}):
        for call, what in bad:
            assert call() == -1 and what.encode() in lib.pnp_last_error(), (what, lib.pnp_last_error())
    for call in (lambda: e.nufft_dcf(0), lambda: e.nufft_dcf(257)):
        with pytest.raises(_lib.PnPError, match="iters must be 1..256"):
            call()
    assert e.workspace_bytes == ws0
    # the workspace is the feature's own: the grid 8 gh gw, w in float64 8 M, the chunk sums 8 ceil(M / 2048); the maxima only with info
    raw_psi(e, w0)
    want = 8 * gh * gw + 8 * m + 8 * ((m + 2047) // 2048)
    print(f"pnp_nufft_psi grew the workspace by {e.workspace_bytes - ws0} bytes, documented {want}")
    assert e.workspace_bytes - ws0 == want
    raw_dcf(e, 30, w0, info=False)
    assert e.workspace_bytes - ws0 == want
    raw_dcf(e, 30, w0)
    assert e.workspace_bytes - ws0 == want + 4 * 31 * ((m + 255) // 256)
    raw_dcf(e, 5, w0)
    raw_psi(e, w0)
    assert e.workspace_bytes - ws0 == want + 4 * 31 * ((m + 255) // 256)
    # a start that is not positive and finite: the Python layer refuses it; the library reads such an entry as 1, so nothing spreads
    start = D.case_start(i)
    poisoned, mended = start.copy(), start.copy()
    poisoned[[0, 7, 700, 1499]] = (0.0, -2.0, np.nan, np.inf)
    mended[[0, 7, 700, 1499]] = 1.0
    for call in (lambda: e.nufft_dcf(3, HC.f32(poisoned)), lambda: e.nufft_psi(HC.f32(poisoned))):
        with pytest.raises(ValueError, match="positive and finite"):
            call()
    a, b = raw_dcf(e, 5, TN.g_f32(poisoned)), raw_dcf(e, 5, TN.g_f32(mended))
    assert HC.differing(a[0], b[0]) == 0 and HC.differing(a[1], b[1]) == 0
    assert torch.isfinite(a[0]).all() and (a[0] > 0).all() and torch.isfinite(a[1]).all()
    assert HC.differing(raw_psi(e, TN.g_f32(poisoned)), raw_psi(e, TN.g_f32(mended))) == 0


# ---- between two steps of a live episode ------------------------------------------------------------------------------------------------------

def _both_calls(e, f):
    """the two entry points on foreign weights of the live plan's length"""
    _, wts = f.samples(e.nufft_samples)
    w, info = e.nufft_dcf(iters=3, w0=wts, return_info=True)
    return {"psi": e.nufft_psi(wts), "dcf": (w, info), "dcf ones": e.nufft_dcf(iters=2)}


@pytest.mark.parametrize("mode", ("nc", "ns") + TT.TZ)
def test_the_two_calls_between_two_steps_of_an_episode_change_nothing(mode):
    ep = TT._episode(mode)
    f = HC.Foreign(ep.n, ep.h, ep.w)
    calls = set()
    e = HC.record(TS._tv(TT._engine(ep.n, ep.h, ep.w)), calls)
    outs = []

    def between():
        outs.append(_both_calls(e, f))
        assert e.toeplitz_live == (mode in TT.TZ)

    got = TS._steps(e, ep, ep.reset(e), 0, 2, between=between)
    TS._assert_same(got, TT.fresh(mode), f"{mode} with the density compensation between two steps")
    assert set(DC.ENTRY_POINTS) <= calls
    bare = TT._engine(ep.n, ep.h, ep.w)                                             # what they return does not depend on the episode either
    ep.plan(bare)
    HC.compare_outputs(outs[0], _both_calls(bare, f), f"the two calls in a {mode} episode")


# ---- end to end, and the command line --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc_normal", ("nufft", "toeplitz"))
def test_end_to_end_spiral_tv_admm_through_the_fixed_schedule_solver_with_the_devices_own_weights(nc_normal, record_property):
    from dt4image_restoration_amd.denoiser import TVDenoiser2D
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    from dt4image_restoration_amd.env import PnPEnv
    import tv_ref
    t = D.FIXTURE
    d, P = D.fixture_problem()
    mu, sig = D.fixture_schedules()
    env = PnPEnv(max_episode_step=t["iters"], denoiser=TVDenoiser2D(scale=t["tv_scale"], iters=t["tv_iters"]), device_type="cuda",
                 cg_iters=t["cg_iters"], nufft_width=t["width"], nc_normal=nc_normal)
    env._engine_for(t["n"], t["h"], t["w"], torch.device("cuda", 0))               # the handle the episode will run on
    wdev = acquisition.pipe_dcf(env, d["traj"], iters=t["dcf_iters"], width=t["width"])
    ref = D.pipe(P, t["dcf_iters"])[0]
    assert (np.abs(_np(wdev) - ref) <= REL * ref).all()
    mat = TN._mat(d)
    mat["dcf"] = wdev                                                               # the device's own weights
    r = FixedScheduleSolver(env, max_iter=t["iters"], dc=True).run(mat, np.tile(mu, (t["n"], 1)), np.tile(sig, (t["n"], 1)))
    assert env._engine.toeplitz_live == (nc_normal == "toeplitz")
    gt = d["gt"][:, 0].astype(np.float64)
    pdev = tv_ref.psnr(_np(r.x)[:, 0], gt)
    dp = float(np.abs(pdev - D.FIXTURE_PSNR[1]).max())
    print(f"{nc_normal}: device PSNR of x0 {r.initial_psnr.reshape(-1).tolist()}, final {pdev} (engine's own {r.psnr.reshape(-1).tolist()}), "
          f"recorded float64 {D.FIXTURE_PSNR}, |dPSNR| {dp:.3e} dB, dc {r.dc.tolist()}")
    record_property("max_abs_dpsnr_db", dp)
    assert dp <= 0.01
    assert abs(float(r.psnr.reshape(-1)[0]) - D.FIXTURE_PSNR[1]) <= 0.01


def test_cli_traj_spiral_fixed_on_a_ground_truth_folder(tmp_path):
    from dt4image_restoration_amd import cli
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", np.stack([synthetic.phantom(64, 64, 5), synthetic.phantom(64, 64, 6)]).astype(np.float32))
    base = ["--block_size", "6", "--n_embeds", "9", "--gt", str(gtd), "--tasks", "4x_5", "--prior", "tv", "--seed", "3"]

    def run(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = cli.main(base + extra + ["fixed", "--max_iter", "10", "--dc"])
        lines = [json.loads(l) for l in buf.getvalue().splitlines() if l.startswith("{")]
        assert lines == out and len(out) == 1 and out[0]["n"] == 2
        return out[0]

    a = run(["--traj", "spiral", "--interleaves", "8"])                            # dcf on a spiral: the iterated weights
    b = run(["--traj", "spiral", "--interleaves", "8", "--nc-weights", "pipe", "--dcf-iters", "30"])
    c = run(["--traj", "spiral", "--interleaves", "8", "--nc-weights", "none"])
    r = run(["--traj", "rosette", "--petals", "17", "--nc-normal", "toeplitz", "--nc-coils", "2"])
    print(f"cli --traj spiral fixed: {a['psnr']:.3f} dB (+{a['psnr_increment']:.3f}), without weights {c['psnr']:.3f} dB "
          f"(+{c['psnr_increment']:.3f}); --traj rosette --nc-normal toeplitz --nc-coils 2: {r['psnr']:.3f} dB (+{r['psnr_increment']:.3f})")
    assert "spiral-nc" in a["set"] and "spiral-nc" in c["set"] and "rosette-nc" in r["set"]
    assert a["psnr"] == b["psnr"] and a["dc"] == b["dc"]                            # dcf and pipe are the same weights off the radial trajectory
    assert a["dc"] != c["dc"]                                                       # ... and --nc-weights none is not
    for x in (a, c, r):
        assert np.isfinite(x["psnr"]) and x["dc"] > 0.0
    assert a["psnr_increment"] > 1.0
    assert sorted(DC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_DCF)
