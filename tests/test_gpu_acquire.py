"""The simulated acquisition on the device (pnp_acquire, PnPEngine.acquire, acquisition.simulate) against float64.

Expected values are computed here, in float64 from the exact float32 ground truth the GPU sees, with the noise of `synthetic._gauss`
(the counter hash the kernel restates); nothing is computed by the code under test.  Bounds:
  * noise alone (gt = 0): every sampled bin within ONE float32 ulp of float32(_gauss64 * sigma_n) - the device forms Box-Muller and the
    product in float64, whose libm differs from numpy's by a few float64 ulps, which can only flip the final float32 rounding; unsampled
    bins are +0.0 bit for bit;
  * y0 and ATy0: rms(err) / rms(ref) <= REL_RMS = 1e-6 (the suite's bound for its FFTs); ATy0, O(1) data: max abs <= FFT_ATOL = 3e-6;
    y0, whose DC bin is 45-180 at these sizes (one float32 ulp there is above 3e-6): max abs <= 1e-6 * max|ref|.  A float32 CPU FFT
    (pocketfft) measures 0.6-1.8e-7, <= 7.8e-8 and <= 2.8e-7 on the three: the bounds keep the ~10x margin the suite gives its FFTs.
Measured values are attached with record_property."""
import json
import os

import numpy as np
import pytest
import torch

from dt4image_restoration_amd import _lib, acquisition, data as D, synthetic

gpu = pytest.mark.gpu

FFT_ATOL = 3e-6        # FLOAT TOLERANCE: f32 FFT of O(1) data against float64 (tests/test_gpu_sizes.py)
REL_RMS = 1e-6         # rms(err) / rms(ref)
Y0_REL_MAX = 1e-6      # max abs error of y0 over max |ref|
SENTINEL = -7.25
SIDES = [16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024]
PAIRS = [(2, SIDES[i], SIDES[(i + 5) % 13]) for i in range(13)]          # every accepted side on both axes
BIG = [(64, 256, 256), (16, 512, 512)]
ACCELS = (2, 4, 8)
SIGMAS = (0.0, 5.0 / 255.0, 10.0 / 255.0, 15.0 / 255.0)
MASKS = ("radial", "cartesian")


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


def fft2c64(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.complex128)
    return np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def ifft2c64(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.complex128)
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(a, axes=(-2, -1)), norm="ortho"), axes=(-2, -1))


def noise64(seed, n, h, w, first=0) -> np.ndarray:
    """complex128 [n,h,w]: g_re + i g_im of slices first .. first + n - 1, unit variance per component (synthetic.make_problem:105)."""
    return np.stack([(synthetic._gauss(seed + first + i, 9001, h * w) + 1j * synthetic._gauss(seed + first + i, 9003, h * w)).reshape(h, w)
                     for i in range(n)])


def _c(t: torch.Tensor) -> np.ndarray:
    """[N,1,H,W,2] float32 or [N,1,H,W] complex64 on the device -> complex128 [N,H,W]."""
    t = t.cpu()
    if not t.is_complex():
        t = torch.view_as_complex(t.contiguous())
    return t.numpy().astype(np.complex128).reshape(t.shape[0], t.shape[-2], t.shape[-1])


def _errs(got: np.ndarray, ref: np.ndarray):
    d = got - ref
    mx = float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
    den = float((np.abs(ref) ** 2).mean())
    return mx, float(np.sqrt((np.abs(d) ** 2).mean() / den)) if den > 0 else 0.0


def _engine(n, h, w, **kw):
    from dt4image_restoration_amd.engine import PnPEngine
    kw.setdefault("denoiser", False)
    return PnPEngine(n, h, w, **kw)


def _phantoms(n, h, w, seed) -> np.ndarray:
    return np.stack([synthetic.phantom(h, w, seed + i) for i in range(n)]).astype(np.float32)[:, None]


def _check(d, gt32, mask, sigma, noise, fgt, record=None, tag=""):
    """One acquisition dict against float64; returns the measured (y0 max / max|ref|, y0 rel, ATy0 max, ATy0 rel)."""
    n, _, h, w = gt32.shape
    m = np.broadcast_to(np.asarray(mask, dtype=bool).reshape(-1, h, w), (n, h, w))
    y_ref = np.where(m, fgt + sigma * noise, 0.0)
    a_ref = ifft2c64(y_ref)
    y, a = _c(d["y0"]), _c(d["ATy0"])
    ymx, yrel = _errs(y, y_ref)
    amx, arel = _errs(a, a_ref)
    ymax = float(np.abs(y_ref).max())
    if record is not None:
        record(tag, f"y0 {ymx / ymax:.3e} {yrel:.3e} ATy0 {amx:.3e} {arel:.3e}")
    assert yrel <= REL_RMS and ymx <= Y0_REL_MAX * ymax, (tag, ymx, ymax, yrel)
    assert arel <= REL_RMS and amx <= FFT_ATOL, (tag, amx, arel)
    # unsampled bins are +0.0 bit for bit
    bits = torch.view_as_real(torch.view_as_complex(d["y0"].contiguous())).view(torch.int32).cpu().numpy().reshape(n, h, w, 2)
    assert not bits[~m].any(), tag
    # x0 = max(ATy0, 0) of the device's own ATy0 on both planes; x0_raw = Re ATy0
    assert torch.equal(d["x0"], d["ATy0"].clamp_min(0)), tag
    assert torch.equal(d["x0_raw"], d["ATy0"][..., 0]), tag
    assert d["x0"].shape == (n, 1, h, w, 2) and d["x0_raw"].shape == (n, 1, h, w) and d["gt"].shape == (n, 1, h, w)
    assert all(d[k].is_cuda for k in ("x0", "y0", "ATy0", "mask", "gt", "x0_raw"))
    return ymx / ymax, yrel, amx, arel


# ---- 1. noise alone ---------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("per_slice", [False, True], ids=["shared-mask", "mask-per-slice"])
@pytest.mark.parametrize("n,h,w", [(3, 128, 128), (3, 256, 64), (3, 320, 160), (2, 80, 1024)], ids=_ids([(3, 128, 128), (3, 256, 64), (3, 320, 160), (2, 80, 1024)]))
def test_noise_alone_is_make_problems_noise_to_one_ulp(n, h, w, per_slice, record_property):
    seed, sigma = 4242 + h, 10.0 / 255.0
    rng = np.random.default_rng(h * 1031 + w)
    mask = rng.random((n, h, w) if per_slice else (h, w)) < 0.4
    e = _engine(n, h, w)
    try:
        y0, aty0, x0 = e.acquire(torch.zeros((n, 1, h, w), device="cuda"), torch.from_numpy(mask).cuda(), sigma, seed)
        got = torch.view_as_real(y0).cpu().numpy().reshape(n, h, w, 2)
    finally:
        e.close()
    g = noise64(seed, n, h, w) * sigma                     # float64
    ref = np.stack([g.real, g.imag], axis=-1).astype(np.float32)
    m = np.broadcast_to(mask.reshape(-1, h, w), (n, h, w))
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    record_property("max_ulps", f"{float(ulps[m].max()):.2f}")
    record_property("share_exact", f"{float((got[m] == ref[m]).mean()):.6f}")
    assert float(ulps[m].max()) <= 1.0
    assert not got.view(np.int32)[~m].any()                # +0.0 bit for bit
    assert float((got[m] == ref[m]).mean()) > 0.99         # a rounding flip is the rare case, not the rule


# ---- 2. the full acquisition against float64 ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n,h,w", PAIRS + BIG, ids=_ids(PAIRS + BIG))
def test_acquisition_against_float64(n, h, w, record_property):
    """Both mask kinds x accel 2 / 4 / 8 x sigma_n 0 / 5 / 10 / 15 over 255 at one shape."""
    seed = 900 + h + 3 * w
    gt = _phantoms(n, h, w, seed)
    fgt = fft2c64(gt[:, 0].astype(np.float64))
    noise = noise64(seed, n, h, w)
    worst = np.zeros(4)
    e = _engine(n, h, w)
    try:
        gtd = torch.from_numpy(gt).cuda()
        for kind in MASKS:
            for accel in ACCELS:
                mask = acquisition.make_mask(h, w, accel, kind, seed=seed)
                assert mask.mean() >= 1.0 / accel - 1e-12
                md = torch.from_numpy(mask).cuda()
                for sigma in SIGMAS:
                    d = acquisition.simulate(e, gtd, md, sigma, seed)
                    tag = f"{kind}_{accel}x_{round(sigma * 255)}"
                    worst = np.maximum(worst, _check(d, gt, mask, sigma, noise, fgt, tag=tag))
                    if sigma == 0.0:                       # on the mask, y0 is the transform of gt itself
                        y = _c(d["y0"])
                        mx, rel = _errs(y[:, mask], fgt[:, mask])
                        assert rel <= REL_RMS and mx <= Y0_REL_MAX * float(np.abs(fgt).max()), (tag, mx, rel)
    finally:
        e.close()
    record_property("y0_max_over_max", f"{worst[0]:.3e}")
    record_property("y0_rel_rms", f"{worst[1]:.3e}")
    record_property("aty0_max_abs", f"{worst[2]:.3e}")
    record_property("aty0_rel_rms", f"{worst[3]:.3e}")
    print(f"acquire {n}x{h}x{w}: y0 max/max|ref| {worst[0]:.3e} rel {worst[1]:.3e}  ATy0 max {worst[2]:.3e} rel {worst[3]:.3e}")


# ---- 3. drop-in for make_problem ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n,h,w,accel,sig", [(3, 128, 128, 4, 10), (2, 320, 320, 8, 15), (2, 640, 320, 2, 5), (2, 256, 512, 4, 0)],
                         ids=["3x128x128", "2x320x320", "2x640x320", "2x256x512"])
def test_simulate_is_a_drop_in_for_make_problem(n, h, w, accel, sig, record_property):
    seed, first = 1234, 2
    p = synthetic.make_problem(n, h, w, accel=accel, sigma_n=sig / 255.0, seed=seed, first_slice=first)
    e = _engine(n, h, w)
    try:
        d = acquisition.simulate(e, p["gt"], p["mask"], sig / 255.0, seed, first_slice=first)
        for key, atol in (("y0", None), ("ATy0", FFT_ATOL), ("x0", FFT_ATOL)):
            ref = (p[key][..., 0].astype(np.float64) + 1j * p[key][..., 1].astype(np.float64)).reshape(n, h, w)
            mx, rel = _errs(_c(d[key]), ref)
            record_property(key, f"{mx:.3e} {rel:.3e}")
            assert rel <= REL_RMS, (key, rel)
            assert mx <= (Y0_REL_MAX * float(np.abs(ref).max()) if atol is None else atol), (key, mx)
        assert float(np.abs(d["x0_raw"].cpu().numpy().astype(np.float64) - p["x0_raw"]).max()) <= FFT_ATOL
        assert torch.equal(d["mask"].cpu(), torch.from_numpy(p["mask"])) and torch.equal(d["gt"].cpu(), torch.from_numpy(p["gt"]))
    finally:
        e.close()


# ---- 4. determinism and placement -----------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("h,w", [(256, 256), (128, 128), (320, 160)], ids=_ids([(256, 256), (128, 128), (320, 160)]))
def test_same_bits_whatever_the_batch_stream_or_handle_kind(h, w):
    n, a, b, seed, sigma = 8, 3, 6, 77, 10.0 / 255.0
    rng = np.random.default_rng(h + w)
    gt = torch.from_numpy(rng.random((n, 1, h, w), dtype=np.float32)).cuda()
    shared = torch.from_numpy(rng.random((h, w)) < 0.3).cuda()
    per = torch.from_numpy(rng.random((n, h, w)) < 0.3).cuda()
    e8, e3 = _engine(n, h, w), _engine(b - a, h, w)
    try:
        for mask, cut in ((shared, shared), (per, per[a:b].contiguous())):
            full = acquisition.simulate(e8, gt, mask, sigma, seed)
            again = acquisition.simulate(e8, gt, mask, sigma, seed)
            part = acquisition.simulate(e3, gt[a:b].contiguous(), cut, sigma, seed, first_slice=a)
            for k in ("y0", "ATy0", "x0", "x0_raw"):
                assert torch.equal(full[k], again[k]), k                    # two calls, the same bits
                assert torch.equal(full[k][a:b], part[k]), k                # rows [a, b) of the batch = the shard's own call
            # another seed or another slice index is another draw
            other = acquisition.simulate(e3, gt[a:b].contiguous(), cut, sigma, seed, first_slice=a + 1)
            assert not torch.equal(other["y0"], part["y0"])
            # a non-default stream
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                side = acquisition.simulate(e8, gt, mask, sigma, seed)
            st.synchronize()
            for k in ("y0", "ATy0", "x0"):
                assert torch.equal(full[k], side[k]), k
        # handle kinds: with the denoiser's planes, and in bf16 mode
        want = acquisition.simulate(e8, gt, shared, sigma, seed)
        for kw in (dict(denoiser=True), dict(denoiser=True, bf16_convs=True)):
            ek = _engine(n, h, w, **kw)
            try:
                got = acquisition.simulate(ek, gt, shared, sigma, seed)
                for k in ("y0", "ATy0", "x0"):
                    assert torch.equal(want[k], got[k]), (kw, k)
            finally:
                ek.close()
    finally:
        e8.close()
        e3.close()


# ---- 5. through the environment -----------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("h,w", [(128, 128), (160, 320)], ids=_ids([(128, 128), (160, 320)]))
def test_env_reset_takes_the_device_dict_like_its_host_copy(h, w):
    from dt4image_restoration_amd.denoiser import UNetDenoiser2D
    from dt4image_restoration_amd.env import PnPEnv
    n, seed = 3, 31
    env = PnPEnv(max_episode_step=30, denoiser=UNetDenoiser2D.seeded(0), device_type="cuda")
    gt = _phantoms(n, h, w, seed)
    dev = acquisition.simulate(env, gt, synthetic.radial_mask(h, w, 4), 10.0 / 255.0, seed)
    host = {k: v.cpu().numpy().copy() for k, v in dev.items()}
    action = {"mu": torch.tensor([0.1, 0.3, 0.5]), "sigma_d": torch.tensor([40.0, 30.0, 20.0]) / 255.0, "T": torch.zeros(n)}

    def run(mat):
        st = env.reset(mat, "cuda")
        first = {k: st[k].clone() for k in ("x", "z", "u", "y0", "mask", "gt")}
        for _ in range(3):
            st, _done = env.step(st, action)
        return first, {k: st[k].clone() for k in ("x", "z", "u")}

    f_dev, s_dev = run(dev)
    f_host, s_host = run({k: torch.from_numpy(v) for k, v in host.items()})
    for k in f_dev:
        assert torch.equal(f_dev[k], f_host[k]), k
    for k in s_dev:
        assert torch.equal(s_dev[k], s_host[k]), k
    assert float((s_dev["x"] - f_dev["x"]).abs().max()) > 1e-3        # the steps did something


# ---- 6. validation --------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("h,w", [(64, 80), (64, 128), (256, 256)], ids=_ids([(64, 80), (64, 128), (256, 256)]))
def test_argument_errors_name_the_argument_and_touch_nothing(h, w):
    """(64 x 80 runs the mixed-radix passes, the other two the power-of-two ones: with x0 but no ATy0 the inverse row pass of either
    family works in place in the scratch plane.)"""
    n = 2
    e = _engine(n, h, w)
    try:
        gt = torch.rand((n, 1, h, w), device="cuda")
        mask = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        outs = [torch.full((n, 1, h, w), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device="cuda") for _ in range(3)]
        y0, aty0, x0 = (t.data_ptr() for t in outs)
        s = e._stream()
        nan, inf = float("nan"), float("inf")
        cases = [((None, mask.data_ptr(), 1, 0.04, 5, 0, y0, aty0, x0), "null gt"),
                 ((gt.data_ptr(), None, 1, 0.04, 5, 0, y0, aty0, x0), "null mask"),
                 ((gt.data_ptr(), mask.data_ptr(), 1, 0.04, 5, 0, None, aty0, x0), "null y0"),
                 ((gt.data_ptr(), mask.data_ptr(), 3, 0.04, 5, 0, y0, aty0, x0), "mask_n must be 1 or n=2"),
                 ((gt.data_ptr(), mask.data_ptr(), 0, 0.04, 5, 0, y0, aty0, x0), "mask_n must be 1 or n=2"),
                 ((gt.data_ptr(), mask.data_ptr(), 1, -0.04, 5, 0, y0, aty0, x0), "sigma_n"),
                 ((gt.data_ptr(), mask.data_ptr(), 1, nan, 5, 0, y0, aty0, x0), "sigma_n"),
                 ((gt.data_ptr(), mask.data_ptr(), 1, inf, 5, 0, y0, aty0, x0), "sigma_n"),
                 ((gt.data_ptr(), mask.data_ptr(), 1, 0.04, 5, 1, y0, aty0, x0), "flags must be 0")]
        for args, what in cases:
            assert e.lib.pnp_acquire(e._h, *args, s) == -1, what                 # PNP_ERR_INVALID
            msg = e.lib.pnp_last_error().decode()
            assert msg.startswith("pnp_acquire:") and what in msg, msg
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == complex(SENTINEL, SENTINEL)).all())
        # the optional outputs may be left out; y0 is the same
        full = e.acquire(gt, mask, 0.04, 5)
        only = torch.empty_like(full[0])
        _lib.check(e.lib.pnp_acquire(e._h, gt.data_ptr(), mask.data_ptr(), 1, 0.04, 5, 0, only.data_ptr(), None, None, s), "pnp_acquire")
        assert torch.equal(only, full[0])
        x0_only = torch.empty_like(full[0])
        _lib.check(e.lib.pnp_acquire(e._h, gt.data_ptr(), mask.data_ptr(), 1, 0.04, 5, 0, only.data_ptr(), None, x0_only.data_ptr(), s),
                   "pnp_acquire")
        assert torch.equal(x0_only, full[2]) and torch.equal(only, full[0])
        # the Python layer's own checks
        with pytest.raises(ValueError, match="mask"):
            e.acquire(gt, torch.ones((h, w + 1), dtype=torch.uint8, device="cuda"), 0.04, 5)
        with pytest.raises(ValueError, match="seed"):
            e.acquire(gt, mask, 0.04, -1)
        with pytest.raises(ValueError, match="gt"):
            e.acquire(gt.double(), mask, 0.04, 5)
        with pytest.raises(ValueError, match="does not fit"):
            acquisition.simulate(e, torch.rand((n + 1, 1, h, w)), mask, 0.04, 5)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("h,w", [(48, 64), (128, 96), (1024, 1008)], ids=_ids([(48, 64), (128, 96), (1024, 1008)]))
def test_refused_sizes_name_the_supported_list(h, w):
    from dt4image_restoration_amd._lib import PnPError
    e = _engine(1, h, w)
    try:
        gt = torch.rand((1, 1, h, w), device="cuda")
        mask = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        outs = [torch.full((1, 1, h, w), complex(SENTINEL, SENTINEL), dtype=torch.complex64, device="cuda") for _ in range(3)]
        with pytest.raises(PnPError) as ei:
            _lib.check(e.lib.pnp_acquire(e._h, gt.data_ptr(), mask.data_ptr(), 1, 0.04, 5, 0, *(t.data_ptr() for t in outs), e._stream()),
                       "pnp_acquire")
        assert f"{h}x{w}" in str(ei.value) and ", ".join(str(s) for s in SIDES) in str(ei.value)
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == complex(SENTINEL, SENTINEL)).all())
    finally:
        e.close()


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------------------

def _json_lines(text):
    return [json.loads(line) for line in text.splitlines() if line.startswith("{")]


def _finite(v):
    return all(_finite(x) for x in v) if isinstance(v, list) else (not isinstance(v, float) or np.isfinite(v))


@gpu
def test_cli_eval_on_device_acquired_sets(tmp_path, capsys):
    from dt4image_restoration_amd import cli
    base = ["--block_size", "18", "--n_embeds", "9", "--limit", "2", "--size", "128"]
    cli.main(base + ["--acquire", "device", "eval", "--max_timesteps", "3"])
    dev = _json_lines(capsys.readouterr().out)
    cli.main(base + ["eval", "--max_timesteps", "3"])
    cpu = _json_lines(capsys.readouterr().out)
    assert len(dev) == 2 and [r["set"] for r in dev] == [r["set"] for r in cpu]
    for a, b in zip(dev, cpu):
        assert all(_finite(v) for v in a.values()) and a["n"] == 2
        # the same problems to rounding: the zero-filled PSNR the run starts from agrees closely
        assert abs((a["psnr"] - a["psnr_increment"]) - (b["psnr"] - b["psnr_increment"])) < 1e-3
    gtd = tmp_path / "gt"
    gtd.mkdir()
    np.save(gtd / "a.npy", _phantoms(2, 128, 128, 5)[:, 0])
    np.save(gtd / "b.npy", _phantoms(1, 128, 128, 9)[0, 0])
    cli.main(base + ["--gt", str(gtd), "--tasks", "4x_10,8x_5", "--mask", "cartesian", "eval", "--max_timesteps", "3"])
    rows = _json_lines(capsys.readouterr().out)
    assert [r["set"] for r in rows] == [f"{gtd} 4x_10", f"{gtd} 8x_5"]
    for r in rows:
        assert r["n"] == 2 and all(_finite(v) for v in r.values()) and 5.0 < r["psnr"] < 60.0
    cli.main(base + ["--gt", str(gtd), "--tasks", "4x_10", "fixed", "--max_iter", "3", "--dc"])
    rows = _json_lines(capsys.readouterr().out)
    assert len(rows) == 1 and all(_finite(v) for v in rows[0].values())


@gpu
def test_cli_acquire_writes_mat_files_that_load_back_as_the_device_tensors(tmp_path, capsys):
    from dt4image_restoration_amd import cli
    gtd, out = tmp_path / "gt", tmp_path / "out"
    gtd.mkdir()
    gt = _phantoms(3, 160, 128, 21)
    np.save(gtd / "vol.npy", gt[:2, 0])
    np.save(gtd / "z_last.npy", gt[2, 0])
    cli.main(["--block_size", "18", "--n_embeds", "9", "--seed", "3", "--tasks", "4x_10,8x_5", "acquire", "--gt", str(gtd),
              "--out", str(out), "--batch", "2"])
    rows = _json_lines(capsys.readouterr().out)
    assert [(r["task"], r["n"]) for r in rows] == [("4x_10", 3), ("8x_5", 3)]
    e = _engine(3, 160, 128)
    try:
        for task in ("4x_10", "8x_5"):
            files = sorted(os.listdir(out / task))
            assert len(files) == 3 and all(D.task_from_filename(f) == task for f in files)
            batch, tasks = D.load_dir(str(out / task))
            assert tasks == [task] * 3
            want = acquisition.task_problem(task, gt, e, seed=3)
            for k in ("x0", "y0", "ATy0", "gt", "x0_raw"):
                assert np.array_equal(batch[k], want[k].cpu().numpy()), (task, k)
            assert np.array_equal(batch["mask"], want["mask"].cpu().numpy())
    finally:
        e.close()
