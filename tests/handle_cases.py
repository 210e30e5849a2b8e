"""One table of the C ABI's entry points by what they may do to a running episode, and the episodes, foreign data and calls the handle-level
GPU tests are built from (no test in here).

ENTRY_POINTS classifies every `pnp_*` function of include/pnpadmm.h:
  INTRUDER   must not disturb: between two steps of an episode it changes neither the iterate's future nor the installed constants
  REPLACES   documented to replace the episode's constants (or the plan they hang on); the matching pnp_set_kspace* puts them back
  STEP       the episode itself: pnp_step, and pnp_prox_dual, the half of it tests/test_gpu_step_composition.py composes a step from.  In the
             CG modes pnp_prox_dual rewrites the solve's scalars (pnp_mc_cg_residual reads them), so it cannot be an intruder
  STATELESS  takes no device state: create, destroy, version, last_error, the getters, the profile calls, pnp_load_unet_weights
tests/test_entry_point_table_host.py requires that the table and the header name the same functions and that every INTRUDER, REPLACES and
STEP entry is covered by a call listed below; tests/test_gpu_handle_noninterference.py runs INTRUDERS and REPLACERS - built from this
table - records every library call its handles make, and requires the recorded names to contain what the lists say they cover.

Episodes (make_episode): single-coil ("sc"), multi-coil ("mc", tests/sense_ref.solve_case: per-slice maps and masks) and non-Cartesian
("nc", 13 golden-angle spokes, J = 6, the default 1.25x grid) problems of synthetic phantoms.  Foreign: unrelated data of another seed,
another mask, 2 and 8 coils (fewer and more than an episode's 4), another trajectory."""
from __future__ import annotations

import re

import numpy as np

INTRUDER = "intruder: must not disturb"
REPLACES = "replaces the episode's constants"
STEP = "the episode itself"
STATELESS = "takes no device state"

ENTRY_POINTS = {
    "pnp_create": STATELESS, "pnp_destroy": STATELESS, "pnp_last_error": STATELESS, "pnp_version": STATELESS,
    "pnp_load_unet_weights": STATELESS,
    "pnp_reset": REPLACES, "pnp_set_kspace": REPLACES,
    "pnp_step": STEP, "pnp_prox_dual": STEP,
    "pnp_denoise": INTRUDER, "pnp_tv_denoise": INTRUDER, "pnp_haar_denoise": INTRUDER,
    "pnp_set_prior": INTRUDER, "pnp_get_prior": STATELESS, "pnp_set_prior_haar": INTRUDER, "pnp_get_prior_haar": STATELESS,
    "pnp_fft2c": INTRUDER, "pnp_psnr": INTRUDER, "pnp_ssim": INTRUDER, "pnp_residuals": INTRUDER,
    "pnp_acquire": INTRUDER,
    "pnp_set_kspace_mc": REPLACES, "pnp_reset_mc": REPLACES, "pnp_mc_coils": STATELESS, "pnp_mc_cg_residual": INTRUDER,
    "pnp_mc_normal": INTRUDER, "pnp_acquire_mc": INTRUDER,
    "pnp_nufft_plan": REPLACES, "pnp_nufft_samples": STATELESS, "pnp_nufft_grid": STATELESS,
    "pnp_nufft_forward": INTRUDER, "pnp_nufft_adjoint": INTRUDER,
    "pnp_set_kspace_nc": REPLACES, "pnp_reset_nc": REPLACES, "pnp_nc_cg_residual": INTRUDER, "pnp_nc_normal": INTRUDER,
    "pnp_acquire_nc": INTRUDER,
    "pnp_estimate_sens": INTRUDER, "pnp_coil_compress_matrix": INTRUDER, "pnp_coil_compress_apply": INTRUDER,
    "pnp_noise_cov": INTRUDER, "pnp_whiten_matrix": INTRUDER, "pnp_whiten_apply": INTRUDER,
    "pnp_espirit_sens": INTRUDER, "pnp_grappa_weights": INTRUDER, "pnp_grappa_apply": INTRUDER,
    "pnp_snapshot_bytes": STATELESS, "pnp_snapshot": INTRUDER, "pnp_restore": INTRUDER,
    "pnp_unet_read_stage": INTRUDER,
    "pnp_profile_reset": STATELESS, "pnp_profile_collect": STATELESS, "pnp_profile_layers": STATELESS,
    "pnp_conv_algorithms": STATELESS, "pnp_conv_schedules": STATELESS, "pnp_bf16_weight_terms": STATELESS, "pnp_workspace_bytes": STATELESS,
}


def header_functions(text: str):
    """every function include/pnpadmm.h declares: `<type> pnp_name(` at the start of a line (comments are indented or start with ` *`)"""
    return sorted(set(re.findall(r"^(?:const\s+)?[A-Za-z_][A-Za-z_0-9]*\s*\*?\s*(pnp_[a-z0-9_]+)\s*\(", text, flags=re.M)))


# ---- bits ------------------------------------------------------------------------------------------------------------------------------
def bits(t):
    """the tensor as integers: float32 / complex64 -> int32, float64 / complex128 -> int64, integer types as they are"""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def differing(a, b) -> int:
    """elements of a and b whose bits differ (shapes must agree)"""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum())


def flat_outputs(out):
    """[(name, tensor-or-value)] of an intruder's result: a dict whose values are tensors, tuples of tensors, or plain values"""
    import torch
    flat = []
    for k, v in out.items():
        for i, t in enumerate(v if isinstance(v, (tuple, list)) and any(isinstance(q, torch.Tensor) for q in v) else (v,)):
            flat.append((f"{k}[{i}]", t))
    return flat


def compare_outputs(got, want, label):
    """every output of two runs of one call, bit for bit; returns the number of elements compared"""
    import torch
    g, w = flat_outputs(got), flat_outputs(want)
    assert [k for k, _ in g] == [k for k, _ in w], label
    count = 0
    for (k, a), (_, b) in zip(g, w):
        if isinstance(a, torch.Tensor):
            d = differing(a, b)
            assert d == 0, f"{label}: {k} differs in {d} of {a.numel()} elements"
            count += a.numel()
        else:
            assert a == b, f"{label}: {k}: {a!r} != {b!r}"
            count += 1
    return count


class Recorder:
    """stands in for an engine's `lib`: every pnp_* function fetched from it is noted in `calls` by name when it is called"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pnp_"):
            return fn

        def call(*a):
            self._calls.add(name)
            return fn(*a)
        return call


def record(engine, calls):
    engine.lib = Recorder(engine.lib, calls)
    return engine


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def c64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.complex64).cuda()


def f32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).cuda()


def u8(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).cuda()


def _uniform(seed, stream, shape):
    from dt4image_restoration_amd.weights import hash_uniform
    return hash_uniform(seed, stream, int(np.prod(shape))).astype(np.float64).reshape(shape)


def _cuniform(seed, stream, shape):
    return _uniform(seed, stream, shape) + 1j * _uniform(seed, stream + 1, shape)


def _pack(a):
    return a[..., 0] + 1j * a[..., 1]


class Episode:
    """The constants and the start of one episode on the device.  mode "sc": y [n,1,h,w], mask [n,h,w]; "mc": y [n,C,h,w], sens [n,C,h,w],
    mask [n,h,w]; "nc": y [n,M], traj float64 [M,2] (host), dcf [M]."""

    def __init__(self, mode, n, h, w, x0, y, mask=None, sens=None, traj=None, dcf=None, cg_iters=4):
        self.mode, self.n, self.h, self.w = mode, n, h, w
        self.x0, self.y, self.mask, self.sens, self.traj, self.dcf, self.cg_iters = x0, y, mask, sens, traj, dcf, cg_iters

    def plan(self, e):
        if self.mode == "nc" and not e.nufft_planned(self.traj, None, 6):
            e.nufft_plan(self.traj, width=6)

    def reset(self, e):
        """install the constants and start the iterate: (x, z, u)"""
        if self.mode == "nc":
            self.plan(e)
            return e.reset_nc(self.x0, self.y, self.dcf, cg_iters=self.cg_iters)
        return e.reset(self.x0, self.y, self.mask, sens=self.sens, cg_iters=self.cg_iters)

    def reinstall(self, e):
        """the constants only, by the matching pnp_set_kspace*, re-planning first where the plan is another's"""
        if self.mode == "nc":
            self.plan(e)
            e.set_kspace_nc(self.y, self.dcf, cg_iters=self.cg_iters)
        else:
            e.set_kspace(self.y, self.mask, sens=self.sens, cg_iters=self.cg_iters)

    def cg_residual(self, e):
        return None if self.mode == "sc" else (e.cg_residual() if self.mode == "mc" else e.nc_cg_residual())


_episode_cache = {}


def make_episode(mode, n, h, w, seed=11, coils=4, spokes=13):
    """the host arrays are made once per argument set; every call uploads fresh device tensors"""
    from dt4image_restoration_amd import acquisition, synthetic
    key = (mode, n, h, w, seed, coils, spokes)
    if key not in _episode_cache:
        if mode == "sc":
            # per-slice masks (mask_n = n): slice i is sampled by a radial mask of acceleration 4 + i
            gt = np.stack([synthetic.phantom(h, w, seed + (i % 4)) for i in range(n)])
            masks = {a: synthetic.radial_mask(h, w, 4.0 + a) for a in range(min(n, 3))}
            mask = np.stack([masks[i % 3] for i in range(n)])
            noise = _cuniform(seed, 71, (n, h, w)) * (10.0 / 255.0)
            y = mask * (synthetic.fft2c_np(gt) + noise)
            aty = synthetic.ifft2c_np(y)
            x0 = np.maximum(aty.real, 0) + 1j * np.maximum(aty.imag, 0)
            _episode_cache[key] = dict(x0=x0[:, None], y=y[:, None], mask=mask)
        elif mode == "mc":
            import sense_ref
            cs = sense_ref.solve_case(h, w, coils, True, "radial", 4, n=n, seed=seed)
            _episode_cache[key] = dict(x0=cs["z0"][:, None], y=cs["y"], mask=cs["mask"], sens=cs["sens"])
        else:
            import nufft_ref
            traj = nufft_ref.radial(h, w, spokes)
            d = synthetic.make_problem_nc(n, h, w, traj, dcf=acquisition.radial_dcf(traj, h, w), seed=seed)
            _episode_cache[key] = dict(x0=_pack(d["x0"]), y=_pack(d["y0"])[:, 0], traj=traj, dcf=d["dcf"])
    d = _episode_cache[key]
    return Episode(mode, n, h, w, c64(d["x0"]), c64(d["y"]), mask=u8(d["mask"]) if "mask" in d else None,
                   sens=c64(d["sens"]) if "sens" in d else None, traj=d.get("traj"), dcf=f32(d["dcf"]) if "dcf" in d else None)


def step_params(n, t, stop=None):
    """(mu, sigma_d, t_action) of step t on the device: per-slice values that differ between slices; slice `stop` stopped"""
    import torch
    mu = torch.tensor([0.12 + 0.07 * t + 0.05 * i for i in range(n)], dtype=torch.float32).cuda()
    sigma = torch.tensor([(40.0 - 6.0 * t - 1.5 * (i % 5)) / 255.0 for i in range(n)], dtype=torch.float32).cuda()
    tact = torch.zeros(n, dtype=torch.float32)
    if stop is not None:
        tact[stop] = 1.0
    return mu, sigma, tact.cuda()


COILS = (2, 8)                # the intruders' coil counts: fewer and more than the episode's 4, so the coil scratch grows mid-episode
ACS = (16, 16)


class Foreign:
    """Unrelated data of one handle shape (another seed, another mask, 2 and 8 coils, another trajectory), on the device"""

    def __init__(self, n, h, w, seed=901):
        import nufft_ref
        from dt4image_restoration_amd import synthetic
        self.n, self.h, self.w = n, h, w
        self.gt = f32((_uniform(seed, 1, (n, 1, h, w)) + 1) * 0.5)
        self.img = f32((_uniform(seed, 2, (n, 1, h, w)) + 1) * 0.5)
        self.cimg = c64(_cuniform(seed, 3, (n, h, w)))
        self.lam = f32(np.linspace(0.03, 0.12, n))
        self.mu = f32(np.linspace(0.2, 0.45, n))
        # a comb of every second column (offset 1) with a fully sampled centre block: also GRAPPA's geometry at accel 2
        cols = (np.arange(w) % 2 == 1) | (np.abs(np.arange(w) - w // 2) < ACS[1] // 2 + 1)
        mask1 = np.broadcast_to(cols, (h, w)).copy()
        self.mask1 = u8(mask1)
        self.maskn = u8(np.stack([np.roll(mask1, 2 * i, axis=1) | mask1 for i in range(n)]))
        self.y1 = c64(mask1 * _cuniform(seed, 5, (n, 1, h, w)))
        self.x1 = c64(_cuniform(seed, 7, (n, 1, h, w)) * 0.5)
        self.sens = {c: c64(synthetic.coil_maps(c, h, w, radius=1.5, width=1.0)) for c in COILS}
        self.yc = {c: c64(mask1 * _cuniform(seed, 10 + c, (n, c, h, w))) for c in COILS}
        self.noise = {c: c64(_cuniform(seed, 30 + c, (c, 256))) for c in COILS}
        self.traj = nufft_ref.radial(h, w, 7, golden=False)
        self._samples = {}
        self.seed = seed

    def samples(self, m):
        if m not in self._samples:
            self._samples[m] = (c64(_cuniform(self.seed, 50, (self.n, m))), f32((_uniform(self.seed, 52, (m,)) + 1.5) * 0.5))
        return self._samples[m]


class Ctx:
    """what an intruder is handed beside the engine: the foreign data, the episode's mode, and the live iterate (read only)"""

    def __init__(self, foreign, mode, iterate, unet, keep_stages):
        self.f, self.mode, self.iterate, self.unet, self.keep_stages = foreign, mode, iterate, unet, keep_stages


# ---- raw calls with optional outputs left out ------------------------------------------------------------------------------------------
def _acquire_variants(call, n, h, w, y_shape):
    """`call(y, aty0, x0)` with both optional outputs, without aty0 (the sum then lives in the handle's scratch), and without either"""
    import torch
    from dt4image_restoration_amd import _lib
    out = {}
    for name, want_aty, want_x0 in (("full", True, True), ("no_aty0", False, True), ("y_only", False, False)):
        y = torch.empty(y_shape, dtype=torch.complex64, device="cuda")
        aty = torch.empty((n, 1, h, w), dtype=torch.complex64, device="cuda") if want_aty else None
        x0 = torch.empty((n, 1, h, w), dtype=torch.complex64, device="cuda") if want_x0 else None
        _lib.check(call(y.data_ptr(), None if aty is None else aty.data_ptr(), None if x0 is None else x0.data_ptr()), name)
        out[name] = tuple(t for t in (y, aty, x0) if t is not None)
    return out


def i_fft2c(e, c):
    f, out = c.f, {}
    for inverse in (False, True):
        out[f"n inv={inverse}"] = e.fft2c(f.cimg, inverse=inverse)
        if f.n > 1:
            out[f"n-1 inv={inverse}"] = e.fft2c(f.cimg[:f.n - 1].contiguous(), inverse=inverse)
    return out


def i_metrics(e, c):
    return {"psnr": e.psnr(c.f.img, c.f.gt), "ssim": e.ssim(c.f.img, c.f.gt, return_map=True)}


def i_state(e, c):
    import torch
    x, z, u, t = c.iterate
    snap = e.snapshot(x, z, u, t)
    out = {"snapshot": snap}
    for prev in (None, snap):
        for dc in (False, True):
            out[f"residuals prev={prev is not None} dc={dc}"] = e.residuals(x, z, u, prev=prev, dc=dc)
    sx, sz, su, st = torch.zeros_like(x), torch.zeros_like(z), torch.zeros_like(u), torch.zeros_like(t)
    e.restore(snap, sx, sz, su, st)
    out["restore"] = (sx, sz, su, st)
    return out


def i_priors(e, c):
    """the prior switched to each of the others and back; the stored settings read back unchanged"""
    before = (e.prior_settings(), e.haar_settings())
    prior, tv_scale, tv_iters = before[0]
    seen = []
    for other in ("tv", "haar", "unet"):
        if other == prior or (other == "unet" and not c.unet):
            continue
        if other == "tv":
            e.set_prior("tv", tv_scale, tv_iters)
        elif other == "haar":
            e.set_haar_prior(*before[1])
        else:
            e.set_prior("unet")
        seen.append(e.prior)
    if prior == "haar":
        e.set_haar_prior(*before[1])
    else:
        e.set_prior(prior, tv_scale, tv_iters)
    assert (e.prior_settings(), e.haar_settings()) == before, (before, e.prior_settings(), e.haar_settings())
    return {"visited": tuple(seen), "settings": before}


def i_denoise(e, c):
    f = c.f
    out = {"tv": e.tv_denoise(f.img, f.lam, 11), "haar ti": e.haar_denoise(f.img, f.lam, 3, "ti"), "haar ortho": e.haar_denoise(f.img, f.lam, 2, "ortho")}
    if c.unet:
        out["unet"] = e.denoise(f.img, f.lam)
        if c.keep_stages:
            out["stage"] = e.read_stage(0)
    return out


def i_acquire(e, c):
    f = c.f
    call = lambda y, a, x: e.lib.pnp_acquire(e._h, f.gt.data_ptr(), f.mask1.data_ptr(), 1, 0.02, 4242, 0, y, a, x, e._stream())
    return _acquire_variants(call, f.n, f.h, f.w, (f.n, 1, f.h, f.w))


def i_acquire_mc(e, c):
    f, out = c.f, {}
    for coils in COILS:
        s = f.sens[coils]
        call = lambda y, a, x: e.lib.pnp_acquire_mc(e._h, f.gt.data_ptr(), s.data_ptr(), coils, 1, f.maskn.data_ptr(), f.n, 0.02, 77, 0, y, a, x,
                                                    e._stream())
        out.update({f"C={coils} {k}": v for k, v in _acquire_variants(call, f.n, f.h, f.w, (f.n, coils, f.h, f.w)).items()})
    return out


def i_nufft(e, c):
    """the NUFFT pair and the non-Cartesian acquisition: on the live plan in non-Cartesian mode, and on a single- or multi-coil handle
    that merely holds a plan (made here: pnp_nufft_plan leaves Cartesian and multi-coil constants alone)"""
    f = c.f
    if c.mode != "nc":
        e.nufft_plan(f.traj, width=4)
    m = e.nufft_samples
    samples, wts = f.samples(m)
    out = {"forward": e.nufft_forward(f.cimg), "adjoint": e.nufft_adjoint(samples), "adjoint w": e.nufft_adjoint(samples, wts)}
    if f.n > 1:
        out["forward n-1"] = e.nufft_forward(f.cimg[:f.n - 1].contiguous())
    call = lambda y, a, x: e.lib.pnp_acquire_nc(e._h, f.gt.data_ptr(), wts.data_ptr(), 0.02, 99, 0, y, a, x, e._stream())
    out.update({f"acquire_nc {k}": v for k, v in _acquire_variants(call, f.n, f.h, f.w, (f.n, m)).items()})
    return out


def i_calibration(e, c):
    f, out = c.f, {}
    for coils in COILS:
        y = f.yc[coils]
        out[f"C={coils} estimate_sens"] = e.estimate_sens(y, ACS, window="hann", thresh=0.05)
        out[f"C={coils} estimate_sens rss"] = e.estimate_sens(y, ACS, window="box", return_rss=True)
        out[f"C={coils} espirit"] = e.espirit_sens(y, ACS, ksize=3, iters=4, crop=0.5, thresh=0.05, return_eval=True)
        cmat, eig = e.coil_compress_matrix(y, ACS)
        out[f"C={coils} compress"] = (cmat, eig, e.coil_compress_apply(y, cmat, max(1, coils // 2)))
        psi = e.noise_cov(f.noise[coils])
        wmat, lmat, info = e.whiten_matrix(psi)
        out[f"C={coils} whiten"] = (psi, wmat, lmat, info, e.whiten_apply(y, wmat))
        wts, ginfo = e.grappa_weights(y, ACS, 2, kernel=(3, 2))
        out[f"C={coils} grappa"] = (wts, ginfo, e.grappa_apply(y, wts, f.mask1, 2, 1, kernel=(3, 2)))
    return out


def i_operators(e, c):
    f = c.f
    if c.mode == "mc":
        return {"normal_op": e.normal_op(f.x1, f.mu)}
    return {"nc_normal": e.nc_normal(f.x1, f.mu)}


# (name, the entry points it covers, the modes / handles it runs on, the call).  The order is the order of a round.
INTRUDERS = [
    ("fft2c", ("pnp_fft2c",), lambda c: True, i_fft2c),
    ("metrics", ("pnp_psnr", "pnp_ssim"), lambda c: True, i_metrics),
    ("state", ("pnp_snapshot", "pnp_restore", "pnp_residuals"), lambda c: True, i_state),
    ("priors", ("pnp_set_prior", "pnp_set_prior_haar"), lambda c: True, i_priors),
    ("denoise", ("pnp_tv_denoise", "pnp_haar_denoise"), lambda c: not c.unet, i_denoise),
    ("denoise unet", ("pnp_tv_denoise", "pnp_haar_denoise", "pnp_denoise"), lambda c: c.unet and not c.keep_stages, i_denoise),
    ("denoise unet stages", ("pnp_tv_denoise", "pnp_haar_denoise", "pnp_denoise", "pnp_unet_read_stage"), lambda c: c.unet and c.keep_stages, i_denoise),
    ("acquire", ("pnp_acquire",), lambda c: True, i_acquire),
    ("acquire_mc", ("pnp_acquire_mc",), lambda c: True, i_acquire_mc),
    ("nufft", ("pnp_nufft_forward", "pnp_nufft_adjoint", "pnp_acquire_nc"), lambda c: True, i_nufft),
    ("calibration", ("pnp_estimate_sens", "pnp_espirit_sens", "pnp_coil_compress_matrix", "pnp_coil_compress_apply", "pnp_noise_cov",
                     "pnp_whiten_matrix", "pnp_whiten_apply", "pnp_grappa_weights", "pnp_grappa_apply"), lambda c: True, i_calibration),
    ("mc operator", ("pnp_mc_normal",), lambda c: c.mode == "mc", i_operators),
    ("nc operator", ("pnp_nc_normal",), lambda c: c.mode == "nc", i_operators),
]
# what the test itself calls after every step to compare the two handles: the remaining intruders, and the episode's own entry point
CHECKS = {"sc": ("pnp_step", "pnp_residuals"), "mc": ("pnp_step", "pnp_residuals", "pnp_mc_cg_residual"),
          "nc": ("pnp_step", "pnp_residuals", "pnp_nc_cg_residual")}
# pnp_prox_dual: tests/test_gpu_step_composition.py (every case ends in it)
COMPOSITION = ("pnp_step", "pnp_prox_dual")


# ---- the entry points that replace the constants ---------------------------------------------------------------------------------------
def r_reset(e, f):
    e.reset(f.x1, f.y1, f.mask1)


def r_set_kspace(e, f):
    e.set_kspace(f.y1, f.maskn)


def r_reset_mc(e, f):
    e.reset(f.x1, f.yc[8], f.mask1, sens=f.sens[8], cg_iters=2)


def r_set_kspace_mc(e, f):
    e.set_kspace(f.yc[2], f.maskn, sens=f.sens[2], cg_iters=3)


def r_nufft_plan(e, f):
    e.nufft_plan(f.traj, width=4)


def r_reset_nc(e, f):
    if not e.nufft_samples:
        e.nufft_plan(f.traj, width=4)
    samples, wts = f.samples(e.nufft_samples)
    e.reset_nc(f.x1, samples, wts, cg_iters=2)


def r_set_kspace_nc(e, f):
    if not e.nufft_samples:
        e.nufft_plan(f.traj, width=4)
    samples, _ = f.samples(e.nufft_samples)
    e.set_kspace_nc(samples, None, cg_iters=3)


# every one runs in every mode: a handle in mode a visits mode b and comes back, for the whole 3 x 3 grid
REPLACERS = [
    ("reset", ("pnp_reset",), r_reset), ("set_kspace", ("pnp_set_kspace",), r_set_kspace),
    ("reset_mc", ("pnp_reset_mc",), r_reset_mc), ("set_kspace_mc", ("pnp_set_kspace_mc",), r_set_kspace_mc),
    ("nufft_plan", ("pnp_nufft_plan",), r_nufft_plan), ("reset_nc", ("pnp_reset_nc",), r_reset_nc),
    ("set_kspace_nc", ("pnp_set_kspace_nc",), r_set_kspace_nc),
]


def covered():
    """every entry point the lists above say part A and part B call"""
    out = set(COMPOSITION)
    for _, names, _, _ in INTRUDERS:
        out.update(names)
    for _, names, _ in REPLACERS:
        out.update(names)
    for names in CHECKS.values():
        out.update(names)
    return out
