"""Field map estimation (include/pnpadmm_fieldmap.h) without a GPU: the header, the table and the binding; the argument validation through
ctypes and through the stand-alone sanitizer program tests/asan_fieldmap_host.cpp (`make asan_fieldmap`: a CPU build with its own main,
nothing preloaded); the restatement tests/fieldmap_ref.py against itself - descent of Psi, the fixed points, float32 against float64 - and
"the estimate helps" in float64, which produces the PSNR figures the GPU test is held to; the Python layers on a fake engine; the CLI's
argument checks.  Every figure is printed before it is asserted.

MEASURED (float64 restatement, tests/offres_ref.py's fixture, dte = 2 ms, scan noise 5/255, beta = 0.05, 200 sweeps): true map 50.549 dB,
regularised estimate 28.415 dB, raw phase difference 20.223 dB, no map 17.735 dB: the estimate gains 10.68 dB over the plain stage.  Psi
falls from 133.85 to 0.672 and never rises, on the fixture and on three seeds of the 32 x 32 case.  Float32 against float64 restatement:
1.3e-05 Hz at 200 sweeps on the fixture."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldmap_ref as FR  # noqa: E402
import handle_cases as HC  # noqa: E402
import offres_ref as OR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HEADER = "pnpadmm_fieldmap.h"
NAMES = ["pnp_fieldmap_cost", "pnp_fieldmap_estimate"]
NARGS = {"pnp_fieldmap_estimate": 11, "pnp_fieldmap_cost": 9}


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


# ---- the header, the binding, the build files ----------------------------------------------------------------------------------------------

def test_the_new_header_and_the_binding_name_the_same_functions():
    text = _header(HEADER)
    assert HC.header_functions(text) == sorted(_lib.SIGNATURES_FIELDMAP) == NAMES
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m is not None and len([p for p in m.group(1).split(",") if p.strip()]) == NARGS[name] == len(_lib.SIGNATURES_FIELDMAP[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_FIELDMAP[name][1]
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    assert re.search(r"#define PNP_FIELDMAP_MAX_ITERS 4096\b", text) and _lib.PNP_FIELDMAP_MAX_ITERS == 4096
    assert re.search(r"#define PNP_FIELDMAP_T %d\b" % FR.FUSE_T, text) and _lib.PNP_FIELDMAP_T == FR.FUSE_T
    for word in ("OUT OF SCOPE", "NO PHASE UNWRAPPING", "|omega| dte < pi", "PNP_FIELDMAP_NAIVE", "De Pierro", "fma(-g, rd_j, t)", "pnp_workspace_bytes"):
        assert word in text, word
    older = set()
    for h in ("pnpadmm.h", "pnpadmm_ncsense.h", "pnpadmm_toeplitz.h", "pnpadmm_dcf.h", "pnpadmm_offres.h"):
        assert "fieldmap" not in _header(h)
        older |= set(HC.header_functions(_header(h)))
    assert not older & set(NAMES)


def test_build_files_the_kernel_unit_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bfieldmap_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_fieldmap_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*pnpadmm_fieldmap\.h", mk, flags=re.M)) == 2           # both dependency lists
    assert re.search(r"^asan_fieldmap: asan .*asan_fieldmap_host\.cpp", mk, flags=re.M) and re.search(r"^\.PHONY:.*\basan_fieldmap\b", mk, flags=re.M)
    unit = open(os.path.join(CSRC, "fieldmap_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()                                       # a launch ends; the next starts
    assert unit.count("sinf(") == 1                                                # one device function of the sweep, for every form
    internal = open(os.path.join(CSRC, "pnp_internal.h")).read()
    assert re.search(r"kFmT = %d\b" % FR.FUSE_T, internal)
    p = inspect.signature(engine.PnPEngine.fieldmap_estimate).parameters
    assert list(p) == ["self", "x1", "x2", "dte", "beta", "iters", "return_weight"]
    assert p["beta"].default == 0.05 and p["iters"].default == 200 and p["return_weight"].default is False
    assert list(inspect.signature(engine.PnPEngine.fieldmap_cost).parameters) == ["self", "x1", "x2", "dte", "beta", "omega"]
    assert list(inspect.signature(acquisition.field_map_scan).parameters) == ["gt", "omega", "te", "dte", "sigma_n", "seed", "sens"]
    p = inspect.signature(acquisition.estimate_field_map).parameters
    assert list(p) == ["engine_or_env", "x1", "x2", "dte", "beta", "iters"] and p["beta"].default == 0.05 and p["iters"].default == 200
    p = inspect.signature(acquisition.field_map_dte).parameters
    assert list(p) == ["omega_max", "margin"] and p["margin"].default == 0.8
    with pytest.raises(TypeError, match="estimate_field_map"):
        acquisition.estimate_field_map(object(), np.zeros((1, 1, 4, 4)), np.zeros((1, 1, 4, 4)), 1e-3)
    assert "|omega| dte < pi" in acquisition.estimate_field_map.__doc__


def test_every_argument_error_is_reported_without_a_gpu_and_leaves_the_outputs_untouched():
    """Host buffers stand in for device memory: a call that is rejected reads and writes none of it."""
    lib = _lib.load()
    a = np.arange(64, dtype=np.float32)
    b = np.arange(64, dtype=np.float32) + 100.0
    om, wt = np.full(64, 7.0, dtype=np.float32), np.full(64, 7.0, dtype=np.float32)
    cost = np.full(8, 7.0, dtype=np.float64)
    pa, pb, po, pw, pc = (v.ctypes.data for v in (a, b, om, wt, cost))
    nan, inf = float("nan"), float("inf")
    est, cst = lib.pnp_fieldmap_estimate, lib.pnp_fieldmap_cost
    cases = [
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, -1, 0, po, pw, None), b"iters must be 0..4096 (got -1)"),
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, 4097, 0, po, pw, None), b"iters must be 0..4096 (got 4097)"),
        (lambda: est(None, None, None, 0, -1.0, 0.0, -1, 1, None, None, None), b"iters"),           # scalar ranges first
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, 200, 1, po, pw, None), b"flags"),
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, 200, -1, po, pw, None), b"flags"),
        (lambda: est(None, pa, pb, 0, 2e-3, 0.05, 200, 0, po, pw, None), b"coils must be 1..32 (got 0)"),
        (lambda: est(None, pa, pb, 33, 2e-3, 0.05, 200, 0, po, pw, None), b"coils must be 1..32 (got 33)"),
        (lambda: est(None, pa, pb, 1, 0.0, 0.05, 200, 0, po, pw, None), b"dte"),
        (lambda: est(None, pa, pb, 1, -2e-3, 0.05, 200, 0, po, pw, None), b"dte"),
        (lambda: est(None, pa, pb, 1, nan, 0.05, 200, 0, po, pw, None), b"dte"),
        (lambda: est(None, pa, pb, 1, inf, 0.05, 200, 0, po, pw, None), b"dte"),
        (lambda: est(None, pa, pb, 1, 2e-3, 0.0, 200, 0, po, pw, None), b"beta"),
        (lambda: est(None, pa, pb, 1, 2e-3, -0.05, 200, 0, po, pw, None), b"beta"),
        (lambda: est(None, pa, pb, 1, 2e-3, nan, 200, 0, po, pw, None), b"beta"),
        (lambda: est(None, pa, pb, 1, 2e-3, inf, 200, 0, po, pw, None), b"beta"),
        (lambda: est(None, None, pb, 1, 2e-3, 0.05, 200, 0, po, pw, None), b"null x1"),
        (lambda: est(None, pa, None, 1, 2e-3, 0.05, 200, 0, po, pw, None), b"null x2"),
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, 200, 0, None, pw, None), b"null omega"),
        (lambda: est(None, pa, pb, 1, 2e-3, 0.05, 200, 0, po, pw, None), b"null handle"),
        (lambda: est(None, pa, pb, 32, 2e-3, 0.05, 0, 0, po, None, None), b"null handle"),        # weight may be NULL, iters may be 0
        (lambda: cst(None, pa, pb, 0, 2e-3, 0.05, po, pc, None), b"coils"),
        (lambda: cst(None, pa, pb, 1, 0.0, 0.05, po, pc, None), b"dte"),
        (lambda: cst(None, pa, pb, 1, nan, 0.05, po, pc, None), b"dte"),
        (lambda: cst(None, pa, pb, 1, 2e-3, 0.0, po, pc, None), b"beta"),
        (lambda: cst(None, pa, pb, 1, 2e-3, inf, po, pc, None), b"beta"),
        (lambda: cst(None, None, pb, 1, 2e-3, 0.05, po, pc, None), b"null x1"),
        (lambda: cst(None, pa, None, 1, 2e-3, 0.05, po, pc, None), b"null x2"),
        (lambda: cst(None, pa, pb, 1, 2e-3, 0.05, None, pc, None), b"null omega"),
        (lambda: cst(None, pa, pb, 1, 2e-3, 0.05, po, None, None), b"null cost"),
        (lambda: cst(None, pa, pb, 1, 2e-3, 0.05, po, pc, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert (om == 7.0).all() and (wt == 7.0).all() and (cost == 7.0).all()
    assert np.array_equal(a, np.arange(64, dtype=np.float32)) and np.array_equal(b, np.arange(64, dtype=np.float32) + 100.0)


def test_the_sanitizer_program_of_the_argument_validation_passes():
    """`make asan_fieldmap`: the instrumented host build of the library (host code only) and tests/asan_fieldmap_host.cpp, a program with its
    own main, run directly."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "asan_fieldmap"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "_asan", "asan_fieldmap_host")], capture_output=True, text=True)
    assert r.returncode == 0 and "asan_fieldmap_host: ok" in r.stdout, r.stdout + r.stderr


# ---- the restatement checks itself -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_psi_never_increases_along_the_float64_iteration(seed):
    """De Pierro's split makes the surrogate separable, so the simultaneous (Jacobi) update descends too: not one sweep of 200 raises Psi"""
    x1, x2, _ = FR.case(1, 32, 32, 1 + 2 * (seed % 2), seed)
    trace = []
    FR.estimate(x1, x2, FR.CASE_DTE, FR.CASE_BETA, 200, trace=trace)
    phi, w = FR.prepare(x1, x2)
    psi = np.array([FR.psi_theta(t, phi, w, FR.CASE_BETA)[0] for t in trace])
    rise = float(np.max(psi[1:] - psi[:-1]))
    print(f"seed {seed}: Psi {psi[0]:.6f} -> {psi[-1]:.6f} over {len(psi) - 1} sweeps, largest step {rise:.3e}")
    assert len(psi) == 201 and rise <= 0.0 and psi[-1] < psi[0]


def _constant_phase(h, w, which):
    """echo images whose product has the SAME float32 phase on every pixel, with magnitudes that vary: sx == sy (or one of them 0) exactly"""
    r = (0.25 + 0.75 * synthetic.phantom(h, w, 5)).astype(np.float32)
    q = (0.5 + 0.5 * synthetic.phantom(h, w, 6)).astype(np.float32)
    x1 = {"pi/4": r + 1j * r, "0": r + 0j, "pi/2": 1j * r, "-3pi/4": -r - 1j * r}[which].astype(np.complex64)
    return x1[None, None], (q + 0j).astype(np.complex64)[None, None]


@pytest.mark.parametrize("which, phase", [("pi/4", math.pi / 4), ("0", 0.0), ("pi/2", math.pi / 2), ("-3pi/4", -3 * math.pi / 4)])
def test_a_pixel_constant_phase_difference_is_a_fixed_point_bit_for_bit(which, phase):
    x1, x2 = _constant_phase(24, 20, which)
    phi, w = FR.prepare(x1, x2, f32=True)
    assert np.unique(phi).size == 1 and phi[0, 0, 0] == np.float32(phase) and w.min() < 0.5 and abs(w.max() - 1.0) <= 2.0 ** -23
    want = phi.astype(np.float64) / 2e-3
    for iters in (0, 1, FR.FUSE_T, 37):
        got = FR.estimate(x1, x2, 2e-3, 0.05, iters, f32=True)
        assert np.array_equal(got, want), (which, iters)


def test_an_all_zero_slice_gives_zeros():
    z = np.zeros((1, 2, 8, 8), dtype=np.complex64)
    for f32 in (False, True):
        phi, w = FR.prepare(z, z, f32)
        assert not phi.any() and not w.any()
        om = FR.estimate(z, z, 2e-3, 0.05, 12, f32=f32)
        assert not om.any() and not np.signbit(om).any()
    assert FR.cost(z, z, 2e-3, 0.05, np.zeros((1, 8, 8)))[0] == 0.0


def test_float32_against_float64_restatement_on_a_200_hz_map():
    """the rounding level of the float32 expression order: recorded, and held to what float32 can give (theta is of order 1 rad, one ulp is
    1.2e-7 rad = 9.5e-6 Hz at dte = 2 ms; 800 sweeps of a contraction do not accumulate more than a few of them)"""
    gt = synthetic.phantom(32, 32, 3)[None]
    om = 2.0 * math.pi * synthetic.field_map(32, 32, 200.0, 1)
    x1, x2 = acquisition.field_map_scan(gt, om, 1e-3, 2e-3, 5.0 / 255.0, 9)
    a = FR.estimate(x1, x2, 2e-3, 0.05, 800)
    b = FR.estimate(x1, x2, 2e-3, 0.05, 800, f32=True)
    gap = float(np.abs(a - b).max()) / (2.0 * math.pi)
    print(f"float32 against float64 restatement, 800 sweeps, 200 Hz map: {gap:.3e} Hz")
    assert gap <= 16 * 2.0 ** -24 * math.pi / 2e-3 / (2.0 * math.pi)              # 16 ulps of pi, in Hz: 2.4e-4


# ---- the estimate helps, in float64 on the CPU: the figures the GPU test is held to ------------------------------------------------------------

def test_the_restatement_alone_shows_that_the_estimate_helps():
    """fieldmap_ref.ESTIMATES in float64: the two-echo scan of offres_ref's fixture, the regularised estimate and the raw phase difference
    through offres_ref.corrects_admm; produces fieldmap_ref.ESTIMATES_PSNR and ESTIMATES_F32_GAP.  The true map's and the plain stage's
    figures are offres_ref.CORRECTS_PSNR (tests/test_offres_host.py produces those)."""
    e = FR.ESTIMATES
    x1, x2 = FR.estimates_scan()
    _, _, omega, _, _, _ = FR.estimates_problem()
    assert float(np.abs(omega).max()) * e["dte"] < math.pi                         # no wrap: the estimator's range of validity
    est = FR.estimate(x1, x2, e["dte"], e["beta"], e["iters"])[0]
    raw = FR.estimate(x1, x2, e["dte"], e["beta"], 0)[0]
    est32 = FR.estimate(x1, x2, e["dte"], e["beta"], e["iters"], f32=True)[0]
    p_est, p_raw, p_est32 = FR.estimates_psnr(est), FR.estimates_psnr(raw), FR.estimates_psnr(est32)
    p_true, p_plain = OR.CORRECTS_PSNR
    hz = 1.0 / (2.0 * math.pi)
    print(f"float64: true map {p_true} dB, regularised estimate {p_est:.4f} dB, raw phase difference {p_raw:.4f} dB, no map {p_plain} dB "
          f"(recorded {FR.ESTIMATES_PSNR}); the float32 restatement's map gives {p_est32:.6f} dB, {abs(p_est32 - p_est):.2e} dB from float64 "
          f"(recorded {FR.ESTIMATES_F32_GAP}); map error rms {np.sqrt(((est - omega) ** 2).mean()) * hz:.2f} Hz (estimate), "
          f"{np.sqrt(((raw - omega) ** 2).mean()) * hz:.2f} Hz (raw), float32 map {np.abs(est32 - est).max() * hz:.2e} Hz from float64")
    assert p_plain < p_raw < p_est < p_true
    assert p_est >= p_plain + 5.0
    assert abs(p_est - FR.ESTIMATES_PSNR[0]) <= 2e-3 and abs(p_raw - FR.ESTIMATES_PSNR[1]) <= 2e-3
    # a map perturbation of 1e-5 Hz under a map error of 28 Hz: the recorded gap, with room for another host's libm and BLAS
    assert abs(p_est32 - p_est) <= 10.0 * FR.ESTIMATES_F32_GAP


# ---- the scan, the echo spacing -----------------------------------------------------------------------------------------------------------------

def test_field_map_scan_and_field_map_dte_values_and_argument_errors():
    h, w = 12, 10
    gt = np.stack([synthetic.phantom(h, w, 1), synthetic.phantom(h, w, 2)])
    om = 2.0 * math.pi * synthetic.field_map(h, w, 80.0, 3)
    x1, x2 = acquisition.field_map_scan(gt, om, 1e-3, 2e-3, 0.0, 7)
    assert x1.shape == x2.shape == (2, 1, h, w) and x1.dtype == x2.dtype == np.complex64
    assert np.allclose(x1[:, 0], gt * np.exp(-1j * om * 1e-3), atol=1e-6) and np.allclose(x2[:, 0], gt * np.exp(-1j * om * 3e-3), atol=1e-6)
    big = gt > 0.2                                                                  # without noise the phase difference IS the map
    assert np.allclose(np.angle(x1[:, 0] * np.conj(x2[:, 0]))[big], np.broadcast_to(om * 2e-3, gt.shape)[big], atol=1e-5)
    # the noise: the hash streams 9601 + 8 c + 4 e at seed + slice, so a slice does not depend on its batch
    sens = synthetic.coil_maps(3, h, w)
    n1, n2 = acquisition.field_map_scan(np.zeros((2, 1, h, w)), om, 0.0, 1e-3, 0.5, 7, sens=sens)
    assert n1.shape == (2, 3, h, w)
    for i in range(2):
        for c in range(3):
            for e, x in enumerate((n1, n2)):
                st = acquisition.FIELD_MAP_STREAM + 8 * c + 4 * e
                want = 0.5 * (synthetic._gauss(7 + i, st, h * w) + 1j * synthetic._gauss(7 + i, st + 2, h * w)).reshape(h, w)
                assert np.array_equal(x[i, c], want.astype(np.complex64))
    alone = acquisition.field_map_scan(np.zeros((1, h, w)), om, 0.0, 1e-3, 0.5, 8, sens=sens)
    assert np.array_equal(alone[0][0], n1[1]) and np.array_equal(alone[1][0], n2[1])
    assert acquisition.FIELD_MAP_STREAM == 9601 and abs(n1.real.std() - 0.5) < 0.05
    both = acquisition.field_map_scan(gt, np.stack([om, 2 * om]), 1e-3, 2e-3, 0.0, 7)
    assert np.array_equal(both[0][0], x1[0]) and not np.array_equal(both[1][1], x2[1])
    for bad, what in ((dict(gt=np.zeros((h, w))), "gt must be"), (dict(omega=np.zeros((3, h, w))), "omega must be"), (dict(te=-1.0), "te >= 0"),
                      (dict(dte=0.0), "dte > 0"), (dict(dte=float("nan")), "dte > 0"), (dict(sigma_n=-1.0), "sigma_n >= 0"),
                      (dict(sens=np.ones((h, w))), "sens must be"), (dict(sens=np.ones((33, h, w))), "sens must be")):
        kw = dict(gt=gt, omega=om, te=1e-3, dte=2e-3, sigma_n=0.0, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError, match=what):
            acquisition.field_map_scan(**kw)
    assert acquisition.field_map_dte(2 * math.pi * 100.0) == 0.8 * math.pi / (2 * math.pi * 100.0) == 4e-3
    assert acquisition.field_map_dte(-500.0, 0.5) == 0.5 * math.pi / 500.0
    for bad in ((0.0, 0.8), (float("inf"), 0.8), (float("nan"), 0.8), (100.0, 0.0), (100.0, 1.0), (100.0, float("nan"))):
        with pytest.raises(ValueError, match="field_map_dte"):
            acquisition.field_map_dte(*bad)


# ---- task_problem and the CLI -----------------------------------------------------------------------------------------------------------------

class _FakeEngine:
    """enough of a PnPEngine for `task_problem` to pick it as the handle (no GPU): it records the estimator's call and answers with a marker"""
    device = "cpu"
    n, h, w = 2, 16, 16

    def __init__(self):
        self.calls = []

    def acquire(self):
        raise AssertionError("not reached")

    def fieldmap_estimate(self, x1, x2, dte, beta=0.05, iters=200, return_weight=False):
        import torch
        self.calls.append((x1.clone(), x2.clone(), dte, beta, iters))
        return torch.full((x1.shape[0],) + tuple(x1.shape[-2:]), 3.0)


def test_task_problem_estimates_the_map_and_keeps_the_truth(monkeypatch):
    import torch
    calls = []

    def fake_simulate(eng, gt, mask, sigma_n, seed, first_slice=0, **k):
        calls.append(k)
        return {"omega": torch.as_tensor(k["omega"]), "times": "T", "segments": 9} if "omega" in k else {}

    monkeypatch.setattr(acquisition, "simulate", fake_simulate)
    monkeypatch.setattr(acquisition, "pipe_dcf", lambda *a, **k: "PIPE")
    gt = np.stack([synthetic.phantom(16, 16, 1), synthetic.phantom(16, 16, 2)]).astype(np.float32)[:, None]
    e = _FakeEngine()
    base = dict(seed=4, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0, b0_segments=9)
    # the default is today's call and today's dict, word for word
    today = acquisition.task_problem("4x_10", gt, e, **base)
    k_today = calls[-1]
    same = acquisition.task_problem("4x_10", gt, e, b0_map="true", **base)
    assert sorted(calls[-1]) == sorted(k_today) == ["dcf", "nufft_grid", "nufft_width", "omega", "segments", "times", "traj"]
    assert sorted(same) == sorted(today) == ["omega", "segments", "times"] and torch.equal(same["omega"], today["omega"]) and e.calls == []
    omega = (2 * math.pi * synthetic.field_map(16, 16, 80.0, 4)).astype(np.float32)
    assert np.array_equal(today["omega"].numpy(), omega)
    # estimate: the data are the true map's; the scan is of the task's own ground truth under it; the estimate replaces omega
    out = acquisition.task_problem("4x_10", gt, e, first_slice=3, b0_map="estimate", b0_dte_ms=2.0, b0_beta=0.1, b0_iters=50, b0_scan_noise=0.02, **base)
    assert np.array_equal(calls[-1]["omega"], omega) and sorted(calls[-1]) == sorted(k_today)
    assert sorted(out) == ["omega", "omega_true", "segments", "times"]
    assert np.array_equal(out["omega_true"].numpy(), omega) and tuple(out["omega"].shape) == (2, 16, 16) and float(out["omega"][0, 0, 0]) == 3.0
    x1, x2, dte, beta, iters = e.calls[-1]
    w1, w2 = acquisition.field_map_scan(gt, omega, 0.0, 2e-3, 0.02, 4 + 3)
    assert (dte, beta, iters) == (2e-3, 0.1, 50) and x1.dtype == torch.complex64
    assert np.array_equal(x1.numpy(), w1) and np.array_equal(x2.numpy(), w2)
    # the defaults of the estimate: dte from b0_hz at margin 0.8, the task's own noise, beta 0.05, 200 sweeps
    acquisition.task_problem("4x_10", gt, e, b0_map="estimate", **base)
    x1, x2, dte, beta, iters = e.calls[-1]
    assert dte == acquisition.field_map_dte(2 * math.pi * 80.0) == 5e-3 and (beta, iters) == (0.05, 200)
    w1, _ = acquisition.field_map_scan(gt, omega, 0.0, 5e-3, 10.0 / 255.0, 4)
    assert np.array_equal(x1.numpy(), w1)
    for bad, what in ((dict(b0_map="guess"), "b0_map must be"), (dict(b0_map="estimate", b0_dte_ms=0.0), "b0_dte_ms > 0"),
                      (dict(b0_map="estimate", b0_dte_ms=7.0), "no phase unwrapping"), (dict(b0_map="estimate", b0_beta=0.0), "b0_beta > 0"),
                      (dict(b0_map="estimate", b0_iters=5000), "b0_iters"), (dict(b0_map="estimate", b0_scan_noise=-1.0), "b0_scan_noise >= 0")):
        with pytest.raises(ValueError, match=what):
            acquisition.task_problem("4x_10", gt, e, **dict(base, **bad))
    with pytest.raises(ValueError, match="needs b0_hz"):
        acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", b0_map="estimate")
    sig = inspect.signature(acquisition.task_problem).parameters
    names = list(sig)
    assert names[names.index("nc_weights") + 1:names.index("nufft_width")] == ["b0_map", "b0_dte_ms", "b0_beta", "b0_iters", "b0_scan_noise"]
    assert sig["b0_map"].default == "true" and sig["b0_dte_ms"].default is None and sig["b0_beta"].default == 0.05 and sig["b0_iters"].default == 200
    assert "|omega| dte < pi" in acquisition.field_map_dte.__doc__ or "phase unwrapping" in acquisition.field_map_dte.__doc__


def test_cli_b0_map_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    b0 = ["--traj", "spiral", "--b0", "50", "--readout-ms", "5"]
    for extra, what in ((["--b0-map", "estimate"], "need --b0"), (["--traj", "spiral", "--b0-map", "estimate"], "need --b0"),
                        (["--traj", "spiral", "--b0-iters", "10"], "need --b0"), (["--b0-dte", "2"], "need --b0"), (["--b0-beta", "0.1"], "need --b0"),
                        (b0 + ["--b0-dte", "2"], "need --b0-map estimate"), (b0 + ["--b0-map", "true", "--b0-iters", "10"], "need --b0-map estimate"),
                        (b0 + ["--b0-beta", "0.1"], "need --b0-map estimate"),
                        (b0 + ["--b0-map", "estimate", "--b0-dte", "0"], "--b0-dte must be"), (b0 + ["--b0-map", "estimate", "--b0-dte", "nan"], "--b0-dte must be"),
                        (b0 + ["--b0-map", "estimate", "--b0-dte", "10"], "no phase unwrapping"),
                        (b0 + ["--b0-map", "estimate", "--b0-beta", "0"], "--b0-beta must be"), (b0 + ["--b0-map", "estimate", "--b0-beta", "inf"], "--b0-beta must be"),
                        (b0 + ["--b0-map", "estimate", "--b0-iters", "-1"], "--b0-iters must be 0..4096"),
                        (b0 + ["--b0-map", "estimate", "--b0-iters", "4097"], "--b0-iters must be 0..4096")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit):                                                 # argparse: not one of the choices
        cli.main(base + b0 + ["--b0-map", "guess", "fixed", "--max_iter", "2"])

    class A:
        traj, spokes, nc_weights, nufft_width, nufft_grid, nc_coils, interleaves, petals, dcf_iters = "spiral", None, "dcf", 6, None, 0, 4, None, 30
        b0, readout_ms, b0_segments = 50.0, 5.0, 8
        b0_map, b0_dte, b0_beta, b0_iters = "true", None, None, None
    today = ["b0_hz", "b0_segments", "coils", "dcf_iters", "interleaves", "mask_kind", "nc_weights", "nufft_grid", "nufft_width", "petals", "readout_ms",
             "spokes"]
    assert sorted(cli._nc_kwargs(A)) == today                                       # --b0-map true: the call of today
    A.b0_map, A.b0_dte, A.b0_iters = "estimate", 2.0, 50
    kw = cli._nc_kwargs(A)
    assert sorted(kw) == sorted(today + ["b0_map", "b0_dte_ms", "b0_beta", "b0_iters"])
    assert (kw["b0_map"], kw["b0_dte_ms"], kw["b0_beta"], kw["b0_iters"]) == ("estimate", 2.0, 0.05, 50)
