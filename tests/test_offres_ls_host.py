"""CPU-only checks of the least-squares temporal interpolator of the off-resonance operator (include/pnpadmm_offres_ls.h): the header, the
table `_lib.SIGNATURES_OFFRES_LS` and the library name the same functions; the header is plain C and links from C; every argument error that
needs no handle comes back without a GPU and leaves the outputs untouched; the pure-host plan code (csrc/offres_ls_plan.hip) is compiled into
a stand-alone program with its own main (tests/asan_offres_ls_host.cpp), plain and with -fsanitize=address,undefined, refuses every invalid
argument and prints its coefficient table; the table's model error is held to the numpy restatement's and to the figures the feature was
proposed with; the segment chooser; the float64 fixture; the Python plumbing with a monkeypatched engine.

BOUNDS (none is measured on the code under test).
  |1 - sum_l b_l(t_m)| <= the plan's own model error: omega = 0 lies in the band.
  model error of the program's float32 table <= 2 x the numpy restatement's (float64 coefficients rounded to float32) + 2^-23 max sum |b|:
  two correct float64 solvers of the ill-conditioned G may differ in b, not in the fit, beyond a small factor; rounding b to float32 moves
  the fit by at most 2^-24 sum |b| per coefficient set, once for each side.
  model error <= 2 x offres_ls_ref.TABLE where the table has the case (the table's own times are 257 equispaced points of a 10 ms span).
  coefficient difference from the restatement: printed; asserted only at 1e-3 max |b|.
  fixture: the PSNR recorded in offres_ls_ref.CORRECTS_LS to 2e-3, as tests/test_offres_host.py asserts its own."""
import inspect
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_cases as HC  # noqa: E402
import nufft_ref as NR  # noqa: E402
import offres_cases as OC  # noqa: E402
import offres_ls_ref as LS  # noqa: E402
import offres_ref as OR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HEADER = "pnpadmm_offres_ls.h"
NAMES = ["pnp_offres_interpolator", "pnp_offres_ls_coeffs", "pnp_offres_plan_ls"]
NARGS = {"pnp_offres_plan_ls": 5, "pnp_offres_interpolator": 1, "pnp_offres_ls_coeffs": 2}
SPAN = 10e-3


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


# ---- the header, the table, the binding, the build ---------------------------------------------------------------------------------------------

def test_the_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(HEADER)
    assert HC.header_functions(text) == sorted(_lib.SIGNATURES_OFFRES_LS) == NAMES
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m is not None and len([p for p in m.group(1).split(",") if p.strip()]) == NARGS[name] == len(_lib.SIGNATURES_OFFRES_LS[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_OFFRES_LS[name][1]
    assert not set(NAMES) & set(OC.ENTRY_POINTS)                                    # the linear header's set stays the set it was
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    for word in ("OUT OF SCOPE", "kOffresLsRidge = 1e-10", "PNP_OFFRES_LS_NAIVE", "PNP_OFFRES_SEG_BLOCK", "fma(b_l, v_l, o)", "OUTSIDE THE BAND",
                 "not centred on 0", "evaluated numerically", "sinc(0) = 1"):
        assert word in text, word
    assert _lib.OFFRES_INTERPOLATORS == {"linear": 1, "ls": 2}


def test_build_files_the_units_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\boffres_ls_kernels\.o\b.*\boffres_ls_plan\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_offres_ls_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*offres_ls_plan\.h.*pnpadmm_offres_ls\.h", mk, flags=re.M)) == 2        # both dependency lists
    unit = open(os.path.join(CSRC, "offres_ls_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()
    plan_src = open(os.path.join(CSRC, "offres_ls_plan.hip")).read() + open(os.path.join(CSRC, "offres_ls_plan.h")).read()
    assert "hip_runtime" not in plan_src and "pnp_internal.h" not in plan_src          # pure host code: no HIP header, no HIP call
    assert re.search(r"kOffresLsRidge\s*=\s*1e-10\s*;", plan_src) and acquisition.OFFRES_LS_RIDGE == LS.RIDGE == 1e-10
    for name, params in (("offres_plan_ls", ["self", "times", "segments", "omega_max"]),
                         ("offres_ls_planned", ["self", "times", "segments", "omega_max"]), ("offres_interpolator", ["self"]),
                         ("offres_ls_coeffs", ["self"])):
        assert list(inspect.signature(getattr(engine.PnPEngine, name)).parameters) == params, name
    for name in ("reset", "set_kspace"):
        p = inspect.signature(getattr(engine.PnPEngine, name)).parameters
        assert p["interpolator"].default == "linear" and p["omega_max"].default is None
    sim = inspect.signature(acquisition.simulate).parameters
    assert sim["interpolator"].default == "linear" and sim["omega_max"].default is None
    assert inspect.signature(acquisition.task_problem).parameters["b0_interp"].default == "linear"
    assert list(inspect.signature(acquisition.offres_ls_coeffs).parameters) == ["times", "segments", "omega_max"]
    assert list(inspect.signature(acquisition.offres_ls_error).parameters)[:4] == ["times", "segments", "omega_max", "omega"]
    assert list(inspect.signature(acquisition.offres_ls_segments).parameters) == ["omega_max", "span", "tol"]


def test_the_header_is_plain_c_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_offres.h"\n#include "pnpadmm_offres_ls.h"\n'
        "int main(void) {\n"
        "    double t[4] = {0.0, 1e-3, 2e-3, 3e-3};\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    if (pnp_offres_plan_ls(0, t, 0, 600.0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"segments\")) return 1;\n"
        "    if (pnp_offres_plan_ls(0, t, PNP_MC_MAX_COILS + 1, 600.0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"segments\")) return 2;\n"
        "    if (pnp_offres_plan_ls(0, t, 4, 600.0, 1) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 3;\n"
        "    if (pnp_offres_plan_ls(0, t, 4, 0.0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"omega_max\")) return 4;\n"
        "    if (pnp_offres_plan_ls(0, 0, 4, 600.0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null t\")) return 5;\n"
        "    if (pnp_offres_plan_ls(0, t, 4, 600.0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 6;\n"
        "    if (pnp_offres_ls_coeffs(0, y) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 7;\n"
        "    if (pnp_offres_interpolator(0) != 0 || pnp_offres_segments(0) != 0) return 8;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f) return 9;\n"
        '    printf("%s\\n", pnp_version());\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_every_argument_error_that_needs_no_handle_is_reported_without_a_gpu_and_leaves_the_outputs_untouched():
    lib = _lib.load()
    t = np.linspace(0.0, 1e-2, 16)
    keep = t.copy()
    out = np.full(64, 7.0, dtype=np.float32)
    pt, po = t.ctypes.data, out.ctypes.data
    nan, inf = float("nan"), float("inf")
    cases = [
        (lambda: lib.pnp_offres_plan_ls(None, pt, 4, 600.0, 1), b"flags"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 4, 600.0, -1), b"flags"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 0, 600.0, 0), b"segments must be 1..32 (got 0)"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 33, 600.0, 0), b"segments must be 1..32 (got 33)"),
        (lambda: lib.pnp_offres_plan_ls(None, None, -1, nan, 0), b"segments"),                # scalar ranges first
        (lambda: lib.pnp_offres_plan_ls(None, None, 4, nan, 0), b"omega_max"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 4, nan, 0), b"omega_max"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 4, inf, 0), b"omega_max"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 4, 0.0, 0), b"omega_max"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 2, -600.0, 0), b"omega_max"),
        (lambda: lib.pnp_offres_plan_ls(None, None, 4, 600.0, 0), b"null t"),
        (lambda: lib.pnp_offres_plan_ls(None, pt, 1, nan, 0), b"null handle"),                # one centre does not read the band
        (lambda: lib.pnp_offres_plan_ls(None, pt, 32, 600.0, 0), b"null handle"),
        (lambda: lib.pnp_offres_ls_coeffs(None, None), b"null coef_host"),
        (lambda: lib.pnp_offres_ls_coeffs(None, po), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_offres_interpolator(None) == 0
    assert (out == 7.0).all() and np.array_equal(t, keep)


# ---- the pure-host plan code: the stand-alone program, plain and sanitized -------------------------------------------------------------------

def _build(workdir, sanitize):
    exe = os.path.join(workdir, "asan_offres_ls_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-std=c++17", "--offload-arch=gfx950"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "tests", "asan_offres_ls_host.cpp"), os.path.join(CSRC, "offres_ls_plan.hip"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def plan_tools(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("offres_ls_plan_host"))
    return d, _build(d, False), _build(d, True)


def test_plan_builder_refuses_every_invalid_argument(plan_tools):
    for exe in plan_tools[1:]:
        r = subprocess.run([exe, "--invalid"], capture_output=True, text=True)
        assert r.returncode == 0 and "asan_offres_ls_host: invalid ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _dump(d, exe, t, L, om):
    inp, outp = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(inp, "wb") as f:
        f.write(np.int64(t.size).tobytes() + t.tobytes())
    r = subprocess.run([exe, "--dump", inp, str(L), repr(float(om)), outp], capture_output=True, text=True)
    assert r.returncode == 0 and "dump ok" in r.stdout and "ridge=1e-10" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    raw = open(outp, "rb").read()
    return np.frombuffer(raw, np.float64, L, 0), np.frombuffer(raw, np.float32, L * t.size, 8 * L).reshape(L, t.size)


@pytest.mark.parametrize("k", (2, 3))
def test_the_coefficients_fit_the_band_as_the_restatement_and_the_table_say(plan_tools, k):
    d, *exes = plan_tools
    t = np.linspace(0.0, SPAN, 257)                                                 # the times the table was computed on
    t = np.concatenate([t, acquisition.readout_times("spiral", 4 * 96, 96, SPAN, te=0.0)])      # ... and a readout clock that repeats
    om = k * math.pi / SPAN
    for L in (1, 2, 3, 8, 10, 32):
        want = acquisition.offres_ls_coeffs(t, L, om)
        tau = LS.centres(t, L)
        grid = LS.band(om, L) if L > 1 else np.zeros(1)                             # one centre fits omega = 0 alone
        e_ref = LS.model_error(t, tau, want.astype(np.float32), grid)
        assert acquisition.offres_ls_error(t, L, om) == pytest.approx(e_ref, rel=1e-12) or L == 1
        for exe in exes:
            tau_c, B = _dump(d, exe, t, L, om)
            assert np.array_equal(tau_c.view(np.int64), tau.view(np.int64)), L      # plan_offres' centres, bit for bit
            sab = float(np.abs(B.astype(np.float64)).sum(axis=0).max())
            e_dev = LS.model_error(t, tau, B, grid)
            one = float(np.abs(1.0 - B.astype(np.float64).sum(axis=0)).max())
            dif = float(np.abs(B - want).max())
            print(f"{k} pi, L = {L:2d}: model error {e_dev:.3e} (restatement {e_ref:.3e}, table {LS.TABLE.get((k, L))}), |1 - sum b| {one:.3e}, "
                  f"max sum |b| {sab:.2f}, max |b| {np.abs(B).max():.2f}, max |b - restatement| {dif:.3e}")
            assert np.isfinite(B).all()
            if L == 1:
                assert (B == 1.0).all()
                continue
            assert one <= e_dev * (1.0 + 1e-9) + 1e-12                              # omega = 0 is a point of the grid (to a rounding of linspace)
            assert e_dev <= 2.0 * e_ref + 2.0 ** -23 * sab
            if (k, L) in LS.TABLE:
                assert e_dev <= 2.0 * LS.TABLE[(k, L)]
            assert dif <= 1e-3 * float(np.abs(want).max())


def test_the_segment_chooser_for_the_least_squares_interpolator():
    """7 at 2 pi and 9 at 3 pi for tol = 1e-3, where the linear chooser asks for 72 and 107 (tests/test_offres_host.py keeps those).  The
    proposal's table lists even counts only (6, 8, 10, 12) and so names 8 and 10; the rule it states - the smallest L whose error on 257
    equispaced times is <= tol - gives one fewer, because the odd counts between them already meet the tolerance: L = 7 leaves 9.0e-4 at 2 pi
    (L = 6: 6.0e-3) and L = 9 leaves 5.1e-4 at 3 pi (L = 8: 2.8e-3), the same on 2049 times.  The even counts' errors are the table's."""
    got = [acquisition.offres_ls_segments(k * math.pi / SPAN, SPAN) for k in (2, 3)]
    print(f"offres_ls_segments(tol = 1e-3): {got[0]} at 2 pi, {got[1]} at 3 pi; linear: {acquisition.offres_segments(2 * math.pi / SPAN, SPAN)}, "
          f"{acquisition.offres_segments(3 * math.pi / SPAN, SPAN)}")
    assert got == [7, 9]
    assert acquisition.offres_segments(2 * math.pi / SPAN, SPAN) == 72 and acquisition.offres_segments(3 * math.pi / SPAN, SPAN) == 107
    assert acquisition.offres_ls_segments(0.0, SPAN) == 1 and acquisition.offres_ls_segments(100.0, 0.0) == 1
    for k, L in ((2, 7), (3, 9)):                                                   # the smallest: one fewer misses the tolerance
        t = np.linspace(0.0, SPAN, 257)
        assert acquisition.offres_ls_error(t, L, k * math.pi / SPAN) <= 1e-3 < acquisition.offres_ls_error(t, L - 1, k * math.pi / SPAN)
        assert acquisition.offres_ls_error(t, L + 1, k * math.pi / SPAN) <= 2.0 * LS.TABLE[(k, L + 1)]      # the table's 8 and 10
    assert acquisition.offres_ls_segments(40 * math.pi / SPAN, SPAN) == acquisition.OFFRES_MAX_SEGMENTS + 1      # more than the library takes
    with pytest.raises(ValueError):
        acquisition.offres_ls_segments(float("nan"), SPAN)
    # the error over a map's own values is at most the error over the band it lies in (the band's grid aside: 2x)
    t = np.linspace(0.0, SPAN, 257)
    om = OR.case_omega(16, 16, 100.0, 1).astype(np.float64)
    top = float(np.abs(om).max()) * (1 + 1e-6)
    assert acquisition.offres_ls_error(t, 8, top, omega=om) <= 2.0 * acquisition.offres_ls_error(t, 8, top)


# ---- the correction corrects, in float64 on the CPU: the figures the GPU test is held to ---------------------------------------------------------

def test_the_restatement_shows_that_eight_least_squares_segments_correct_as_well_as_thirty_two_linear():
    """offres_ref.CORRECTS in float64 on the NUFFT model with the least-squares interpolator at L = 8; produces offres_ls_ref.CORRECTS_LS"""
    import dcf_ref
    c = OR.CORRECTS
    traj, t, omega, gt, y, _ = OR.corrects_problem()
    L = LS.CORRECTS_LS_L
    P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
    dcf = dcf_ref.pipe(P, 30)[0]
    om_max = float(np.abs(omega).max()) * (1.0 + 1e-6)
    B = acquisition.offres_ls_coeffs(t, L, om_max).astype(np.float32).astype(np.float64)
    E = OR.maps(omega, LS.plan_like(t, L)).astype(np.complex64).astype(np.complex128)
    psnr, misfit = OR.corrects_admm(P, lambda p: LS.model_forward(P, B, E, p), lambda q: LS.model_adjoint(P, B, E, q, dcf), y, gt, dcf)
    eps = acquisition.offres_ls_error(t, L, om_max, omega=omega)
    print(f"float64, least squares L = {L}: {psnr:.4f} dB (recorded {LS.CORRECTS_LS[0]}; linear L = 32: {OR.CORRECTS_PSNR[0]}), misfit at x = gt "
          f"{misfit:.4e} (recorded {LS.CORRECTS_LS[1]}; linear L = 32: {LS.LINEAR_L32_MISFIT}), model error at the map's frequencies {eps:.3e}, "
          f"max sum |b| {np.abs(B).sum(axis=0).max():.2f}")
    assert psnr >= OR.CORRECTS_PSNR[0]
    assert abs(psnr - LS.CORRECTS_LS[0]) <= 2e-3
    assert misfit < LS.LINEAR_L32_MISFIT


# ---- task_problem, PnPEnv, the CLI -----------------------------------------------------------------------------------------------------------------

class _FakeEngine:
    """enough of a PnPEngine for `task_problem` to pick it as the handle, and for PnPEnv to install an episode on (no GPU)"""
    device = "cpu"
    live_episode = 0
    n, h, w = 2, 16, 16

    def __init__(self):
        self.calls, self.nufft, self.offres = [], None, None

    def acquire(self):
        raise AssertionError("not reached")

    def nufft_planned(self, traj, grid=None, width=6):
        return self.nufft is not None and self.nufft[0] is traj

    def nufft_plan(self, traj, grid=None, width=6):
        self.calls.append(("nufft_plan", tuple(traj.shape), grid, width))
        self.nufft, self.offres, self.live_episode = (traj, grid, width), None, 0

    def offres_planned(self, times, segments):
        return self.offres is not None and len(self.offres) == 2 and np.array_equal(self.offres[0], np.asarray(times)) and self.offres[1] == segments

    def offres_plan(self, times, segments):
        self.calls.append(("offres_plan", tuple(times.shape), segments))
        self.offres, self.live_episode = (np.asarray(times).copy(), segments), 0

    def offres_ls_planned(self, times, segments, omega_max):
        return self.offres is not None and len(self.offres) == 3 and np.array_equal(self.offres[0], np.asarray(times)) and \
            self.offres[1:] == (segments, omega_max)

    def offres_plan_ls(self, times, segments, omega_max):
        self.calls.append(("offres_plan_ls", tuple(times.shape), segments, omega_max))
        self.offres, self.live_episode = (np.asarray(times).copy(), segments, omega_max), 0

    def reset_offres(self, x0, y, omega, w=None, cg_iters=8):
        self.calls.append(("reset_offres", tuple(y.shape), tuple(omega.shape), w is not None, cg_iters))
        self.live_episode = 77
        return x0.real.clone(), x0.clone(), x0 * 0

    def set_kspace_offres(self, y, omega, w=None, episode=0, cg_iters=8):
        self.calls.append(("set_kspace_offres", tuple(y.shape), tuple(omega.shape), w is not None, episode, cg_iters))
        self.live_episode = episode


def test_task_problem_hands_the_interpolator_to_simulate(monkeypatch):
    calls = []

    def fake_simulate(eng, gt, mask, sigma_n, seed, first_slice=0, **k):
        calls.append(k)
        return {}

    monkeypatch.setattr(acquisition, "simulate", fake_simulate)
    monkeypatch.setattr(acquisition, "pipe_dcf", lambda *a, **k: "PIPE")
    gt = np.zeros((2, 64, 64), dtype=np.float32)
    e = _FakeEngine()
    acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0, b0_segments=9)
    assert "interpolator" not in calls[-1]                                          # the linear call is the call it always was
    acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0, b0_segments=9, b0_interp="ls")
    assert calls[-1]["interpolator"] == "ls" and calls[-1]["segments"] == 9
    for bad, what in ((dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, b0_interp="cubic"), "b0_interp"),
                      (dict(mask_kind="spiral-nc", b0_interp="ls"), "b0_interp needs b0_hz")):
        with pytest.raises(ValueError, match=what):
            acquisition.task_problem("4x_10", gt, e, **bad)
    for bad, what in ((dict(interpolator="cubic"), "interpolator"), (dict(interpolator="ls"), "go with omega"), (dict(omega_max=3.0), "go with omega")):
        monkeypatch.undo()
        with pytest.raises(ValueError, match=what):
            acquisition.simulate(e, gt, None, 0.0, 1, **bad)


def test_the_environment_installs_and_rebinds_a_least_squares_episode():
    import torch
    from dt4image_restoration_amd import env as envmod
    n, h, w, m = 2, 16, 16, 48
    fake = _FakeEngine()
    env = envmod.PnPEnv.__new__(envmod.PnPEnv)
    env.nc_normal, env.cg_iters, env.nufft_width, env.nufft_grid = "nufft", 5, 6, None
    env._engine_for = lambda *a: fake
    times = np.tile(np.arange(24) * 1e-4, 2)
    omega = torch.full((h, w), 2 * math.pi * 100.0)
    band = float(omega.abs().max()) * (1.0 + 1e-6)
    data = {"x0": torch.zeros(n, 1, h, w, 2), "y0": torch.zeros(n, 1, m, 2), "gt": torch.zeros(n, 1, h, w), "traj": torch.zeros(m, 2, dtype=torch.float64),
            "dcf": torch.ones(m), "omega": omega, "times": torch.from_numpy(times), "segments": 4, "b0_interp": "ls"}
    x0 = torch.zeros(n, 1, h, w, dtype=torch.complex64)
    st = env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    assert [c[0] for c in fake.calls] == ["nufft_plan", "offres_plan_ls", "reset_offres"]
    assert fake.calls[1] == ("offres_plan_ls", (m,), 4, band) and st["b0_interp"] == "ls" and st["omega_max"] == band and st["segments"] == 4
    del fake.calls[:]
    env._bind_episode(fake, st)                                                     # the live episode on the live plan: nothing to do
    assert fake.calls == []
    fake.offres = (times.copy(), 4)                                                 # a linear plan of the same times took its place
    fake.live_episode = 5
    env._bind_episode(fake, st)
    assert [c[0] for c in fake.calls] == ["offres_plan_ls", "set_kspace_offres"]
    del fake.calls[:]
    st2 = env._reset_nc(dict(data, b0_interp=torch.tensor(2)), x0, n, h, w, torch.device("cpu"))      # the code `simulate` writes
    assert st2["b0_interp"] == "ls" and fake.calls[-1][0] == "reset_offres" and "offres_plan" not in [c[0] for c in fake.calls]
    lin = env._reset_nc({k: v for k, v in data.items() if k != "b0_interp"}, x0, n, h, w, torch.device("cpu"))
    assert "b0_interp" not in lin and "omega_max" not in lin and fake.calls[-2][0] == "offres_plan"
    auto = {k: v for k, v in data.items() if k != "segments"}                       # the chooser: 2 pi 100 Hz over 2.3 ms = 1.45 rad
    st = env._reset_nc(auto, x0, n, h, w, torch.device("cpu"))
    assert st["segments"] == acquisition.offres_ls_segments(band, 23e-4) and 2 <= st["segments"] <= 8
    with pytest.raises(ValueError, match="b0_interp"):
        env._reset_nc(dict(data, b0_interp="cubic"), x0, n, h, w, torch.device("cpu"))


def test_cli_b0_interp_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--b0-interp", "ls"], "--b0-interp needs --b0"), (["--traj", "spiral", "--b0-interp", "ls"], "--b0-interp needs --b0")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit):                                                 # argparse refuses an unknown choice
        cli.main(base + ["--traj", "spiral", "--b0", "50", "--readout-ms", "5", "--b0-interp", "cubic", "fixed", "--max_iter", "2"])

    class A:
        traj, spokes, nc_weights, nufft_width, nufft_grid, nc_coils, interleaves, petals, dcf_iters = "spiral", None, "dcf", 6, None, 0, 4, None, 30
        b0, readout_ms, b0_segments, b0_interp = 50.0, 5.0, 8, "linear"
    assert "b0_interp" not in cli._nc_kwargs(A)
    A.b0_interp = "ls"
    assert cli._nc_kwargs(A)["b0_interp"] == "ls"
