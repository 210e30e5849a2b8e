"""CPU-only checks of the density compensation: the entry points of include/pnpadmm_dcf.h are declared, exported, bound from
`_lib.SIGNATURES_DCF` and classified in tests/dcf_cases.py, while the three older headers and tables stay the sets they were; the header
compiles as C99 and links from C; every argument error that needs no handle comes back without a GPU - from ctypes, from C and from the
stand-alone sanitizer program tests/asan_dcf_host.cpp (`make asan_dcf`: a CPU build with its own main, nothing preloaded) - and leaves the
outputs untouched; the build files name the new unit; the float64 restatement the GPU tests compare against (tests/dcf_ref.py) checks
itself; the trajectory generators, `task_problem` and the CLI accept the new spellings.

Restatement, on the three cases of dcf_ref.CASES (13 radial spokes at 16 x 16, J = 8; a 9-petal rosette of 1500 samples at 32 x 16, J = 4;
a spiral of 3064 samples at 64 x 64, J = 6): Psi is symmetric (0 .. 6e-16 observed), Psi w > 0, max |Psi w - 1| falls from 0.271, 0.263,
0.271 after one iteration to 0.055, 0.059, 0.051 after 30, and the sidelobe norm of the exact point-spread function falls from 1.450, 1.405,
1.929 with uniform weights to 0.844, 1.105, 1.421 with the iterated ones.
Order sensitivity: 30 iterations on a permutation of the samples move a weight by at most 1.8e-15, 1.8e-15, 2.4e-15 relative (bound: 2^-40
= 9.1e-13); the GPU tests' 2^-23 is one float32 rounding (2^-24) plus a margin 2^-24 = 6e-8 that dwarfs this number.

End to end: dcf_ref.FIXTURE (64 x 64 phantom, 8 spiral interleaves of 384 samples, 6 turns, TV prior, K = 8) in float64 goes from 15.174 dB
to 36.530 dB with the iterated weights and from 1.670 dB to 35.223 dB without; recorded in dcf_ref.FIXTURE_PSNR / FIXTURE_PSNR_UNWEIGHTED and
produced here."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcf_cases as DC  # noqa: E402
import dcf_ref as D  # noqa: E402
import handle_cases as HC  # noqa: E402
import ncsense_cases as NC  # noqa: E402
import nufft_ref as NR  # noqa: E402
import toeplitz_cases as TC  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
ORDER_BOUND = 2.0 ** -40


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(DC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(DC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_DCF) == ["pnp_nufft_dcf", "pnp_nufft_psi"]
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in DC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_DCF[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{DC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_DCF[name][1]          # bound by _lib.load()'s loop
        assert cls == HC.INTRUDER
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_dcf.py")).read()
    for name in DC.ENTRY_POINTS:
        assert f"def {DC.COVERED_BY[name]}(" in gpu, name
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    for gone in DC.ENTRY_POINTS:                                                    # deleting any row of the table is noticed
        assert DC.missing(names, {k: v for k, v in DC.ENTRY_POINTS.items() if k != gone}) == [gone]
    assert DC.missing(names) == []
    assert _lib.PNP_DCF_MAX_ITERS == 256 and re.search(r"#define\s+PNP_DCF_MAX_ITERS\s+256\b", text)


def test_the_three_older_headers_and_tables_are_the_sets_they_were():
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) == sorted(HC.ENTRY_POINTS) and len(old) == 57
    ns = HC.header_functions(_header(NC.HEADER))
    assert ns == sorted(_lib.SIGNATURES_NCSENSE) == sorted(NC.ENTRY_POINTS) and len(ns) == 8
    tz = HC.header_functions(_header(TC.HEADER))
    assert tz == sorted(_lib.SIGNATURES_TOEPLITZ) == sorted(TC.ENTRY_POINTS) and len(tz) == 10
    new = set(DC.ENTRY_POINTS)
    assert not new & set(old) and not new & set(ns) and not new & set(tz)
    for h in ("pnpadmm.h", NC.HEADER, TC.HEADER):
        assert "pnp_nufft_dcf" not in _header(h) and "pnp_nufft_psi" not in _header(h)


def test_build_files_the_kernel_unit_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bdcf_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_dcf_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*pnpadmm_dcf\.h", mk, flags=re.M)) == 2           # both dependency lists
    assert re.search(r"^asan_dcf: asan .*asan_dcf_host\.cpp", mk, flags=re.M) and re.search(r"^\.PHONY:.*\basan_dcf\b", mk, flags=re.M)
    unit = open(os.path.join(CSRC, "dcf_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()                                       # a launch ends; the next starts
    assert list(inspect.signature(engine.PnPEngine.nufft_psi).parameters) == ["self", "w"]
    assert list(inspect.signature(engine.PnPEngine.nufft_dcf).parameters) == ["self", "iters", "w0", "return_info"]
    sig = inspect.signature(engine.PnPEngine.nufft_dcf).parameters
    assert sig["iters"].default == 30 and sig["w0"].default is None and sig["return_info"].default is False
    assert list(inspect.signature(acquisition.pipe_dcf).parameters) == ["engine_or_env", "traj", "iters", "width", "grid"]
    sig = inspect.signature(acquisition.pipe_dcf).parameters
    assert sig["iters"].default == 30 and sig["width"].default == 6 and sig["grid"].default is None
    with pytest.raises(TypeError, match="pipe_dcf"):
        acquisition.pipe_dcf(object(), np.zeros((4, 2)))


def test_the_new_header_is_plain_c_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_dcf.h"\n'
        "int main(void) {\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    if (pnp_nufft_psi(0, 0, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null w\")) return 1;\n"
        "    if (pnp_nufft_psi(0, y, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null out\")) return 2;\n"
        "    if (pnp_nufft_psi(0, y, y + 2, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 3;\n"
        "    if (pnp_nufft_dcf(0, y, 0, 0, y + 2, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"iters\")) return 4;\n"
        "    if (pnp_nufft_dcf(0, y, PNP_DCF_MAX_ITERS + 1, 0, y + 2, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"iters\")) return 5;\n"
        "    if (pnp_nufft_dcf(0, y, 30, 1, y + 2, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 6;\n"
        "    if (pnp_nufft_dcf(0, 0, 30, 0, 0, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null w\")) return 7;\n"
        "    if (pnp_nufft_dcf(0, 0, 30, 0, y, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 8;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f || PNP_DCF_MAX_ITERS != 256) return 9;\n"
        '    printf("%s\\n", pnp_version());\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_every_argument_error_that_needs_no_handle_is_reported_without_a_gpu_and_leaves_the_outputs_untouched():
    """Host buffers stand in for device memory: a call that is rejected reads and writes none of it.  (The rejection that reads the handle -
    no plan - is made on the GPU by tests/test_gpu_dcf.py.)"""
    lib = _lib.load()
    a = np.arange(64, dtype=np.float32)
    out, info = np.full(64, 7.0, dtype=np.float32), np.full(257, 7.0, dtype=np.float32)
    pa, po, pi = (v.ctypes.data for v in (a, out, info))
    cases = [
        (lambda: lib.pnp_nufft_psi(None, None, po, None), b"null w"),
        (lambda: lib.pnp_nufft_psi(None, pa, None, None), b"null out"),
        (lambda: lib.pnp_nufft_psi(None, pa, po, None), b"null handle"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 0, 0, po, pi, None), b"iters"),
        (lambda: lib.pnp_nufft_dcf(None, pa, -1, 0, po, pi, None), b"iters"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 257, 0, po, pi, None), b"iters"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 0, 1, None, pi, None), b"iters"),          # scalar ranges first
        (lambda: lib.pnp_nufft_dcf(None, pa, 30, 1, po, pi, None), b"flags"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 30, -1, po, pi, None), b"flags"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 30, 0, None, pi, None), b"null w"),
        (lambda: lib.pnp_nufft_dcf(None, pa, 30, 0, po, pi, None), b"null handle"),
        (lambda: lib.pnp_nufft_dcf(None, None, 1, 0, po, None, None), b"null handle"),   # w0 and info may be NULL
        (lambda: lib.pnp_nufft_dcf(None, None, 256, 0, po, None, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert (out == 7.0).all() and (info == 7.0).all() and np.array_equal(a, np.arange(64, dtype=np.float32))


def test_the_sanitizer_program_of_the_argument_validation_passes():
    """`make asan_dcf`: the instrumented host build of the library (host code only) and tests/asan_dcf_host.cpp, a program with its own
    main, run directly."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "asan_dcf"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "_asan", "asan_dcf_host")], capture_output=True, text=True)
    assert r.returncode == 0 and "asan_dcf_host: ok" in r.stdout, r.stdout + r.stderr


# ---- the restatement checks itself ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_the_restatement_is_symmetric_positive_converges_and_sharpens_the_point_spread_function(i):
    h, w, gh, gw, J, kind = D.CASES[i]
    traj, P = D.case_traj(i), D.case_plan(i)
    m = P["m"]
    assert (P["gh"], P["gw"], P["J"]) == (gh, gw, J) and traj.shape == (m, 2)
    if kind == "radial":                                                           # the centre samples coincide and the footprints wrap
        assert (np.hypot(traj[:, 0], traj[:, 1]) == 0).sum() == NR.SPOKES and P["i0"].min() < 0
    if kind == "spiral":
        assert m % 256 and m % 2048 and m > 2048
    rng = np.random.default_rng(40 + i)
    u, v = rng.random(m) + 0.1, rng.random(m) + 0.1
    a, b = float(u @ D.psi(P, v)), float(v @ D.psi(P, u))
    w1, info1 = D.case_ref(i, 1)
    w30, info30 = D.case_ref(i, 30)
    s0, s30 = D.sidelobe(traj, h, w), D.sidelobe(traj, h, w, w30)
    print(f"case {i} {D.CASES[i]} M = {m}: |<u, Psi v> - <v, Psi u>| / <u, Psi v> {abs(a - b) / a:.2e}; max |Psi w - 1| {info30[0]:.2f} at the "
          f"start, {info1[1]:.4f} after 1, {info30[30]:.4f} after 30; sidelobe norm {s0:.3f} uniform, {s30:.3f} iterated")
    assert abs(a - b) <= 1e-12 * a
    for wv in (np.ones(m), D.case_start(i), w1, w30):
        assert (D.psi(P, wv) > 0).all()
    assert np.array_equal(info1[:1], info30[:1]) and info30[1] == info1[1]         # info[k] does not depend on iters
    assert info30[30] < info1[1] < info30[0]
    assert s30 < s0
    for wv in (w1, w30, D.case_ref(i, 30, True)[0]):
        assert abs(wv.sum() - h * w) <= 1e-12 * h * w and (wv > 0).all()


@pytest.mark.parametrize("i", range(len(D.CASES)))
def test_order_sensitivity_of_the_restatement_is_below_the_bound_the_device_tolerance_leans_on(i):
    h, w, gh, gw, J, _ = D.CASES[i]
    traj = D.case_traj(i)
    perm = np.random.default_rng(5).permutation(traj.shape[0])
    wp, ip = D.pipe(NR.plan(h, w, gh, gw, J, traj[perm]), 30)
    w30, info30 = D.case_ref(i, 30)
    rel = float(np.abs(wp / w30[perm] - 1.0).max())
    print(f"case {i}: 30 iterations on a permutation of the {traj.shape[0]} samples: largest relative difference {rel:.2e} (bound {ORDER_BOUND:.2e}), "
          f"info {np.abs(ip - info30).max():.2e}")
    assert rel < ORDER_BOUND and np.abs(ip - info30).max() < 1e-12


# ---- generators, task_problem, the CLI -----------------------------------------------------------------------------------------------------

def test_the_generators():
    for h, w, L, R, turns in ((64, 64, 8, 384, 6), (32, 16, 3, 101, 2.5), (16, 16, 1, 2, 1)):
        t = acquisition.spiral_trajectory(h, w, L, readout=R, turns=turns)
        assert t.shape == (L * R, 2) and t.dtype == np.float64 and (np.hypot(t[:, 0], t[:, 1]) < 0.5).all()
        assert (t[::R] == 0).all()                                                 # the first sample of every interleaf
        l, j = L - 1, R - 1                                                        # the row order and the axis convention
        a = 2 * np.pi * (turns * j / R + l / L)
        assert np.allclose(t[l * R + j], (0.5 * j / R * np.sin(a), 0.5 * j / R * np.cos(a)), rtol=0, atol=1e-15)
    t = acquisition.spiral_trajectory(64, 64, 8)                                   # the documented defaults: 4 turns, ceil(4 pi 64) = 805 samples
    assert t.shape == (8 * 805, 2) and np.allclose(t[804], acquisition.spiral_trajectory(64, 64, 8, readout=805, turns=4)[804])
    assert acquisition.spiral_trajectory(16, 16, 64).shape == (64 * 51, 2)         # at least one turn
    for h, w, P, R in ((32, 16, 9, 1500), (16, 16, 5, 200), (64, 64, 7, None)):
        t = acquisition.rosette_trajectory(h, w, P, readout=R)
        R = int(np.ceil(0.5 * np.pi * P * max(h, w))) if R is None else R
        # a sample on a petal's tip sits at 0.5 itself (9 petals of 1500 samples: t = 1/6), which the plan accepts; never beyond
        assert t.shape == (R, 2) and t.dtype == np.float64 and (np.hypot(t[:, 0], t[:, 1]) <= 0.5).all() and (np.abs(t) <= 0.5).all()
        assert (t[0] == 0).all()
        j = R // 3
        r, a = 0.5 * np.sin(np.pi * P * j / R), np.pi * (P - 2) * j / R
        assert np.allclose(t[j], (r * np.sin(a), r * np.cos(a)), rtol=0, atol=1e-15)
    for bad in (lambda: acquisition.spiral_trajectory(16, 16, 0), lambda: acquisition.spiral_trajectory(16, 16, 2, readout=1),
                lambda: acquisition.spiral_trajectory(16, 16, 2, turns=0), lambda: acquisition.rosette_trajectory(16, 16, 0),
                lambda: acquisition.rosette_trajectory(16, 16, 3, readout=1)):
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(D.fixture_traj(), acquisition.spiral_trajectory(64, 64, 8, readout=384, turns=6))


class _FakeEngine:
    """enough of a PnPEngine for `task_problem` to pick it as the handle (no GPU)"""
    device = "cuda:0"

    def acquire(self):
        raise AssertionError("not reached")


def test_the_ramp_is_not_reachable_for_a_trajectory_it_was_not_written_for(monkeypatch):
    calls = []

    def no_ramp(*a, **k):
        raise AssertionError("radial_dcf called")

    def fake_pipe(eng, traj, iters=30, width=6, grid=None):
        calls.append(("pipe", traj.shape, iters, width, grid))
        return "PIPE"

    def fake_simulate(eng, gt, mask, sigma_n, seed, first_slice=0, **k):
        calls.append(("simulate", k["traj"].shape, k["dcf"] if isinstance(k["dcf"], (str, type(None))) else "ramp", k["sens"] is not None))
        return {}

    gt = np.zeros((2, 64, 64), dtype=np.float32)
    monkeypatch.setattr(acquisition, "pipe_dcf", fake_pipe)
    monkeypatch.setattr(acquisition, "simulate", fake_simulate)
    e = _FakeEngine()
    acquisition.task_problem("4x_10", gt, e, mask_kind="radial-nc")                 # the ramp where it belongs
    acquisition.task_problem("4x_10", gt, e, mask_kind="radial-nc", nc_weights="pipe", dcf_iters=7, nufft_width=4)
    assert calls == [("simulate", (16 * 128, 2), "ramp", False), ("pipe", (16 * 128, 2), 7, 4, None), ("simulate", (16 * 128, 2), "PIPE", False)]
    del calls[:]
    monkeypatch.setattr(acquisition, "radial_dcf", no_ramp)
    for kind, kw, m in (("spiral-nc", {}, 8 * 805), ("spiral-nc", {"interleaves": 5}, 5 * 1408), ("rosette-nc", {}, 1710),
                        ("rosette-nc", {"petals": 9}, 905)):
        for nc_weights in ("dcf", "pipe"):
            acquisition.task_problem("4x_10", gt, e, mask_kind=kind, nc_weights=nc_weights, coils=2 if "petals" in kw else 0, **kw)
            assert calls == [("pipe", (m, 2), 30, 6, None), ("simulate", (m, 2), "PIPE", "petals" in kw)], (kind, kw, calls)
            del calls[:]
        acquisition.task_problem("4x_10", gt, e, mask_kind=kind, nc_weights="none", **kw)
        assert calls == [("simulate", (m, 2), None, False)]
        del calls[:]
    with pytest.raises(ValueError, match="nc_weights"):
        acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", nc_weights="ramp")
    with pytest.raises(ValueError, match="takes no mask"):
        acquisition.task_problem("4x_10", gt, e, mask_kind="rosette-nc", mask=np.ones((64, 64)))
    assert acquisition.NC_KINDS == ("radial-nc", "spiral-nc", "rosette-nc")
    names = list(inspect.signature(acquisition.task_problem).parameters)
    assert names[-3:] == ["interleaves", "petals", "dcf_iters"] and names.index("nufft_grid") == len(names) - 4      # new keywords at the end


def test_cli_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--interleaves", "4"], "--interleaves needs --traj spiral"), (["--petals", "5"], "--petals needs --traj rosette"),
                        (["--dcf-iters", "10"], "--dcf-iters needs --traj"), (["--nc-weights", "pipe"], "need --traj radial"),
                        (["--traj", "radial", "--interleaves", "4"], "--interleaves needs --traj spiral"),
                        (["--traj", "spiral", "--spokes", "4"], "--spokes needs --traj radial"),
                        (["--traj", "spiral", "--petals", "4"], "--petals needs --traj rosette"),
                        (["--traj", "spiral", "--interleaves", "0"], "--interleaves must be"),
                        (["--traj", "rosette", "--petals", "0"], "--petals must be"),
                        (["--traj", "spiral", "--dcf-iters", "0"], "--dcf-iters must be 1..256"),
                        (["--traj", "rosette", "--dcf-iters", "257"], "--dcf-iters must be 1..256"),
                        (["--traj", "spiral", "--coils", "4"], "--traj with --coils"),
                        (["--traj", "rosette", "--mask", "cartesian"], "--traj takes no --mask"),
                        (["--traj", "spiral", "--nc-normal", "toeplitz", "--size", "640"], "h, w up to 512")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    for bad in (["--traj", "lissajous"], ["--traj", "spiral", "--nc-weights", "ramp"]):
        with pytest.raises(SystemExit):                                            # argparse: not a choice
            cli.main(base + bad + ["fixed"])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------

def test_the_end_to_end_constants():
    t = D.FIXTURE
    mu, sig = D.fixture_schedules()
    out = []
    for weights, recorded in ((True, D.FIXTURE_PSNR), (False, D.FIXTURE_PSNR_UNWEIGHTED)):
        d, P = D.fixture_problem(weights)
        assert P["m"] == 8 * 384 and (d["dcf"] is not None) == weights
        x, p0, p1 = NR.admm_tv_nc(d, P, mu, sig, t["cg_iters"], t["tv_scale"], t["tv_iters"])
        out.append((p0[0], p1[0]))
        print(f"spiral fixture, weights {weights}: x0 {p0[0]:.3f} dB, final {p1[0]:.4f} dB (recorded {recorded})")
        assert abs(p0[0] - recorded[0]) <= 2e-3 and abs(p1[0] - recorded[1]) <= 2e-3
    assert out[0][0] > out[1][0] + 10.0 and out[0][1] > out[1][1] + 1.0              # what the weights buy: the start and the K iterations
