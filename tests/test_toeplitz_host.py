"""CPU-only checks of the Toeplitz normal operator: the entry points of include/pnpadmm_toeplitz.h are declared, exported, bound from
`_lib.SIGNATURES_TOEPLITZ` and classified in tests/toeplitz_cases.py, while the two older headers and tables stay the sets they were; the
header compiles as C99 and links from C; every argument error that needs no handle comes back without a GPU - from ctypes, from C and from
the stand-alone sanitizer program tests/asan_toeplitz_host.cpp (`make asan_toeplitz`: a CPU build with its own main, nothing preloaded) - and
leaves the outputs untouched; the build files name the new unit; the float64 restatement the GPU tests compare against
(tests/toeplitz_ref.py) checks itself; the Python layers and the CLI accept the new spelling.

Restatement, on the five cases of nufft_ref.CASES with non-trivial weights: toeplitz_ref.apply equals ndft_adjoint(ndft(p)), the exact
operator, to 1e-12 relative l2 (1e-15 .. 2e-15 observed); `spectrum` equals the real part of the centred transform of the directly summed T to
1e-12 of max |K|, whose imaginary part is below 1e-14 of max |K|; the float32 restatement (K rounded to float32, every stage to complex64)
lies 3e-8 .. 5e-8 from the exact operator where the NUFFT model lies 1.2e-5, 4.9e-4, 9.0e-4, 1.8e-5, 1.2e-7.

End to end: nufft_ref.FIXTURE and ncsense_ref.FIXTURE with the Toeplitz operator inside the CG (aty on the NUFFT model, as in the library):
the float64 restatement goes from 16.572 dB to 36.812 dB (the NUFFT stage: 36.812 dB as well, max |dx| 1.2e-3 between the two) and from
17.493 dB to 32.399 dB; the constants are recorded in toeplitz_ref.FIXTURE_PSNR / FIXTURE_PSNR_MC and produced here."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_cases as HC  # noqa: E402
import ncsense_cases as NC  # noqa: E402
import ncsense_ref as SR  # noqa: E402
import nufft_ref as NR  # noqa: E402
import toeplitz_cases as TC  # noqa: E402
import toeplitz_ref as T  # noqa: E402

from dt4image_restoration_amd import _lib, engine, env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
MODEL_ERR = (1.2e-5, 4.9e-4, 9.0e-4, 1.8e-5, 1.2e-7)           # the NUFFT model against the exact operator, per case (the issue's table)


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(TC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(TC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_TOEPLITZ) and len(names) == 10
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in TC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_TOEPLITZ[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{TC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_TOEPLITZ[name][1]     # bound by _lib.load()'s loop
    assert {n for n, (c, _) in TC.ENTRY_POINTS.items() if c == HC.STATELESS} == {"pnp_toeplitz_planned", "pnp_toeplitz_live"}
    assert {n for n, (c, _) in TC.ENTRY_POINTS.items() if c == HC.REPLACES} == {n for n in TC.ENTRY_POINTS if n.endswith("_tz")} | {"pnp_toeplitz_plan"}
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_toeplitz.py")).read()
    for name, (cls, _) in TC.ENTRY_POINTS.items():
        if cls != HC.STATELESS:
            assert f"def {TC.COVERED_BY[name]}(" in gpu, name
    assert '#include "pnpadmm_ncsense.h"' in text and 'extern "C"' in text
    for gone in TC.ENTRY_POINTS:                                                    # deleting any row of the table is noticed
        assert TC.missing(names, {k: v for k, v in TC.ENTRY_POINTS.items() if k != gone}) == [gone]
    assert TC.missing(names) == []


def test_the_two_older_headers_and_tables_are_the_sets_they_were():
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) == sorted(HC.ENTRY_POINTS) and len(old) == 57
    ns = HC.header_functions(_header(NC.HEADER))
    assert ns == sorted(_lib.SIGNATURES_NCSENSE) == sorted(NC.ENTRY_POINTS) and len(ns) == 8
    new = set(TC.ENTRY_POINTS)
    assert not new & set(old) and not new & set(ns)
    assert "toeplitz" not in _header("pnpadmm.h").lower() and "toeplitz" not in _header(NC.HEADER).lower()


def test_build_files_the_kernel_unit_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\btoeplitz_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_toeplitz_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*pnpadmm_toeplitz\.h", mk, flags=re.M)) == 2      # both dependency lists
    unit = open(os.path.join(CSRC, "toeplitz_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    tune = open(os.path.join(CSRC, "conv_kernels.hip")).read()
    m = re.search(r"^Tuning tuning_from_env\(\) \{$.*?^\}$", tune, re.S | re.M)
    assert m and 'getenv("PNP_TOEPLITZ_NAIVE")' in m.group(0)                        # read where every other switch is read
    for name, params in (("toeplitz_plan", ["self", "weights"]), ("toeplitz_spectrum", ["self"]), ("toeplitz_apply", ["self", "img"]),
                         ("toeplitz_apply_mc", ["self", "img", "sens"]), ("reset_nc_tz", ["self", "x0", "y", "w", "cg_iters"]),
                         ("set_kspace_nc_tz", ["self", "y", "w", "episode", "cg_iters"]),
                         ("reset_ncsense_tz", ["self", "x0", "y", "sens", "w", "cg_iters"]),
                         ("set_kspace_ncsense_tz", ["self", "y", "sens", "w", "episode", "cg_iters"])):
        assert list(inspect.signature(getattr(engine.PnPEngine, name)).parameters) == params, name
    assert isinstance(engine.PnPEngine.toeplitz_planned, property) and isinstance(engine.PnPEngine.toeplitz_live, property)
    assert inspect.signature(env.PnPEnv.__init__).parameters["nc_normal"].default == "nufft"
    with pytest.raises(ValueError, match="nc_normal"):
        env.PnPEnv(3, None, "cuda", nc_normal="exact")


def test_the_new_header_is_plain_c_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_toeplitz.h"\n'
        "int main(void) {\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    if (pnp_toeplitz_planned(0) != 0 || pnp_toeplitz_live(0) != 0) return 1;\n"
        "    if (pnp_toeplitz_plan(0, y, 1, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 2;\n"
        "    if (pnp_toeplitz_apply(0, y, 0, y + 2, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"batch\")) return 3;\n"
        "    if (pnp_toeplitz_apply_mc(0, y, y + 2, 0, 1, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 4;\n"
        "    if (pnp_set_kspace_nc_tz(0, y, 65, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"cg_iters\")) return 5;\n"
        "    if (pnp_reset_ncsense_tz(0, y, y, y, 4, 0, 4, y, y, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"sens_n\")) return 6;\n"
        "    if (pnp_toeplitz_spectrum(0, y, 0) != PNP_ERR_INVALID || pnp_ncsense_coils(0) != 0) return 7;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f || PNP_TOEPLITZ_MAX_SIDE != 512) return 8;\n"
        '    printf("%s\\n", pnp_version());\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_every_argument_error_that_needs_no_handle_is_reported_without_a_gpu_and_leaves_the_outputs_untouched():
    """Host buffers stand in for device memory: a call that is rejected reads and writes none of it.  (The rejections that read the handle -
    batch > n, sens_n that is neither 1 nor n, no plan, no spectrum, a side above 512 - are made on the GPU by tests/test_gpu_toeplitz.py.)"""
    lib = _lib.load()
    a = np.arange(64, dtype=np.float32)
    b, c, out = a.copy() + 100, a.copy() + 200, np.full(64, 7.0, dtype=np.float32)
    pa, pb, pc, po = (v.ctypes.data for v in (a, b, c, out))
    cases = [
        (lambda: lib.pnp_toeplitz_plan(None, pa, 1, None), b"flags"),
        (lambda: lib.pnp_toeplitz_plan(None, pa, -1, None), b"flags"),
        (lambda: lib.pnp_toeplitz_plan(None, pa, 0, None), b"null handle"),
        (lambda: lib.pnp_toeplitz_plan(None, None, 0, None), b"null handle"),
        (lambda: lib.pnp_toeplitz_spectrum(None, None, None), b"null out"),
        (lambda: lib.pnp_toeplitz_spectrum(None, po, None), b"null handle"),
        (lambda: lib.pnp_toeplitz_apply(None, pa, 0, po, None), b"batch"),
        (lambda: lib.pnp_toeplitz_apply(None, pa, -3, po, None), b"batch"),
        (lambda: lib.pnp_toeplitz_apply(None, None, 1, po, None), b"null img"),
        (lambda: lib.pnp_toeplitz_apply(None, pa, 1, None, None), b"null out"),
        (lambda: lib.pnp_toeplitz_apply(None, po, 1, po, None), b"alias"),
        (lambda: lib.pnp_toeplitz_apply(None, pa, 1, po, None), b"null handle"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 0, 1, 1, po, None), b"coils"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 33, 1, 1, po, None), b"coils"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 4, 0, 1, po, None), b"sens_n"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 4, 1, 0, po, None), b"batch"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, None, pb, 4, 1, 1, po, None), b"null img"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, None, 4, 1, 1, po, None), b"null sens"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 4, 1, 1, None, None), b"null out"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, po, pb, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, po, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_toeplitz_apply_mc(None, pa, pb, 4, 1, 1, po, None), b"null handle"),
        (lambda: lib.pnp_set_kspace_nc_tz(None, pa, 0, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_nc_tz(None, pa, 65, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_nc_tz(None, None, 4, None), b"null y"),
        (lambda: lib.pnp_set_kspace_nc_tz(None, pa, 4, None), b"null handle"),
        (lambda: lib.pnp_reset_nc_tz(None, pa, pb, 0, po, po, po, None), b"cg_iters"),
        (lambda: lib.pnp_reset_nc_tz(None, None, pb, 4, po, po, po, None), b"null x0"),
        (lambda: lib.pnp_reset_nc_tz(None, pa, None, 4, po, po, po, None), b"null y"),
        (lambda: lib.pnp_reset_nc_tz(None, pa, pb, 4, po, None, po, None), b"null x, z or u"),
        (lambda: lib.pnp_reset_nc_tz(None, pa, pb, 4, po, po, po, None), b"null handle"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, pa, pb, 0, 1, 4, None), b"coils"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, pa, pb, 4, 0, 4, None), b"sens_n"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, pa, pb, 4, 1, 65, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, None, pb, 4, 1, 4, None), b"null y"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, pa, None, 4, 1, 4, None), b"null sens"),
        (lambda: lib.pnp_set_kspace_ncsense_tz(None, pa, pb, 4, 1, 4, None), b"null handle"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, pb, pc, 33, 1, 4, po, po, po, None), b"coils"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, pb, pc, 4, 1, 0, po, po, po, None), b"cg_iters"),
        (lambda: lib.pnp_reset_ncsense_tz(None, None, pb, pc, 4, 1, 4, po, po, po, None), b"null x0"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, None, pc, 4, 1, 4, po, po, po, None), b"null y"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, pb, None, 4, 1, 4, po, po, po, None), b"null sens"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, pb, pc, 4, 1, 4, po, po, None, None), b"null x, z or u"),
        (lambda: lib.pnp_reset_ncsense_tz(None, pa, pb, pc, 4, 1, 4, po, po, po, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_toeplitz_planned(None) == 0 and lib.pnp_toeplitz_live(None) == 0
    assert (out == 7.0).all() and np.array_equal(a, np.arange(64, dtype=np.float32)) and np.array_equal(b, a + 100) and np.array_equal(c, a + 200)


def test_the_sanitizer_program_of_the_argument_validation_passes():
    """`make asan_toeplitz`: the instrumented host build of the library (host code only) and tests/asan_toeplitz_host.cpp, a program with its
    own main, run directly."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "asan_toeplitz"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "_asan", "asan_toeplitz_host")], capture_output=True, text=True)
    assert r.returncode == 0 and "asan_toeplitz_host: ok" in r.stdout, r.stdout + r.stderr


# ---- the restatement checks itself ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(NR.CASES)))
def test_the_restatement_is_the_exact_operator_and_the_nufft_model_is_not(i):
    n, h, w, gh, gw, J = NR.CASES[i]
    traj, x, wgt = T.case_traj(i), T.case_image(i), T.case_weights(i).astype(np.float64)
    assert np.array_equal(traj, NR.case_traj(i)) and np.array_equal(x, NR.case_image(i)) and T.case_shape(i) == (n, h, w)
    exact = NR.ndft_adjoint(traj, NR.ndft(traj, x), h, w, wgt)
    rel = lambda a: float(np.linalg.norm(a - exact) / np.linalg.norm(exact))
    K = T.spectrum(traj, h, w, wgt)
    KL = T.spectrum_by_lags(traj, h, w, wgt)
    kmax = np.abs(K).max()
    e64, e32 = rel(T.apply(K, x)), rel(T.apply_f32(K, x))
    P = NR.plan(h, w, gh, gw, J, traj)
    em = rel(NR.adjoint(P, NR.forward(P, x), wgt))
    print(f"case {i} {NR.CASES[i]}: Toeplitz float64 {e64:.3e}, float32 restatement {e32:.3e}, NUFFT model {em:.3e} (recorded {MODEL_ERR[i]:.1e}); "
          f"|K - Re K_lags| / max |K| {np.abs(K - KL.real).max() / kmax:.3e}, |Im K_lags| / max |K| {np.abs(KL.imag).max() / kmax:.3e}, "
          f"min K / max K {K.min() / K.max():.3f}, max B / max |K| {T.spectrum_bound(traj, h, w, wgt).max() / kmax:.3e}")
    assert e64 <= 1e-12 and e32 <= 1e-7
    assert np.abs(K - KL.real).max() <= 1e-12 * kmax and np.abs(KL.imag).max() <= 1e-14 * kmax
    assert 0.5 * MODEL_ERR[i] <= em <= 2 * MODEL_ERR[i]
    assert -0.4 <= K.min() / K.max() <= -0.02                                      # not non-negative
    mu = np.linspace(0.1, 0.5, n)
    assert np.array_equal(T.normal(K, x, mu), T.apply(K, x) + mu[:, None, None] * x)
    one = np.ones((1, h, w), dtype=np.complex128)
    assert np.array_equal(T.apply_mc(K, x, one), T.apply(K, x)) and np.array_equal(T.normal_mc(K, x, one, mu), T.normal(K, x, mu))


def test_the_range_reduction_is_needed_and_the_multi_coil_form_is_exact():
    i = 4                                                                           # samples at k = +-0.5: t = 1.0 against the bin -0.5
    n, h, w = T.case_shape(i)
    traj, wgt = T.case_traj(i), T.case_weights(i).astype(np.float64)
    t = traj[:, 0:1] - ((np.arange(2 * h) - h) / (2.0 * h))[None, :]
    assert (np.abs(t) == 1.0).any()
    d = T.dirichlet(t, h)
    assert np.isfinite(d).all() and (d[np.abs(t) == 1.0] == 2 * h - 1).all()
    S = SR.case_maps(4)                                                             # 9 coils on case 4
    x = T.case_image(i)
    K = T.spectrum(traj, h, w, wgt)
    exact = sum(np.conj(S[c]) * NR.ndft_adjoint(traj, NR.ndft(traj, S[c] * x), h, w, wgt) for c in range(S.shape[0]))
    err = float(np.linalg.norm(T.apply_mc(K, x, S) - exact) / np.linalg.norm(exact))
    print(f"apply_mc against the exact coil operator: relative l2 {err:.3e}")
    assert err <= 1e-12
    assert T.N_CASES == 13 and [T.case_shape(j) for j in range(5, 7)] == [(1, 80, 80), (1, 64, 80)]
    assert sorted({2 * s for j in range(7, 13) for s in T.case_shape(j)[1:]}) == [32, 256, 512, 1024]
    for j in range(5, T.N_CASES):
        assert T.case_traj(j).shape == (NR.SPOKES * 2 * max(T.case_shape(j)[1:]), 2)


def test_the_cg_on_the_toeplitz_operator_and_the_end_to_end_constants():
    i = 4
    n, h, w, gh, gw, J = NR.CASES[i]
    traj, x, wgt = T.case_traj(i), T.case_image(i), T.case_weights(i).astype(np.float64)
    P = NR.plan(h, w, gh, gw, J, traj)
    K = T.spectrum(traj, h, w, wgt)
    y = NR.case_samples(i, P["m"])
    aty, mu = NR.adjoint(P, y, wgt), np.array([0.3, 0.05, 0.6])
    z, u, res = T.prox_dual(K, x.real, x, 0.1 * x, aty, mu, 3)
    zn, un, rn = NR.prox_dual(P, x.real, x, 0.1 * x, aty, mu, 3, wgt)
    d = float(np.abs(z - zn).max() / np.abs(zn).max())
    print(f"three CG iterations, Toeplitz against the NUFFT model (J = 8): max |dz| / max |z| {d:.3e}, cg_res {res} / {rn}")
    assert 0 < d <= 1e-5 and np.array_equal(u, 0.1 * x + x.real - z)
    one = np.ones((1, h, w), dtype=np.complex128)
    z1, u1, r1 = T.prox_dual(K, x.real, x, 0.1 * x, aty, mu, 3, S=one)
    assert np.array_equal(z1, z) and np.array_equal(r1, res)
    # the two fixtures
    t = NR.FIXTURE
    dd, PP = NR.fixture_problem()
    m_, s_ = NR.fixture_schedules()
    xa, p0, p1 = T.admm_tv_nc(dd, PP, m_, s_, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    xb, q0, q1 = NR.admm_tv_nc(dd, PP, m_, s_, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"single-coil fixture: x0 {p0[0]:.3f} dB, Toeplitz stage {p1[0]:.4f} dB, NUFFT stage {q1[0]:.4f} dB, max |dx| {np.abs(xa - xb).max():.2e}")
    assert abs(p0[0] - T.FIXTURE_PSNR[0]) <= 2e-3 and abs(p1[0] - T.FIXTURE_PSNR[1]) <= 2e-3 and np.abs(xa - xb).max() <= 5e-3
    t = SR.FIXTURE
    dd, PP = SR.fixture_problem()
    m_, s_ = SR.fixture_schedules()
    xa, p0, p1 = T.admm_tv_ncmc(dd, PP, m_, s_, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"multi-coil fixture: x0 {p0[0]:.3f} dB, Toeplitz stage {p1[0]:.4f} dB (NUFFT stage recorded {SR.FIXTURE_PSNR[1]})")
    assert abs(p0[0] - T.FIXTURE_PSNR_MC[0]) <= 2e-3 and abs(p1[0] - T.FIXTURE_PSNR_MC[1]) <= 2e-3


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------

def test_cli_nc_normal_and_its_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--nc-normal", "toeplitz"], "--nc-normal toeplitz needs --traj radial"),
                        (["--nc-normal", "toeplitz", "--nc-coils", "2"], "needs --traj radial"),
                        (["--traj", "radial", "--nc-normal", "toeplitz", "--size", "640"], "h, w up to 512"),
                        (["--traj", "radial", "--nc-coils", "2", "--nc-normal", "toeplitz", "--size", "1024"], "h, w up to 512")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit):                                                # argparse: not a choice
        cli.main(base + ["--traj", "radial", "--nc-normal", "exact", "fixed"])
    assert _lib.toeplitz_size_error("f", 512, 16) is None and "640x80" in _lib.toeplitz_size_error("f", 640, 80)
    # the words are the library's: the same format string in pnp_capi.hip
    capi = open(os.path.join(CSRC, "pnp_capi.hip")).read()
    assert "the Toeplitz operator transforms a 2h x 2w grid, so it takes h, w up to %d (got %dx%d)" in capi
