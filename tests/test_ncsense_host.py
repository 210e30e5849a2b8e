"""CPU-only checks of the non-Cartesian SENSE stage: the entry points of include/pnpadmm_ncsense.h are declared, exported, bound from
`_lib.SIGNATURES_NCSENSE` and classified in tests/ncsense_cases.py - the discipline tests/test_entry_point_table_host.py and
tests/test_host_logic.py enforce for include/pnpadmm.h, which gains no function; the header compiles as C99; every argument error that needs
no handle comes back without a GPU and leaves the outputs untouched; the float64 restatement the GPU tests compare against
(tests/ncsense_ref.py) checks itself; the Python layers and the CLI accept the new spelling and keep their remaining refusals.

Restatement: with C = 1 and S = 1 it is tests/nufft_ref.py's; <A p, q> = <p, A^H q> to 1e-12 relative; on the Cartesian-bin trajectory of a
mask (nufft_ref.mask_traj, J = 8, 16 -> 32) A agrees with tests/sense_ref.py's A to the model error tests/test_nufft_host.py records for that
grid and width (9.728e-08 relative l2 against the exact transform; twice that is asserted, as there).

End-to-end fixture (ncsense_ref.FIXTURE: one 64 x 64 phantom, 4 coils of synthetic.coil_maps, 12 golden-angle spokes, ramp dcf, noise 5/255,
mu 0.3, sigma_d 50/255 -> 5/255 over 20 iterations, K = 8, TV(1, 20)): the float64 restatement goes from 17.493 dB (x0) to 32.399 dB; the
condition on the input is a gain of at least 3 dB.

Which tests need the feature: the self-checks of the restatement exercise tests/ncsense_ref.py (and synthetic.make_problem_ncmc); every other
test needs the new header, the new symbols or the new Python functions."""
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
import ncsense_ref as R  # noqa: E402
import nufft_ref as NR  # noqa: E402
import sense_ref  # noqa: E402

from dt4image_restoration_amd import _lib, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
MODEL_ERR_J8_16 = 9.728e-08                                 # tests/test_nufft_host.py: J = 8 on 16 -> 32 against the exact NDFT


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(NC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(NC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_NCSENSE)
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in NC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_NCSENSE[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{NC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_NCSENSE[name][1]      # bound by _lib.load()'s loop
    assert {n for n, (c, _) in NC.ENTRY_POINTS.items() if c == HC.REPLACES} == {"pnp_set_kspace_ncsense", "pnp_reset_ncsense"}
    assert {n for n, (c, _) in NC.ENTRY_POINTS.items() if c == HC.STATELESS} == {"pnp_ncsense_coils"}
    assert all(c in (HC.REPLACES, HC.STATELESS, HC.INTRUDER) for c, _ in NC.ENTRY_POINTS.values())
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_ncsense.py")).read()
    for name, (cls, _) in NC.ENTRY_POINTS.items():
        if cls != HC.STATELESS:
            assert f"def {NC.COVERED_BY[name]}(" in gpu, name
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text


def test_deleting_any_row_of_the_new_table_is_noticed():
    names = HC.header_functions(_header(NC.HEADER))
    for gone in NC.ENTRY_POINTS:
        table = {k: v for k, v in NC.ENTRY_POINTS.items() if k != gone}
        assert NC.missing(names, table) == [gone]
    assert NC.missing(names) == []


def test_the_old_header_and_the_old_binding_are_the_sets_they_were():
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) == sorted(HC.ENTRY_POINTS)
    assert not set(old) & set(NC.ENTRY_POINTS) and not set(_lib.SIGNATURES) & set(_lib.SIGNATURES_NCSENSE)
    assert len(old) == 57 and "ncsense" not in _header("pnpadmm.h")


def test_build_files_and_the_kernel_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bncsense_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_ncsense_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*pnpadmm_ncsense\.h", mk, flags=re.M)) == 2       # both dependency lists
    unit = open(os.path.join(CSRC, "ncsense_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    for name, params in (("nufft_forward_mc", ["self", "img", "sens"]), ("nufft_adjoint_mc", ["self", "samples", "sens", "weights"]),
                         ("reset_ncsense", ["self", "x0", "y", "sens", "w", "cg_iters"]),
                         ("set_kspace_ncsense", ["self", "y", "sens", "w", "episode", "cg_iters"]), ("ncsense_normal", ["self", "p", "mu"]),
                         ("ncsense_cg_residual", ["self"]), ("acquire_ncsense", ["self", "gt", "sens", "sigma_n", "seed", "dcf"])):
        assert list(inspect.signature(getattr(engine.PnPEngine, name)).parameters) == params, name
    assert isinstance(engine.PnPEngine.ncsense_coils, property)


def test_the_new_header_is_plain_c_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_ncsense.h"\n'
        "int main(void) {\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    if (pnp_ncsense_coils(0) != 0) return 1;\n"
        "    if (pnp_nufft_forward_mc(0, y, y + 2, 0, 1, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 2;\n"
        "    if (pnp_set_kspace_ncsense(0, y, y, 4, 1, 0, 65, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"cg_iters\")) return 3;\n"
        "    if (pnp_acquire_ncsense(0, y, y, 4, 1, 0, 0.1, 1u, 1, y, 0, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 4;\n"
        "    if (pnp_ncsense_normal(0, y, y, y, 0) != PNP_ERR_INVALID) return 5;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f) return 6;\n"
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
    batch > n, sens_n that is neither 1 nor n, a call without a plan - are made on the GPU by tests/test_gpu_ncsense.py.)"""
    lib = _lib.load()
    a = np.arange(64, dtype=np.float32)
    b, c, out = a.copy() + 100, a.copy() + 200, np.full(64, 7.0, dtype=np.float32)
    pa, pb, pc, po = (v.ctypes.data for v in (a, b, c, out))
    nan, inf = float("nan"), float("inf")
    cases = [
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 0, 1, 1, po, None), b"coils"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 33, 1, 1, po, None), b"coils"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 4, 0, 1, po, None), b"sens_n"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 4, 1, 0, po, None), b"batch"),
        (lambda: lib.pnp_nufft_forward_mc(None, None, pb, 4, 1, 1, po, None), b"null img"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, None, 4, 1, 1, po, None), b"null sens"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 4, 1, 1, None, None), b"null samples"),
        (lambda: lib.pnp_nufft_forward_mc(None, po, pb, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, po, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_nufft_forward_mc(None, pa, pb, 4, 1, 1, po, None), b"null handle"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, pb, 0, 1, 1, po, None), b"coils"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, pb, 4, -1, 1, po, None), b"sens_n"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, pb, 4, 1, 0, po, None), b"batch"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, None, None, pb, 4, 1, 1, po, None), b"null samples"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, None, 4, 1, 1, po, None), b"null sens"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, pb, 4, 1, 1, None, None), b"null img"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, po, None, pb, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, po, pb, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, po, 4, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_nufft_adjoint_mc(None, pa, None, pb, 4, 1, 1, po, None), b"null handle"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, pb, 0, 1, None, 4, None), b"coils"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, pb, 4, 0, None, 4, None), b"sens_n"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, pb, 4, 1, None, 0, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, pb, 4, 1, None, 65, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_ncsense(None, None, pb, 4, 1, None, 4, None), b"null y"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, None, 4, 1, None, 4, None), b"null sens"),
        (lambda: lib.pnp_set_kspace_ncsense(None, pa, pb, 4, 1, None, 4, None), b"null handle"),
        (lambda: lib.pnp_reset_ncsense(None, pa, pb, pc, 33, 1, None, 4, po, po, po, None), b"coils"),
        (lambda: lib.pnp_reset_ncsense(None, pa, pb, pc, 4, 1, None, 0, po, po, po, None), b"cg_iters"),
        (lambda: lib.pnp_reset_ncsense(None, None, pb, pc, 4, 1, None, 4, po, po, po, None), b"null x0"),
        (lambda: lib.pnp_reset_ncsense(None, pa, None, pc, 4, 1, None, 4, po, po, po, None), b"null y"),
        (lambda: lib.pnp_reset_ncsense(None, pa, pb, None, 4, 1, None, 4, po, po, po, None), b"null sens"),
        (lambda: lib.pnp_reset_ncsense(None, pa, pb, pc, 4, 1, None, 4, None, po, po, None), b"null x, z or u"),
        (lambda: lib.pnp_reset_ncsense(None, pa, pb, pc, 4, 1, None, 4, po, po, po, None), b"null handle"),
        (lambda: lib.pnp_ncsense_cg_residual(None, po, None), b"null argument"),
        (lambda: lib.pnp_ncsense_normal(None, pa, pb, po, None), b"null argument"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, 0.1, 1, 1, po, None, None, None), b"flags"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, -0.1, 1, 0, po, None, None, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, nan, 1, 0, po, None, None, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, inf, 1, 0, po, None, None, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 0, 1, None, 0.1, 1, 0, po, None, None, None), b"coils"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 0, None, 0.1, 1, 0, po, None, None, None), b"sens_n"),
        (lambda: lib.pnp_acquire_ncsense(None, None, pb, 4, 1, None, 0.1, 1, 0, po, None, None, None), b"null gt"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, None, 4, 1, None, 0.1, 1, 0, po, None, None, None), b"null sens"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, 0.1, 1, 0, None, None, None, None), b"null y"),
        (lambda: lib.pnp_acquire_ncsense(None, po, pb, 4, 1, None, 0.1, 1, 0, po, None, None, None), b"alias"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, 0.1, 1, 0, po, po, None, None), b"alias"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, 0.1, 1, 0, po, None, pa, None), b"alias"),
        (lambda: lib.pnp_acquire_ncsense(None, pa, pb, 4, 1, None, 0.1, 1, 0, po, None, None, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_ncsense_coils(None) == 0
    assert (out == 7.0).all() and np.array_equal(a, np.arange(64, dtype=np.float32)) and np.array_equal(b, a + 100) and np.array_equal(c, a + 200)


# ---- the restatement checks itself ---------------------------------------------------------------------------------------------------------

def test_one_unit_map_is_the_single_coil_restatement():
    i = 4
    n, h, w, gh, gw, J = NR.CASES[i]
    P = NR.plan(h, w, gh, gw, J, NR.case_traj(i))
    x, y = NR.case_image(i), NR.case_samples(i, P["m"])
    S = np.ones((1, h, w), dtype=np.complex128)
    wgt = 0.5 + np.abs(NR.case_samples(i, P["m"], seed=1)[0].real)
    mu = np.array([0.3, 0.05, 0.6])
    assert np.array_equal(R.A(P, x, S)[:, 0], NR.forward(P, x))
    assert np.array_equal(R.AH(P, y[:, None], S, wgt), NR.adjoint(P, y, wgt))
    assert np.array_equal(R.normal(P, x, S, mu, wgt), NR.normal(P, x, mu, wgt))
    aty = NR.adjoint(P, y, wgt)
    z1, u1, r1 = R.prox_dual(P, x.real, x, 0.1 * x, aty, S, mu, 3, wgt)
    z0, u0, r0 = NR.prox_dual(P, x.real, x, 0.1 * x, aty, mu, 3, wgt)
    assert np.array_equal(z1, z0) and np.array_equal(u1, u0) and np.array_equal(r1, r0)
    assert np.array_equal(R.dc_misfit(P, x.real, y[:, None], S, wgt), NR.dc_misfit(P, x.real, y, wgt))
    assert abs(R.op_norm(P, S) - NR.op_norm(P)) <= 1e-12 * NR.op_norm(P)


@pytest.mark.parametrize("k", range(len(R.CASES)))
def test_the_model_is_exactly_adjoint(k):
    i, c = R.CASES[k]
    n, h, w, gh, gw, J = NR.CASES[i]
    P = NR.plan(h, w, gh, gw, J, NR.case_traj(i))
    x, y = NR.case_image(i, seed=k), R.case_samples(k, P["m"])
    wgt = 0.5 + np.abs(NR.case_samples(i, P["m"], seed=1)[0].real)
    for S in (R.case_maps(k), R.case_maps(k, per_slice=True)):
        assert S.shape[-3:] == (c, h, w)
        for wv in (None, wgt):
            lhs = np.vdot(R.A(P, x, S) * (1.0 if wv is None else wv), y)
            rhs = np.vdot(x, R.AH(P, y, S, wv))
            print(f"case {k} (C = {c}): <W A x, y> - <x, A^H W y> = {abs(lhs - rhs):.3e} of {abs(lhs):.3e}")
            assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert sorted({cc for _, cc in R.CASES}) == [1, 3, 5, 9, 32] and {ii for ii, _ in R.CASES} == set(range(len(NR.CASES)))


def test_on_cartesian_bins_the_operator_is_the_cartesian_multi_coil_operator():
    n, h, w, c, J = 2, 16, 16, 3, 8
    mask = synthetic.radial_mask(h, w, 4.0)
    traj, (jj, ll) = NR.mask_traj(mask)
    P = NR.plan(h, w, 32, 32, J, traj)
    S = synthetic.coil_maps(c, h, w)
    x = NR.case_image(0)
    ref = sense_ref.A(x, S, mask)[:, :, jj, ll]                                     # [N,C,sampled bins]
    got = R.A(P, x, S)
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"A on the Cartesian bins of a mask against sense_ref.A: relative l2 {err:.3e} (recorded model error {MODEL_ERR_J8_16:.3e})")
    assert err <= 2 * MODEL_ERR_J8_16
    y = np.zeros((n, c, h, w), dtype=np.complex128)
    y[:, :, jj, ll] = R.case_samples(0, len(jj))[:, :c]
    ra = sense_ref.AH(y, S, mask)
    ea = float(np.linalg.norm(R.AH(P, y[:, :, jj, ll], S) - ra) / np.linalg.norm(ra))
    print(f"A^H: relative l2 {ea:.3e}")
    assert ea <= 2 * MODEL_ERR_J8_16


def test_the_float64_problem_and_the_acquisition_of_the_restatement_agree():
    from dt4image_restoration_amd import acquisition
    h, w, c, spokes = 16, 32, 3, 5
    t = acquisition.radial_trajectory(h, w, spokes)
    d = acquisition.radial_dcf(t, h, w)
    p = synthetic.make_problem_ncmc(2, h, w, c, t, dcf=d, sigma_n=0.1, seed=3)
    assert p["y0"].shape == (2, c, t.shape[0], 2) and p["ATy0"].shape == (2, 1, h, w, 2) and p["sens"].shape == (c, h, w)
    assert p["sens"].dtype == np.complex64 and np.array_equal(p["x0"], np.clip(p["ATy0"], 0, None))
    y = p["y0"][..., 0].astype(np.float64) + 1j * p["y0"][..., 1]
    ref = R.acquire(t, p["gt"][:, 0], p["sens"], 0.1, 3)
    assert np.abs(y - ref).max() <= 1e-6                                           # float32 storage of an O(1) value
    one = synthetic.make_problem_ncmc(1, h, w, c, t, dcf=d, sigma_n=0.1, seed=3, first_slice=1)
    assert np.array_equal(one["y0"][0], p["y0"][1])                                 # a slice depends on (seed, its index) only
    sc = synthetic.make_problem_nc(2, h, w, t, dcf=d, sigma_n=0.1, seed=3)          # one unit map: the single-coil problem, coil 0's noise
    u = synthetic.make_problem_ncmc(2, h, w, 1, t, dcf=d, sigma_n=0.1, seed=3, sens=np.ones((1, h, w)))
    assert np.array_equal(u["y0"], sc["y0"]) and np.array_equal(u["ATy0"], sc["ATy0"])


def test_the_end_to_end_fixture_gains_what_the_gpu_test_records():
    t = R.FIXTURE
    d, P = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    x, p0, p1 = R.admm_tv(d, P, mu, sig, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"float64 TV-ADMM, {t['coils']} coils on {t['spokes']} golden spokes: PSNR of x0 {p0[0]:.3f} dB, final {p1[0]:.3f} dB, gain {p1[0] - p0[0]:.3f} dB")
    assert p1[0] - p0[0] >= 3.0
    assert abs(p0[0] - R.FIXTURE_PSNR[0]) <= 2e-3 and abs(p1[0] - R.FIXTURE_PSNR[1]) <= 2e-3
    assert (P["gh"], P["gw"], P["m"]) == (80, 80, t["spokes"] * 128) and d["sens"].shape == (t["coils"], 64, 64)


# ---- Python layers and the CLI ---------------------------------------------------------------------------------------------------------------

def test_cli_nc_coils_and_the_refusals_that_remain():
    from dt4image_restoration_amd import acquisition, cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--traj", "radial", "--coils", "4"], "--traj with --coils"), (["--traj", "radial", "--coils", "4"], "--nc-coils"),
                        (["--nc-coils", "4"], "--nc-coils needs --traj radial"), (["--traj", "radial", "--nc-coils", "33"], "--nc-coils must be 1..32"),
                        (["--traj", "radial", "--nc-coils", "-1"], "--nc-coils must be 1..32"),
                        (["--traj", "radial", "--nc-coils", "4", "--sens", "estimate"], "needs --coils"),
                        (["--traj", "radial", "--nc-coils", "4", "--compress", "2"], "needs --coils"),
                        (["--traj", "radial", "--nc-coils", "4", "--mask", "cartesian"], "--traj takes no --mask")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit):                                                # argparse: not a number
        cli.main(base + ["--traj", "radial", "--nc-coils", "four", "fixed"])
    assert "coils" in inspect.signature(acquisition.task_problem).parameters
    assert "sens=None" in str(inspect.signature(acquisition._simulate_nc))
    # what stays refused: a noise covariance or a mask with the trajectory (before any GPU is asked for)
    with pytest.raises(ValueError, match="radial-nc"):
        acquisition.task_problem("4x_5", np.zeros((1, 16, 16), dtype=np.float32), None, mask_kind="radial-nc", coils=4, noise_cov=np.eye(4))
    with pytest.raises(ValueError, match="radial-nc"):
        acquisition.task_problem("4x_5", np.zeros((1, 16, 16), dtype=np.float32), None, mask_kind="radial-nc", coils=4, mask=np.ones((16, 16)))
