"""CPU-only checks of the off-resonance correction for multi-coil data: the entry points of include/pnpadmm_offres_mc.h are declared,
exported, bound from `_lib.SIGNATURES_OFFRES_MC` and classified in tests/offres_mc_cases.py, while the older headers and tables stay the sets
they were; the header compiles as C99 with -pedantic -Werror and links from C; every argument error that needs no handle comes back from
ctypes without a GPU and leaves the outputs untouched; the build files and the Python layer carry the new unit and names; the float64
restatement of tests/offres_mc_ref.py is held to the exact per-coil NDFT with exp(-i omega t); the fixture figures of the GPU test.

The rejections that read the handle - no plan, sens_n / map_n not 1 or n - need a handle, and pnp_create needs a device:
tests/test_gpu_offres_mc.py makes them.

BOUNDS of the restatement against the exact operator, per sample and coil, in the units of the orthonormal operator (1 / sqrt(H W)):
  L = 1 (case A as it stands): |exp(-i omega t) - exp(-i omega tau)| = 2 |sin(omega (t - tau) / 2)| <= 2 sin(min(omega_max span / 4, pi / 2)),
  times ||S_c . p||_1;   L > 1 (case A's geometry, 12 segments): offres_ref.bound, (1 - cos(omega_max D / 2)) ||S_c . p||_1."""
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
import ncsense_cases as NC  # noqa: E402
import nufft_ref as NR  # noqa: E402
import offres_cases as OC  # noqa: E402
import offres_ls_ref as LS  # noqa: E402
import offres_mc_cases as MC  # noqa: E402
import offres_mc_ref as MR  # noqa: E402
import offres_ref as OR  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
NAMES = ["pnp_acquire_offres_mc", "pnp_offres_adjoint_mc", "pnp_offres_forward_mc", "pnp_offres_mc_cg_residual", "pnp_offres_mc_coils",
         "pnp_offres_mc_normal", "pnp_reset_offres_mc", "pnp_set_kspace_offres_mc"]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(MC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(MC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_OFFRES_MC) == NAMES
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in MC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_OFFRES_MC[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{MC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_OFFRES_MC[name][1]       # bound by _lib.load()'s loop
        assert cls in (HC.INTRUDER, HC.REPLACES, HC.STATELESS)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_offres_mc.py")).read()
    for name, (cls, _) in MC.ENTRY_POINTS.items():
        if cls != HC.STATELESS:
            assert f"def {MC.COVERED_BY[name]}(" in gpu and name in gpu, name
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    for gone in MC.ENTRY_POINTS:                                                    # deleting any row of the table is noticed
        assert MC.missing(names, {k: v for k, v in MC.ENTRY_POINTS.items() if k != gone}) == [gone]
    assert MC.missing(names) == []
    for word in ("THE MODEL", "EXPRESSION ORDER", "PNP_OFFRES_MC_NAIVE", "PNP_OFFRES_MC_COIL_BLOCK", "PNP_OFFRES_SEG_BLOCK", "NO BIT DEPENDS ON SB OR CBc",
                 "65535", "PNP_ERR_STATE", "leaving the outputs untouched"):
        assert word in text, word
    # the exports of the built library, by its dynamic symbol table
    if shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, syms, flags=re.M), name


def test_the_older_headers_and_tables_are_the_sets_they_were():
    new = set(MC.ENTRY_POINTS)
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) and len(old) == 57
    ns = HC.header_functions(_header(NC.HEADER))
    assert ns == sorted(_lib.SIGNATURES_NCSENSE) == sorted(NC.ENTRY_POINTS) and len(ns) == 8
    orr = HC.header_functions(_header(OC.HEADER))
    assert orr == sorted(_lib.SIGNATURES_OFFRES) == sorted(OC.ENTRY_POINTS) and len(orr) == 11
    ls = HC.header_functions(_header("pnpadmm_offres_ls.h"))
    assert ls == sorted(_lib.SIGNATURES_OFFRES_LS) and len(ls) == 3
    for older in (old, ns, orr, ls, sorted(_lib.SIGNATURES_TOEPLITZ), sorted(_lib.SIGNATURES_DCF), sorted(_lib.SIGNATURES_FIELDMAP)):
        assert not new & set(older)
    # the single-coil header points here where it says coils times segments are out of scope; its declarations are untouched
    assert "pnpadmm_offres_mc.h" in _header(OC.HEADER) and "OUT OF SCOPE" in _header(OC.HEADER)
    assert _lib.PNP_OFFRES_MC_COIL_BLOCK == 4


def test_build_files_the_unit_and_the_python_layer():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\boffres_mc_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_offres_mc_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*pnpadmm_offres_mc\.h", mk, flags=re.M)) == 2                       # both dependency lists
    unit = open(os.path.join(CSRC, "offres_mc_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()                                       # a launch ends; the next starts
    for kernel in ("offres_mc_pad_kernel", "offres_mc_crop_kernel"):
        assert f"void {kernel}(" in unit
    internal = open(os.path.join(CSRC, "pnp_internal.h")).read()
    assert "kOffresMcBlock = 4" in internal and "PNP_OFFRES_MC_COIL_BLOCK" in internal and "PNP_OFFRES_MC_NAIVE" in internal
    capi = open(os.path.join(CSRC, "pnp_capi.hip")).read()
    assert "STAGE_ORS" in capi and "int map_n = 1;" in capi                         # a field of its own, not an overloaded sens_n
    P = engine.PnPEngine
    for name, params in (("offres_forward_mc", ["self", "img", "maps", "sens"]), ("offres_adjoint_mc", ["self", "samples", "maps", "sens", "weights"]),
                         ("reset_offres_mc", ["self", "x0", "y", "sens", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres_mc", ["self", "y", "sens", "omega", "w", "episode", "cg_iters"]),
                         ("offres_mc_normal", ["self", "p", "mu"]), ("offres_mc_cg_residual", ["self"]),
                         ("acquire_offres_mc", ["self", "gt", "sens", "omega", "sigma_n", "seed", "dcf"])):
        assert list(inspect.signature(getattr(P, name)).parameters) == params, name
    assert isinstance(P.offres_mc_coils, property)
    sig = inspect.signature(P.reset_offres_mc).parameters
    assert sig["w"].default is None and sig["cg_iters"].default == 8
    assert inspect.signature(P.offres_adjoint_mc).parameters["weights"].default is None
    assert inspect.signature(P.acquire_offres_mc).parameters["dcf"].default is None
    # the layers above keep their parameter orders and their refusal of a field map together with coil maps
    assert list(inspect.signature(P.reset).parameters)[:6] == ["self", "x0", "y0", "mask", "sens", "cg_iters"]
    mk0 = inspect.signature(synthetic.make_problem_ncmcb0).parameters
    assert list(mk0) == ["n", "h", "w", "coils", "traj", "times", "omega", "dcf", "sigma_n", "seed", "first_slice", "sens"]
    assert mk0["dcf"].default is None and mk0["sens"].default is None and mk0["seed"].default == 1234


def test_the_new_header_is_plain_c99_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_offres_mc.h"\n'
        "int main(void) {\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};\n"
        "    if (pnp_offres_forward_mc(0, a, b, 1, b, 1, 0, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 1;\n"
        "    if (pnp_offres_forward_mc(0, a, b, 1, b, 1, PNP_MC_MAX_COILS + 1, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 2;\n"
        "    if (pnp_offres_forward_mc(0, a, b, 0, b, 1, 2, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"map_n\")) return 3;\n"
        "    if (pnp_offres_forward_mc(0, a, b, 1, b, 0, 2, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"sens_n\")) return 4;\n"
        "    if (pnp_offres_forward_mc(0, a, b, 1, b, 1, 2, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 5;\n"
        "    if (pnp_offres_mc_coils(0) != 0) return 6;\n"
        "    if (pnp_offres_mc_cg_residual(0, y, 0) != PNP_ERR_INVALID) return 7;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f) return 8;\n"
        '    printf("%s\\n", pnp_version());\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_every_argument_error_that_needs_no_handle_is_reported_without_a_gpu_and_leaves_the_outputs_untouched():
    """Host buffers stand in for device memory: a call that is rejected reads and writes none of it."""
    lib = _lib.load()
    a = np.arange(64, dtype=np.float32)
    b = np.arange(64, dtype=np.float32) + 100.0
    s = np.arange(64, dtype=np.float32) + 200.0
    out, out2, out3 = (np.full(64, 7.0, dtype=np.float32) for _ in range(3))
    pa, pb, ps, po, po2, po3 = (v.ctypes.data for v in (a, b, s, out, out2, out3))
    nan, inf = float("nan"), float("inf")
    fwd, adj, ins, rst, acq = (lib.pnp_offres_forward_mc, lib.pnp_offres_adjoint_mc, lib.pnp_set_kspace_offres_mc, lib.pnp_reset_offres_mc,
                               lib.pnp_acquire_offres_mc)
    cases = [
        (lambda: fwd(None, pa, pb, 1, ps, 1, 0, 1, po, None), b"coils must be 1..32 (got 0)"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 33, 1, po, None), b"coils must be 1..32 (got 33)"),
        (lambda: fwd(None, None, pb, 1, ps, 1, -1, 1, po, None), b"coils"),                 # scalar ranges first
        (lambda: fwd(None, pa, pb, 1, ps, 0, 2, 1, po, None), b"sens_n must be 1 or n (got 0)"),
        (lambda: fwd(None, pa, pb, 0, ps, 1, 2, 1, po, None), b"map_n must be 1 or n (got 0)"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 2, 0, po, None), b"batch must be 1..n (got 0)"),
        (lambda: fwd(None, None, pb, 1, ps, 1, 2, 1, po, None), b"null img"),
        (lambda: fwd(None, pa, None, 1, ps, 1, 2, 1, po, None), b"null maps"),
        (lambda: fwd(None, pa, pb, 1, None, 1, 2, 1, po, None), b"null sens"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 2, 1, None, None), b"null samples"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 2, 1, pa, None), b"alias"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 2, 1, pb, None), b"alias"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 2, 1, ps, None), b"alias"),
        (lambda: fwd(None, pa, pb, 1, ps, 1, 32, 1, po, None), b"null handle"),
        (lambda: adj(None, pa, None, pb, 1, ps, 1, 0, 1, po, None), b"coils"),
        (lambda: adj(None, pa, None, pb, -3, ps, 1, 2, 1, po, None), b"map_n"),
        (lambda: adj(None, pa, None, pb, 1, ps, -1, 2, 1, po, None), b"sens_n"),
        (lambda: adj(None, pa, None, pb, 1, ps, 1, 2, -1, po, None), b"batch"),
        (lambda: adj(None, None, None, pb, 1, ps, 1, 2, 1, po, None), b"null samples"),
        (lambda: adj(None, pa, None, None, 1, ps, 1, 2, 1, po, None), b"null maps"),
        (lambda: adj(None, pa, None, pb, 1, None, 1, 2, 1, po, None), b"null sens"),
        (lambda: adj(None, pa, None, pb, 1, ps, 1, 2, 1, None, None), b"null img"),
        (lambda: adj(None, pa, po, pb, 1, ps, 1, 2, 1, po, None), b"alias"),
        (lambda: adj(None, pa, None, pb, 1, ps, 1, 2, 1, ps, None), b"alias"),
        (lambda: adj(None, pa, None, pb, 1, ps, 1, 2, 1, po, None), b"null handle"),
        (lambda: ins(None, pa, ps, 0, 1, pb, 1, None, 8, None), b"coils"),
        (lambda: ins(None, pa, ps, 2, 0, pb, 1, None, 8, None), b"sens_n"),
        (lambda: ins(None, pa, ps, 2, 1, pb, 0, None, 8, None), b"map_n"),
        (lambda: ins(None, pa, ps, 2, 1, pb, 1, None, 0, None), b"cg_iters must be 1..64 (got 0)"),
        (lambda: ins(None, pa, ps, 2, 1, pb, 1, None, 65, None), b"cg_iters"),
        (lambda: ins(None, None, ps, 2, 1, pb, 1, None, 8, None), b"null y"),
        (lambda: ins(None, pa, None, 2, 1, pb, 1, None, 8, None), b"null sens"),
        (lambda: ins(None, pa, ps, 2, 1, None, 1, None, 8, None), b"null omega"),
        (lambda: ins(None, pa, ps, 2, 1, pb, 1, None, 8, None), b"null handle"),
        (lambda: rst(None, None, pa, ps, 2, 1, pb, 1, None, 8, po, po2, po3, None), b"null x0"),
        (lambda: rst(None, pa, None, ps, 2, 1, pb, 1, None, 8, po, po2, po3, None), b"null y"),
        (lambda: rst(None, pa, pa, None, 2, 1, pb, 1, None, 8, po, po2, po3, None), b"null sens"),
        (lambda: rst(None, pa, pa, ps, 2, 1, None, 1, None, 8, po, po2, po3, None), b"null omega"),
        (lambda: rst(None, pa, pa, ps, 2, 1, pb, 1, None, 8, None, po2, po3, None), b"null x, z or u"),
        (lambda: rst(None, pa, pa, ps, 2, 1, pb, 1, None, 8, po, po2, None, None), b"null x, z or u"),
        (lambda: rst(None, pa, pa, ps, 2, 1, pb, 1, None, 8, po, po2, po3, None), b"null handle"),
        (lambda: lib.pnp_offres_mc_cg_residual(None, po, None), b"null argument"),
        (lambda: lib.pnp_offres_mc_normal(None, pa, pb, po, None), b"null argument"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, 0.0, 0, 1, po, po2, po3, None), b"flags"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, -1.0, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, nan, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, inf, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: acq(None, pa, ps, 0, 1, pb, 1, None, 0.0, 0, 0, po, po2, po3, None), b"coils"),
        (lambda: acq(None, pa, ps, 2, 0, pb, 1, None, 0.0, 0, 0, po, po2, po3, None), b"sens_n"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 0, None, 0.0, 0, 0, po, po2, po3, None), b"map_n"),
        (lambda: acq(None, None, ps, 2, 1, pb, 1, None, 0.0, 0, 0, po, po2, po3, None), b"null gt"),
        (lambda: acq(None, pa, None, 2, 1, pb, 1, None, 0.0, 0, 0, po, po2, po3, None), b"null sens"),
        (lambda: acq(None, pa, ps, 2, 1, None, 1, None, 0.0, 0, 0, po, po2, po3, None), b"null omega"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, 0.0, 0, 0, None, po2, po3, None), b"null y"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, 0.0, 0, 0, po, po, po3, None), b"alias"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, 0.0, 0, 0, po, ps, po3, None), b"alias"),
        (lambda: acq(None, pa, ps, 2, 1, pb, 1, None, 0.0, 0, 0, po, None, None, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_offres_mc_coils(None) == 0
    for o in (out, out2, out3):
        assert (o == 7.0).all()
    for v, off in ((a, 0.0), (b, 100.0), (s, 200.0)):
        assert np.array_equal(v, np.arange(64, dtype=np.float32) + off)


# ---- the cases and the restatement -------------------------------------------------------------------------------------------------------------

def test_the_cases_are_the_shapes_at_which_the_block_logic_can_go_wrong():
    c = MC.CASES
    assert sorted(c) == list("ABCDE")
    assert (c["A"]["C"], c["A"]["L"]) == (1, 1) and MR.case_traj(c["A"])[0].shape[0] == 96
    assert c["C"]["C"] == 4 + 1 and c["C"]["L"] == 8 + 1 and c["D"]["C"] == 4 + 4 + 1 and c["D"]["L"] == 8 and c["E"]["L"] == 8 + 3
    assert {v["plan"] for v in c.values()} == {"linear", "ls"} and c["D"]["plan"] == c["E"]["plan"] == "ls"
    assert {(v["sens_n"], v["map_n"]) for v in c.values()} == {(1, 1), (1, "n"), ("n", 1), ("n", "n")}
    assert c["D"]["grid"][1] % 5 == 0 and c["D"]["J"] == 8                         # a mixed-radix side
    assert MC.COIL_BLOCKS == (1, 2, 4) and MC.SEG_BLOCKS == (1, 3, 8)
    S = MR.dyadic_sens(5, 4, 4)
    p = (np.float32(0.3) + 1j * np.float32(-1.7))
    for k in range(5):                                                              # S_c . p is exact in float32
        assert complex(np.complex64(S[k, 0, 0] * p)) == S[k, 0, 0] * complex(p)


def test_the_restatement_against_the_exact_per_coil_operator_on_case_a():
    c = dict(MC.CASES["A"], C=3)                                                    # case A's geometry; three coils so that the coil index is exercised
    h, w, n = c["h"], c["w"], c["n"]
    traj, t = MR.case_traj(c)
    om = MR.case_omega(c).astype(np.float64)
    S = MR.case_sens(c)
    x, _, _ = MR.case_data(c, traj.shape[0])
    ex = MR.exact_forward(traj, t, om, S, x)
    assert ex.shape == (n, 3, 96)
    one = OR.exact_forward(traj, t, om, S[1] * x)                                   # a coil plane is the single-coil operator on S_c . p
    assert np.array_equal(ex[:, 1], one)
    span, om_max = float(t.max() - t.min()), float(np.abs(om).max())
    l1 = np.abs(S[None] * x[:, None]).reshape(n, 3, -1).sum(axis=2) / math.sqrt(h * w)
    for L in (1, 12):
        Q = OR.plan(t, L)
        B = OR.weights(Q, unrounded=True)
        seg = MR.segmented_forward(traj, Q["tau"], B, om, S, x)
        err = np.abs(seg - ex).max(axis=2)
        factor = 2.0 * math.sin(min(om_max * span / 4.0, math.pi / 2.0)) if L == 1 else 1.0 - math.cos(om_max * Q["step"] / 2.0)
        print(f"L = {L}: max |segmented - exact| / bound per (slice, coil) {(err / (factor * l1)).max():.3f} (bound factor {factor:.3e})")
        assert (err <= factor * l1 * (1 + 1e-12)).all()
    # adjointness of the restatement itself, and the adjoint as the sum over the coils
    Q = OR.plan(t, 12)
    B = OR.weights(Q)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((n, 3, 96)) + 1j * rng.standard_normal((n, 3, 96))
    wgt = 0.5 + rng.random(96)
    f = MR.segmented_forward(traj, Q["tau"], B, om, S, x)
    a = MR.segmented_adjoint(traj, Q["tau"], B, om, S, q, h, w, wgt)
    lhs, rhs = np.vdot(q * wgt, f), np.vdot(a, x)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    P = NR.plan(h, w, c["grid"][0], c["grid"][1], c["J"], traj)
    E = OR.maps(om, Q)
    assert np.allclose(MR.model_adjoint(P, B, E, S, q, wgt), (np.conj(S)[None] * MR.coil_adjoints(P, B, E, q, wgt)).sum(axis=1))
    assert np.allclose(MR.model_forward(P, B, E, S, x)[:, 2], LS.model_forward(P, B, E, S[2] * x))


def test_the_float64_fixture_figures_the_gpu_test_is_held_to():
    """offres_ref.CORRECTS with 4 coils and L = 8 least squares, in float64 on the NUFFT model; produces offres_mc_ref.CORRECTS_MC_PSNR"""
    import dcf_ref
    c = OR.CORRECTS
    traj, t, omega, gt, S, y = MR.corrects_problem()
    P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
    dcf = dcf_ref.pipe(P, 30)[0]
    om_max = float(np.abs(omega).max()) * (1.0 + 1e-6)
    B = acquisition.offres_ls_coeffs(t, MR.CORRECTS_L, om_max).astype(np.float32).astype(np.float64)
    E = OR.maps(omega, LS.plan_like(t, MR.CORRECTS_L)).astype(np.complex64).astype(np.complex128)
    got = MR.corrects_psnr(P, B, E, S, y, gt, dcf)
    print(f"float64, 4 coils, least squares L = {MR.CORRECTS_L}: {got[0]:.4f} dB; the plain non-Cartesian SENSE stage on the same y: {got[1]:.4f} dB "
          f"(recorded {MR.CORRECTS_MC_PSNR})")
    assert abs(got[0] - MR.CORRECTS_MC_PSNR[0]) <= 2e-3 and abs(got[1] - MR.CORRECTS_MC_PSNR[1]) <= 2e-3
    assert got[0] - got[1] > 30.0


def test_make_problem_ncmcb0_is_make_problem_ncb0_with_coil_maps():
    h = w = 16
    c = MC.CASES["A"]
    traj, t = MR.case_traj(c)
    om = MR.case_omega(c)
    one = synthetic.make_problem_ncmcb0(2, h, w, 1, traj, t, om, sigma_n=0.02, sens=np.ones((1, h, w)))
    ref = synthetic.make_problem_ncb0(2, h, w, traj, t, om, sigma_n=0.02)
    for k in ("y0", "ATy0", "x0", "gt", "times", "omega"):
        assert np.array_equal(one[k], ref[k]), k
    d = synthetic.make_problem_ncmcb0(1, h, w, 3, traj, t, om * 0.0, sigma_n=0.02, seed=7)     # no field: the non-Cartesian SENSE problem
    nc = synthetic.make_problem_ncmc(1, h, w, 3, traj, sigma_n=0.02, seed=7)
    assert np.array_equal(d["y0"], nc["y0"]) and np.array_equal(d["ATy0"], nc["ATy0"]) and np.array_equal(d["sens"], nc["sens"])
    assert d["y0"].shape == (1, 3, 96, 2) and d["sens"].dtype == np.complex64
    full = synthetic.make_problem_ncmcb0(1, h, w, 3, traj, t, om, sigma_n=0.0, seed=7)
    y = full["y0"][0, :, :, 0].astype(np.float64) + 1j * full["y0"][0, :, :, 1].astype(np.float64)
    ex = MR.exact_forward(traj, t, om.astype(np.float64), full["sens"].astype(np.complex128), full["gt"][:, 0].astype(np.float64))[0]
    assert np.abs(y - ex).max() <= 1e-6 * np.abs(ex).max()


# ---- the layers above the engine: simulate, task_problem, PnPEnv, the CLI (no GPU: a fake engine, as tests/test_offres_host.py's) ----------------

import test_offres_host as TH  # noqa: E402


class _FakeEngine(TH._FakeEngine):
    """tests/test_offres_host.py's fake, with the two installers of the new stage"""

    def reset_offres_mc(self, x0, y, sens, omega, w=None, cg_iters=8):
        self.calls.append(("reset_offres_mc", tuple(y.shape), tuple(sens.shape), tuple(omega.shape), w is not None, cg_iters))
        self.live_episode = 78
        return x0.real.clone(), x0.clone(), x0 * 0

    def set_kspace_offres_mc(self, y, sens, omega, w=None, episode=0, cg_iters=8):
        self.calls.append(("set_kspace_offres_mc", tuple(y.shape), tuple(sens.shape), tuple(omega.shape), w is not None, episode, cg_iters))
        self.live_episode = episode

    def offres_ls_planned(self, times, segments, omega_max):
        return self.offres is not None and len(self.offres) == 3 and self.offres[1] == segments

    def offres_plan_ls(self, times, segments, omega_max):
        self.calls.append(("offres_plan_ls", tuple(times.shape), segments))
        self.offres, self.live_episode = (np.asarray(times).copy(), segments, omega_max), 0


def test_the_new_keywords_come_last_and_default_to_what_was():
    sim = inspect.signature(acquisition.simulate).parameters
    assert list(sim)[-1] == "offres_mc" and sim["offres_mc"].default is False
    tp = inspect.signature(acquisition.task_problem).parameters
    names = list(tp)                     # the end of the list is pinned by tests/test_dcf_host.py: the keyword follows b0_interp, as b0_interp followed spokes
    assert names[names.index("b0_interp") + 1] == "b0_coils" and tp["b0_coils"].default == 0 and names[-3:] == ["interleaves", "petals", "dcf_iters"]
    from dt4image_restoration_amd import env as envmod
    ev = inspect.signature(envmod.PnPEnv.__init__).parameters
    assert list(ev)[-1] == "offres_mc" and ev["offres_mc"].default is False
    names = list(tp)
    assert names[names.index("nufft_width") + 1:names.index("nufft_grid")] == ["b0_hz", "readout_ms", "b0_segments"]      # the pinned order


def test_task_problem_hands_the_coil_maps_and_the_field_map_to_simulate_and_refuses_what_it_must(monkeypatch):
    calls = []

    def fake_simulate(eng, gt, mask, sigma_n, seed, first_slice=0, **k):
        calls.append(k)
        return {}

    monkeypatch.setattr(acquisition, "simulate", fake_simulate)
    monkeypatch.setattr(acquisition, "pipe_dcf", lambda *a, **k: "PIPE")
    gt = np.zeros((2, 64, 64), dtype=np.float32)
    e = _FakeEngine()
    acquisition.task_problem("4x_10", gt, e, seed=4, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0, b0_segments=9, b0_coils=3)
    k = calls[-1]
    assert k["offres_mc"] is True and k["segments"] == 9 and "interpolator" not in k
    assert k["sens"].shape == (3, 64, 64) and k["sens"].dtype == np.complex64
    assert np.array_equal(k["sens"], synthetic.coil_maps(3, 64, 64).astype(np.complex64))
    assert np.array_equal(k["omega"], (2 * math.pi * synthetic.field_map(64, 64, 80.0, 4)).astype(np.float32))
    assert np.array_equal(k["times"], acquisition.readout_times("spiral", 8 * 805, 805, 12e-3))
    acquisition.task_problem("4x_10", gt, e, mask_kind="rosette-nc", b0_hz=80.0, readout_ms=12.0, b0_interp="ls", b0_coils=32)
    assert calls[-1]["interpolator"] == "ls" and calls[-1]["offres_mc"] is True and calls[-1]["sens"].shape[0] == 32
    acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0)          # without b0_coils: the call of before
    assert "offres_mc" not in calls[-1] and "sens" not in calls[-1]
    for bad, what in ((dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, b0_coils=2, b0_map="estimate"), "b0_map='estimate' is not supported with b0_coils"),
                      (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, b0_coils=33), "b0_coils must be 1..32"),
                      (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, b0_coils=-1), "b0_coils must be 1..32"),
                      (dict(mask_kind="spiral-nc", b0_coils=2), "b0_coils needs b0_hz"),
                      (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, b0_coils=2, coils=2), "does not go with coils"),
                      (dict(mask_kind="radial", b0_hz=80.0, readout_ms=5.0, b0_coils=2), "non-Cartesian"),
                      (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, coils=2), "single-coil")):      # the pinned refusal, still raised
        with pytest.raises(ValueError, match=what):
            acquisition.task_problem("4x_10", gt, e, **bad)


def test_simulate_keeps_its_refusal_unless_offres_mc_is_set(monkeypatch):
    import torch
    seen = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(acquisition, "_engine", lambda eng, *a: eng)
    monkeypatch.setattr(acquisition, "_simulate_nc", lambda eng, g, traj, dcf, sigma_n, seed, width, grid, **k: seen.append(k) or {})
    e = _FakeEngine()
    gt = np.zeros((2, 16, 16), dtype=np.float32)
    traj, t = np.zeros((8, 2)), np.arange(8) * 1e-4
    om, sens = np.zeros((16, 16), dtype=np.float32), np.ones((2, 16, 16), dtype=np.complex64)
    with pytest.raises(ValueError, match="single-coil"):
        acquisition.simulate(e, gt, None, 0.0, 1, traj=traj, omega=om, times=t, sens=sens)
    with pytest.raises(ValueError, match="single-coil"):
        acquisition.simulate(e, gt, None, 0.0, 1, traj=traj, omega=om, times=t, sens=sens, offres_mc=False)
    acquisition.simulate(e, gt, None, 0.0, 1, traj=traj, omega=om, times=t, sens=sens, offres_mc=True)
    assert seen[-1]["sens"] is sens and seen[-1]["omega"] is om
    acquisition.simulate(e, gt, None, 0.0, 1, traj=traj, omega=om, times=t, offres_mc=True)               # no coils: the single-coil acquisition
    assert seen[-1]["sens"] is None


def test_the_environment_installs_and_rebinds_the_new_stage_only_when_asked():
    import torch
    from dt4image_restoration_amd import env as envmod
    n, h, w, m, C = 2, 16, 16, 48, 3
    fake = _FakeEngine()
    env = envmod.PnPEnv.__new__(envmod.PnPEnv)                                       # no offres_mc attribute at all: the default is read
    env.nc_normal, env.cg_iters, env.nufft_width, env.nufft_grid = "nufft", 5, 6, None
    env._engine_for = lambda *a: fake
    times = np.tile(np.arange(24) * 1e-4, 2)
    omega = torch.full((h, w), 2 * math.pi * 100.0)
    sens = torch.ones(C, h, w, dtype=torch.complex64)
    data = {"x0": torch.zeros(n, 1, h, w, 2), "y0": torch.zeros(n, C, m, 2), "gt": torch.zeros(n, 1, h, w), "traj": torch.zeros(m, 2, dtype=torch.float64),
            "dcf": torch.ones(m), "omega": omega, "times": torch.from_numpy(times), "segments": 4, "sens": sens}
    x0 = torch.zeros(n, 1, h, w, dtype=torch.complex64)
    with pytest.raises(ValueError, match="single-coil"):                             # the pinned refusal, still raised
        env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    env.offres_mc = False
    with pytest.raises(ValueError, match="single-coil"):
        env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    assert not [c for c in fake.calls if c[0].startswith("reset")]
    env.offres_mc = True
    del fake.calls[:]
    fake.nufft = None
    st = env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    assert [c[0] for c in fake.calls] == ["nufft_plan", "offres_plan", "reset_offres_mc"]
    assert fake.calls[2] == ("reset_offres_mc", (n, C, m), (C, h, w), (h, w), True, 5)
    assert st["_episode"] == 78 and st["segments"] == 4 and torch.equal(st["sens"], sens) and torch.equal(st["omega"], omega)
    del fake.calls[:]
    env._bind_episode(fake, st)                                                      # the live episode: nothing to do
    assert fake.calls == []
    fake.live_episode = 5                                                            # another episode ran in between
    env._bind_episode(fake, st)
    assert fake.calls == [("set_kspace_offres_mc", (n, C, m), (C, h, w), (h, w), True, 78, 5)]
    del fake.calls[:]
    fake.offres = None                                                               # ... or the plan was replaced
    env._bind_episode(fake, st)
    assert [c[0] for c in fake.calls] == ["offres_plan", "set_kspace_offres_mc"]
    del fake.calls[:]
    st = env._reset_nc(dict(data, b0_interp="ls"), x0, n, h, w, torch.device("cpu"))  # the least-squares plan
    assert [c[0] for c in fake.calls] == ["nufft_plan", "offres_plan_ls", "reset_offres_mc"] and st["b0_interp"] == "ls"      # (a new traj tensor)
    single = {k: v for k, v in data.items() if k != "sens"}                          # without coil maps the env installs the single-coil stage
    single["y0"] = torch.zeros(n, 1, m, 2)
    del fake.calls[:]
    env._reset_nc(single, x0, n, h, w, torch.device("cpu"))
    assert fake.calls[-1][0] == "reset_offres"
    env.nc_normal = "toeplitz"
    with pytest.raises(ValueError, match="Toeplitz"):
        env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    assert "offres_mc" in inspect.getsource(envmod.PnPEnv.fork)                      # a fork is an env of the same kind


def test_the_engine_still_refuses_a_field_map_with_coil_maps_in_reset_and_set_kspace():
    import torch
    e = engine.PnPEngine.__new__(engine.PnPEngine)                                   # the refusal comes before the handle is read
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="single-coil"):
        e.reset(z, z, sens=z, omega=z)
    with pytest.raises(ValueError, match="single-coil"):
        e.set_kspace(z, sens=z, omega=z)


def test_cli_b0_coils_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    b0 = ["--traj", "spiral", "--b0", "50", "--readout-ms", "5"]
    for extra, what in ((["--traj", "spiral", "--b0-coils", "4"], "--b0-coils needs --b0"), (["--b0-coils", "4"], "--b0-coils needs --b0"),
                        (b0 + ["--b0-coils", "33"], "--b0-coils must be 1..32"), (b0 + ["--b0-coils", "-2"], "--b0-coils must be 1..32"),
                        (b0 + ["--b0-coils", "4", "--nc-coils", "2"], "--b0-coils with --nc-coils"),
                        (b0 + ["--b0-coils", "4", "--coils", "2"], "--b0-coils with --coils"),
                        (b0 + ["--b0-coils", "4", "--nc-normal", "toeplitz"], "--b0-coils with --nc-normal toeplitz"),
                        (b0 + ["--b0-coils", "4", "--b0-map", "estimate"], "--b0-coils with --b0-map estimate"),
                        (["--traj", "radial", "--b0", "50", "--readout-ms", "5", "--nc-coils", "2"], "single-coil")):      # the pinned refusal
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])

    class A:
        traj, spokes, nc_weights, nufft_width, nufft_grid, nc_coils, interleaves, petals, dcf_iters = "spiral", None, "dcf", 6, None, 0, 4, None, 30
        b0, readout_ms, b0_segments = 50.0, 5.0, 8
    assert "b0_coils" not in cli._nc_kwargs(A)                                       # a namespace from before the option: the call of before
    A.b0_coils = 0
    assert "b0_coils" not in cli._nc_kwargs(A)
    A.b0_coils = 4
    assert cli._nc_kwargs(A)["b0_coils"] == 4 and cli._nc_kwargs(A)["coils"] == 0
