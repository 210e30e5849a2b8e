"""CPU-only checks of the Toeplitz form of the off-resonance normal operator: the entry points of include/pnpadmm_offres_tz.h are declared,
exported, bound from `_lib.SIGNATURES_OFFRES_TZ` and classified in tests/offres_tz_cases.py, while the eight older headers stay the sets they
were; the header compiles as C99 with -pedantic -Werror and links from C; every argument error that needs no handle comes back from ctypes
without a GPU and leaves the outputs untouched; the pure-host pair plan (csrc/offres_tz_plan.hip) is compiled into a stand-alone program with
its own main (tests/asan_offres_tz_host.cpp), plain and with -fsanitize=address,undefined, refuses every invalid argument and gives the lists
of the restatement; the float64 identity behind the feature - the FFT form of tests/offres_tz_ref.py equals the dense A^H W A to 1e-12 - and
the band structure under a linear plan; the Python and CLI refusals, with the old refusals untouched.

The rejections that read the handle - no plan, no spectra, a side above 512, P above the limit - need a handle, and pnp_create needs a
device: tests/test_gpu_offres_tz.py makes them."""
import inspect
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_cases as HC  # noqa: E402
import ncsense_cases as NC  # noqa: E402
import offres_cases as OC  # noqa: E402
import offres_mc_cases as MC  # noqa: E402
import offres_mc_ref as MR  # noqa: E402
import offres_ref as OR  # noqa: E402
import offres_tz_cases as ZC  # noqa: E402
import offres_tz_ref as Z  # noqa: E402
import toeplitz_cases as TC  # noqa: E402
import toeplitz_ref as T  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ["pnp_offres_tz_apply", "pnp_offres_tz_apply_mc", "pnp_offres_tz_live", "pnp_offres_tz_plan", "pnp_offres_tz_planned", "pnp_offres_tz_spectra",
         "pnp_offres_tz_spectrum", "pnp_reset_offres_mc_tz", "pnp_reset_offres_tz", "pnp_set_kspace_offres_mc_tz", "pnp_set_kspace_offres_tz"]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(ZC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(ZC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_OFFRES_TZ) == NAMES
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in ZC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_OFFRES_TZ[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{ZC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_OFFRES_TZ[name][1]       # bound by _lib.load()'s loop
        assert cls in (HC.INTRUDER, HC.REPLACES, HC.STATELESS)
    assert {n for n, (c, _) in ZC.ENTRY_POINTS.items() if c == HC.STATELESS} == {"pnp_offres_tz_planned", "pnp_offres_tz_live", "pnp_offres_tz_spectra"}
    assert {n for n, (c, _) in ZC.ENTRY_POINTS.items() if c == HC.REPLACES} == {n for n in ZC.ENTRY_POINTS if n.endswith("_tz")} | {"pnp_offres_tz_plan"}
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_offres_tz.py")).read()
    for name, (cls, _) in ZC.ENTRY_POINTS.items():
        if cls != HC.STATELESS:
            assert f"def {ZC.COVERED_BY[name]}(" in gpu, name
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    for gone in ZC.ENTRY_POINTS:                                                    # deleting any row of the table is noticed
        assert ZC.missing(names, {k: v for k, v in ZC.ENTRY_POINTS.items() if k != gone}) == [gone]
    assert ZC.missing(names) == []
    for word in ("THE MODEL", "EXPRESSION ORDER", "TWO FORMS", "SLICE BLOCKS", "SIZES AND LIMITS", "THE PAIR ORDER", "PNP_OFFRES_TZ_NAIVE",
                 "PNP_OFFRES_TZ_SLICE_BLOCK", "THE BITS DO NOT DEPEND ON CB", "PNP_ERR_STATE", "leaving the outputs untouched"):
        assert word in text, word
    assert _lib.PNP_OFFRES_TZ_MAX_PAIRS == 136 == 16 * 17 // 2 and _lib.PNP_OFFRES_TZ_PLANES == 512
    assert re.search(r"#define PNP_OFFRES_TZ_MAX_PAIRS 136\b", text) and re.search(r"#define PNP_OFFRES_TZ_PLANES 512\b", text)
    if shutil.which("nm"):                                                          # the exports of the built library, by its dynamic symbol table
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r"\bT %s$" % name, syms, flags=re.M), name


def test_the_eight_older_headers_are_the_sets_they_were():
    new = set(ZC.ENTRY_POINTS)
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) and len(old) == 57
    ns = HC.header_functions(_header(NC.HEADER))
    assert ns == sorted(_lib.SIGNATURES_NCSENSE) == sorted(NC.ENTRY_POINTS) and len(ns) == 8
    tz = HC.header_functions(_header(TC.HEADER))
    assert tz == sorted(_lib.SIGNATURES_TOEPLITZ) == sorted(TC.ENTRY_POINTS) and len(tz) == 10
    dcf = HC.header_functions(_header("pnpadmm_dcf.h"))
    assert dcf == sorted(_lib.SIGNATURES_DCF) and len(dcf) == 2
    orr = HC.header_functions(_header(OC.HEADER))
    assert orr == sorted(_lib.SIGNATURES_OFFRES) == sorted(OC.ENTRY_POINTS) and len(orr) == 11
    ls = HC.header_functions(_header("pnpadmm_offres_ls.h"))
    assert ls == sorted(_lib.SIGNATURES_OFFRES_LS) and len(ls) == 3
    mc = HC.header_functions(_header(MC.HEADER))
    assert mc == sorted(_lib.SIGNATURES_OFFRES_MC) == sorted(MC.ENTRY_POINTS) and len(mc) == 8
    fm = HC.header_functions(_header("pnpadmm_fieldmap.h"))
    assert fm == sorted(_lib.SIGNATURES_FIELDMAP) and len(fm) == 2
    for older in (old, ns, tz, dcf, orr, ls, mc, fm):
        assert not new & set(older)
    for name in ("pnpadmm.h", NC.HEADER, TC.HEADER, "pnpadmm_dcf.h"):              # the four oldest headers never speak of the off-resonance stages
        assert "offres" not in _header(name).lower(), name
    assert "OUT OF SCOPE" in _header(OC.HEADER) and "Toeplitz" in _header(OC.HEADER)
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")) == sorted(
        ["pnpadmm.h", NC.HEADER, TC.HEADER, "pnpadmm_dcf.h", OC.HEADER, "pnpadmm_offres_ls.h", MC.HEADER, "pnpadmm_fieldmap.h", ZC.HEADER])


def test_build_files_the_units_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\boffres_tz_kernels\.o\b.*\boffres_tz_plan\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_offres_tz_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*offres_tz_plan\.h.*pnpadmm_offres_tz\.h", mk, flags=re.M)) == 2      # both dependency lists
    unit = open(os.path.join(CSRC, "offres_tz_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()
    for kernel in ("offres_tz_spectra_kernel", "offres_tz_mix_kernel"):
        assert f"void {kernel}(" in unit
    assert "void tz_cols_half_kernel(" in open(os.path.join(CSRC, "fft_kernels.hip")).read()
    tune = open(os.path.join(CSRC, "conv_kernels.hip")).read()
    m = re.search(r"^Tuning tuning_from_env\(\) \{$.*?^\}$", tune, re.S | re.M)
    assert m and 'getenv("PNP_OFFRES_TZ_NAIVE")' in m.group(0) and 'getenv("PNP_OFFRES_TZ_SLICE_BLOCK")' in m.group(0)
    internal = open(os.path.join(CSRC, "pnp_internal.h")).read()
    assert "kOffresTzPlanes = 512" in internal
    capi = open(os.path.join(CSRC, "pnp_capi.hip")).read()
    assert "enum StageForm { FORM_GRID, FORM_TZ, FORM_OTZ };" in capi                # a form of its own in LiveStage, beside the existing one
    assert "return e && e->stage.form == FORM_TZ ? 1 : 0; }" in capi                 # pnp_toeplitz_live reads the old form alone
    assert "return e && e->stage.form == FORM_OTZ ? 1 : 0; }" in capi                # ... and pnp_offres_tz_live this header's
    P = engine.PnPEngine
    for name, params in (("offres_tz_plan", ["self", "weights"]), ("offres_tz_spectrum", ["self"]), ("offres_tz_apply", ["self", "img", "maps"]),
                         ("offres_tz_apply_mc", ["self", "img", "maps", "sens"]), ("reset_offres_tz", ["self", "x0", "y", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres_tz", ["self", "y", "omega", "w", "episode", "cg_iters"]),
                         ("reset_offres_mc_tz", ["self", "x0", "y", "sens", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres_mc_tz", ["self", "y", "sens", "omega", "w", "episode", "cg_iters"]),
                         # the siblings keep their lists
                         ("reset_offres", ["self", "x0", "y", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres", ["self", "y", "omega", "w", "episode", "cg_iters"]),
                         ("reset_offres_mc", ["self", "x0", "y", "sens", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres_mc", ["self", "y", "sens", "omega", "w", "episode", "cg_iters"])):
        assert list(inspect.signature(getattr(P, name)).parameters) == params, name
    assert inspect.signature(P.offres_tz_plan).parameters["weights"].default is None
    for prop in ("offres_tz_planned", "offres_tz_live", "offres_tz_spectra"):
        assert isinstance(getattr(P, prop), property), prop


def test_the_new_header_is_plain_c99_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_offres_tz.h"\n'
        "int main(void) {\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};\n"
        "    if (pnp_offres_tz_planned(0) != 0 || pnp_offres_tz_live(0) != 0 || pnp_offres_tz_spectra(0) != 0) return 1;\n"
        "    if (pnp_offres_tz_plan(0, a, 1, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 2;\n"
        "    if (pnp_offres_tz_apply(0, a, b, 1, 0, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"batch\")) return 3;\n"
        "    if (pnp_offres_tz_apply_mc(0, a, b, 1, b, 1, 0, 1, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 4;\n"
        "    if (pnp_set_kspace_offres_tz(0, a, b, 1, 65, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"cg_iters\")) return 5;\n"
        "    if (pnp_reset_offres_mc_tz(0, a, a, b, 4, 0, b, 1, 4, y, y, y, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"sens_n\")) return 6;\n"
        "    if (pnp_offres_tz_spectrum(0, y, 0) != PNP_ERR_INVALID) return 7;\n"
        "    if (y[0] != 1.f || y[1] != 2.f || y[2] != 3.f || y[3] != 4.f || PNP_OFFRES_TZ_MAX_PAIRS != 136) return 8;\n"
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
    app, amc, ins, rst, imc, rmc = (lib.pnp_offres_tz_apply, lib.pnp_offres_tz_apply_mc, lib.pnp_set_kspace_offres_tz, lib.pnp_reset_offres_tz,
                                    lib.pnp_set_kspace_offres_mc_tz, lib.pnp_reset_offres_mc_tz)
    cases = [
        (lambda: lib.pnp_offres_tz_plan(None, pa, 1, None), b"flags must be 0"),
        (lambda: lib.pnp_offres_tz_plan(None, pa, -1, None), b"flags"),
        (lambda: lib.pnp_offres_tz_plan(None, pa, 0, None), b"null handle"),
        (lambda: lib.pnp_offres_tz_plan(None, None, 0, None), b"null handle"),
        (lambda: lib.pnp_offres_tz_spectrum(None, None, None), b"null out"),
        (lambda: lib.pnp_offres_tz_spectrum(None, po, None), b"null handle"),
        (lambda: app(None, pa, pb, 0, 1, po, None), b"map_n must be 1 or n (got 0)"),
        (lambda: app(None, pa, pb, 1, 0, po, None), b"batch must be 1..n (got 0)"),
        (lambda: app(None, pa, pb, 1, -3, po, None), b"batch"),
        (lambda: app(None, None, pb, 1, 1, po, None), b"null img"),
        (lambda: app(None, pa, None, 1, 1, po, None), b"null maps"),
        (lambda: app(None, pa, pb, 1, 1, None, None), b"null out"),
        (lambda: app(None, po, pb, 1, 1, po, None), b"alias"),
        (lambda: app(None, pa, po, 1, 1, po, None), b"alias"),
        (lambda: app(None, pa, pb, 1, 1, po, None), b"null handle"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 0, 1, po, None), b"coils must be 1..32 (got 0)"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 33, 1, po, None), b"coils must be 1..32 (got 33)"),
        (lambda: amc(None, pa, pb, 1, ps, 0, 2, 1, po, None), b"sens_n must be 1 or n (got 0)"),
        (lambda: amc(None, pa, pb, 0, ps, 1, 2, 1, po, None), b"map_n must be 1 or n (got 0)"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 2, 0, po, None), b"batch must be 1..n (got 0)"),
        (lambda: amc(None, None, pb, 1, ps, 1, 2, 1, po, None), b"null img"),
        (lambda: amc(None, pa, None, 1, ps, 1, 2, 1, po, None), b"null maps"),
        (lambda: amc(None, pa, pb, 1, None, 1, 2, 1, po, None), b"null sens"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 2, 1, None, None), b"null out"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 2, 1, pa, None), b"alias"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 2, 1, pb, None), b"alias"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 2, 1, ps, None), b"alias"),
        (lambda: amc(None, pa, pb, 1, ps, 1, 32, 1, po, None), b"null handle"),
        (lambda: ins(None, pa, pb, 0, 8, None), b"map_n must be 1 or n (got 0)"),
        (lambda: ins(None, pa, pb, 1, 0, None), b"cg_iters must be 1..64 (got 0)"),
        (lambda: ins(None, pa, pb, 1, 65, None), b"cg_iters"),
        (lambda: ins(None, None, pb, 1, 8, None), b"null y"),
        (lambda: ins(None, pa, None, 1, 8, None), b"null omega"),
        (lambda: ins(None, pa, pb, 1, 8, None), b"null handle"),
        (lambda: rst(None, None, pa, pb, 1, 8, po, po2, po3, None), b"null x0"),
        (lambda: rst(None, pa, None, pb, 1, 8, po, po2, po3, None), b"null y"),
        (lambda: rst(None, pa, pa, None, 1, 8, po, po2, po3, None), b"null omega"),
        (lambda: rst(None, pa, pa, pb, 1, 8, None, po2, po3, None), b"null x, z or u"),
        (lambda: rst(None, pa, pa, pb, 1, 8, po, po2, None, None), b"null x, z or u"),
        (lambda: rst(None, pa, pa, pb, 1, 8, po, po2, po3, None), b"null handle"),
        (lambda: imc(None, pa, ps, 0, 1, pb, 1, 8, None), b"coils"),
        (lambda: imc(None, pa, ps, 2, 0, pb, 1, 8, None), b"sens_n"),
        (lambda: imc(None, pa, ps, 2, 1, pb, 0, 8, None), b"map_n"),
        (lambda: imc(None, pa, ps, 2, 1, pb, 1, 0, None), b"cg_iters must be 1..64 (got 0)"),
        (lambda: imc(None, None, ps, 2, 1, pb, 1, 8, None), b"null y"),
        (lambda: imc(None, pa, None, 2, 1, pb, 1, 8, None), b"null sens"),
        (lambda: imc(None, pa, ps, 2, 1, None, 1, 8, None), b"null omega"),
        (lambda: imc(None, pa, ps, 2, 1, pb, 1, 8, None), b"null handle"),
        (lambda: rmc(None, None, pa, ps, 2, 1, pb, 1, 8, po, po2, po3, None), b"null x0"),
        (lambda: rmc(None, pa, pa, None, 2, 1, pb, 1, 8, po, po2, po3, None), b"null sens"),
        (lambda: rmc(None, pa, pa, ps, 2, 1, pb, 1, 8, po, None, po3, None), b"null x, z or u"),
        (lambda: rmc(None, pa, pa, ps, 2, 1, pb, 1, 8, po, po2, po3, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_offres_tz_planned(None) == 0 and lib.pnp_offres_tz_live(None) == 0 and lib.pnp_offres_tz_spectra(None) == 0
    for o in (out, out2, out3):
        assert (o == 7.0).all()
    for v, off in ((a, 0.0), (b, 100.0), (s, 200.0)):
        assert np.array_equal(v, np.arange(64, dtype=np.float32) + off)


# ---- the pure-host pair plan: the stand-alone program, plain and sanitized -------------------------------------------------------------------

def _build(workdir, sanitize):
    exe = os.path.join(workdir, "asan_offres_tz_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-std=c++17", "--offload-arch=gfx950"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "tests", "asan_offres_tz_host.cpp"), os.path.join(CSRC, "offres_tz_plan.hip"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def plan_tools(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("offres_tz_plan_host"))
    return d, _build(d, False), _build(d, True)


def test_pair_plan_builder_refuses_every_invalid_argument(plan_tools):
    for exe in plan_tools[1:]:
        r = subprocess.run([exe, "--invalid"], capture_output=True, text=True)
        assert r.returncode == 0 and "asan_offres_tz_host: invalid ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _times_case(k, m):
    if k == 0:                                                                     # four readouts of the same clock: a segment's samples are not contiguous
        return acquisition.readout_times("spiral", m, m // 4, 8e-3, te=1e-3)
    rng = np.random.default_rng(11)
    t = rng.random(m) * 5e-3 - 1e-3
    t[3], t[5] = t.max(), t.min()
    return t


@pytest.mark.parametrize("k", range(2))
def test_pair_plan_builder_gives_the_header_order_and_complete_ascending_lists(plan_tools, k):
    d, *exes = plan_tools
    m = 384
    t = _times_case(k, m)
    for kind, name, Ls in ((1, "linear", (1, 2, 3, 9, 32)), (2, "ls", (1, 4, 11, 16))):
        for L in Ls:
            seg = OR.plan(t, L)["seg"].astype(np.int32)
            path = os.path.join(d, f"in{k}.bin")
            with open(path, "wb") as f:
                f.write(struct.pack("<q", m) + seg.tobytes())
            want_pairs = Z.pairs(name, L)
            assert len(want_pairs) == _lib.offres_tz_pairs(name, L) == (2 * L - 1 if kind == 1 else L * (L + 1) // 2)
            for exe in exes:
                outp = os.path.join(d, f"out{k}.bin")
                r = subprocess.run([exe, "--dump", path, str(kind), str(L), outp], capture_output=True, text=True)
                assert r.returncode == 0 and "dump ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
                raw = np.frombuffer(open(outp, "rb").read(), np.int32)
                pairs, block, blocks, n_off = (int(v) for v in raw[:4])
                left, right = raw[4:4 + pairs], raw[4 + pairs:4 + 2 * pairs]
                off = raw[4 + 2 * pairs:4 + 2 * pairs + n_off]
                idx = raw[4 + 2 * pairs + n_off:]
                assert list(zip(left.tolist(), right.tolist())) == want_pairs and blocks == -(-pairs // block)
                if kind == 2:
                    assert n_off == 0 and idx.size == 0 and block == 4
                    continue
                assert block == 2 and n_off == blocks + 1 == L + 1 and off[0] == 0 and off[-1] == idx.size
                for b in range(blocks):                                             # block b: the pairs (b, b) and (b, b + 1)
                    want = [s for s in range(m) if seg[s] == b or seg[s] == b - 1]
                    assert idx[off[b]:off[b + 1]].tolist() == want, (k, L, b)
                    # ... which is every sample that carries weight in one of its pairs
                    B = OR.weights(OR.plan(t, L))
                    carries = np.zeros(m, bool)
                    for p in range(block * b, min(block * b + block, pairs)):
                        carries |= (B[left[p]] * B[right[p]]) != 0.0
                    assert set(np.nonzero(carries)[0].tolist()) <= set(want)
                assert idx.size <= 2 * m


# ---- the identity: the FFT form equals the dense operator --------------------------------------------------------------------------------------

def _host_case(name, plan=None, L=None):
    c = dict(ZC.CASES[name])
    if plan is not None:
        c.update(plan=plan, L=L)
    traj, t = MR.case_traj(c)
    om = MR.case_omega(c).astype(np.float64)
    x, _, wgt = MR.case_data(c, traj.shape[0], seed=ord(name))
    if c["plan"] == "ls":
        band = float(np.abs(om).max()) * (1.0 + 1e-6)
        B = acquisition.offres_ls_coeffs(t, c["L"], band).astype(np.float32).astype(np.float64) if c["L"] > 1 else np.ones((1, t.size))
        tau = OR.plan(t, c["L"])["tau"]
    else:
        Q = OR.plan(t, c["L"])
        B, tau = OR.weights(Q), Q["tau"]
    E = OR.maps(om, dict(tau=tau))
    return c, traj, B, E, x, wgt


@pytest.mark.parametrize("name,plan,L", [(n, None, None) for n in ZC.HOST_CASES] + [("A", "ls", 4), ("B", "ls", 8), ("C", "linear", 3)])
def test_the_fft_form_equals_the_dense_operator_and_the_band_holds(name, plan, L):
    c, traj, B, E, x, wgt = _host_case(name, plan, L)
    h, w, L = c["h"], c["w"], c["L"]
    K = Z.spectra(traj, h, w, B, c["plan"], wgt)
    assert K.shape == (len(Z.pairs(c["plan"], L)), 2 * h, 2 * w)
    Kf = Z.full_matrix(K, c["plan"], L)
    assert np.array_equal(Kf, Kf.transpose(1, 0, 2, 3))
    got = Z.apply(Kf, E, x)
    want = Z.dense_normal(traj, B, E, x, wgt)
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    f32 = float(np.linalg.norm(Z.apply_f32(Kf, E, x) - got) / np.linalg.norm(got))
    blocks = Z.nonzero_blocks(B, wgt)
    print(f"case {name} ({h} x {w}, L = {L} {c['plan']}, P = {K.shape[0]}): FFT form against the dense A^H W A: rel l2 {rel:.2e}; the float32 restatement "
          f"against the FFT form: {f32:.2e}; non-zero (l, l') blocks: {len(blocks)}")
    assert rel <= 1e-12
    assert f32 <= 2e-6
    if c["plan"] == "linear":
        assert len(blocks) == max(3 * L - 2, 1) and all(abs(l - r) <= 1 for l, r in blocks)
        assert {(min(l, r), max(l, r)) for l, r in blocks} == set(Z.pairs("linear", L))
    else:
        assert len(blocks) == L * L
    # L = 1 with unit coefficients: the plain Toeplitz spectrum, and every spectrum the transform of its directly summed lags
    if L == 1:
        assert np.array_equal(K[0], T.spectrum(traj, h, w, wgt))
    u = Z.pair_weights(B, wgt)
    l, r = Z.pairs(c["plan"], L)[-1]
    lags = T.spectrum_by_lags(traj, h, w, u[l, r])
    assert np.abs(lags.real - K[-1]).max() <= 1e-9 * max(np.abs(K[-1]).max(), 1.0) and np.abs(lags.imag).max() <= 1e-9 * max(np.abs(K[-1]).max(), 1.0)


def test_the_multi_coil_form_is_the_sum_over_the_coils():
    c, traj, B, E, x, wgt = _host_case("E")
    S = MR.case_sens(c)
    Kf = Z.full_matrix(Z.spectra(traj, c["h"], c["w"], B, c["plan"], wgt), c["plan"], c["L"])
    got = Z.apply_mc(Kf, E, S, x)
    want = Z.dense_normal_mc(traj, B, E, S, x, wgt)
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"case E with {c['C']} coils: FFT form against the dense operator: rel l2 {rel:.2e}")
    assert rel <= 1e-12


def test_the_cases_are_the_shapes_the_issue_names():
    c = ZC.CASES
    assert sorted(c) == list("ABCDEFG")
    assert [(c[k]["n"], c[k]["h"], c[k]["w"], c[k]["L"], c[k]["plan"]) for k in "ABCDEFG"] == [
        (2, 16, 16, 1, "linear"), (3, 16, 32, 3, "linear"), (2, 32, 32, 9, "linear"), (1, 80, 64, 8, "ls"), (2, 32, 32, 11, "ls"),
        (1, 128, 128, 2, "linear"), (1, 256, 256, 2, "linear")]
    assert c["B"]["map_n"] == "n" and c["B"]["wts"] and c["D"]["wts"] and not c["A"]["wts"] and c["C"]["map_n"] == 1
    assert c["E"]["C"] == 3 and c["E"]["sens_n"] == "n" and ZC.COIL_BLOCKS == (1, 2) and ZC.SLICE_BLOCKS == (1,)
    assert (c["A"]["kind"], c["B"]["kind"], c["D"]["kind"]) == ("radial", "spiral", "rosette")
    assert 100 <= MR.case_traj(c["F"])[0].shape[0] <= 999 and 100 <= MR.case_traj(c["G"])[0].shape[0] <= 999       # a few hundred samples
    assert _lib.toeplitz_size_error("f", 80, 64) is None and (2 * 80) % 5 == 0                                    # D: a mixed-radix padded side


# ---- the Python layers and the CLI: the new option, and the old refusals word for word ------------------------------------------------------------

import test_offres_mc_host as TMH  # noqa: E402


class _FakeEngine(TMH._FakeEngine):
    """tests/test_offres_mc_host.py's fake, with the four installers of the Toeplitz form"""

    def reset_offres_tz(self, x0, y, omega, w=None, cg_iters=8):
        self.calls.append(("reset_offres_tz", tuple(y.shape), tuple(omega.shape), w is not None, cg_iters))
        self.live_episode = 79
        return x0.real.clone(), x0.clone(), x0 * 0

    def set_kspace_offres_tz(self, y, omega, w=None, episode=0, cg_iters=8):
        self.calls.append(("set_kspace_offres_tz", tuple(y.shape), tuple(omega.shape), w is not None, episode, cg_iters))
        self.live_episode = episode

    def reset_offres_mc_tz(self, x0, y, sens, omega, w=None, cg_iters=8):
        self.calls.append(("reset_offres_mc_tz", tuple(y.shape), tuple(sens.shape), tuple(omega.shape), w is not None, cg_iters))
        self.live_episode = 80
        return x0.real.clone(), x0.clone(), x0 * 0

    def set_kspace_offres_mc_tz(self, y, sens, omega, w=None, episode=0, cg_iters=8):
        self.calls.append(("set_kspace_offres_mc_tz", tuple(y.shape), tuple(sens.shape), tuple(omega.shape), w is not None, episode, cg_iters))
        self.live_episode = episode


def test_the_environment_option_selects_the_toeplitz_installers_and_defaults_to_what_was():
    import math
    import torch
    from dt4image_restoration_amd import env as envmod
    ev = inspect.signature(envmod.PnPEnv.__init__).parameters
    assert ev["offres_normal"].default == "nufft" and ev["nc_normal"].default == "nufft" and list(ev)[-1] == "offres_mc"
    with pytest.raises(ValueError, match="offres_normal"):
        envmod.PnPEnv(3, None, "cuda", offres_normal="exact")
    assert "offres_normal" in inspect.getsource(envmod.PnPEnv.fork)                  # a fork is an env of the same kind
    n, h, w, m, C = 2, 16, 16, 48, 3
    times = np.tile(np.arange(24) * 1e-4, 2)
    omega = torch.full((h, w), 2 * math.pi * 100.0)
    sens = torch.ones(C, h, w, dtype=torch.complex64)
    x0 = torch.zeros(n, 1, h, w, dtype=torch.complex64)
    base = {"x0": torch.zeros(n, 1, h, w, 2), "gt": torch.zeros(n, 1, h, w), "traj": torch.zeros(m, 2, dtype=torch.float64), "dcf": torch.ones(m),
            "omega": omega, "times": torch.from_numpy(times), "segments": 4}
    for option, single, multi in (("nufft", "offres", "offres_mc"), ("toeplitz", "offres_tz", "offres_mc_tz")):
        fake = _FakeEngine()
        env = envmod.PnPEnv.__new__(envmod.PnPEnv)
        env.nc_normal, env.cg_iters, env.nufft_width, env.nufft_grid, env.offres_mc, env.offres_normal = "nufft", 5, 6, None, True, option
        env._engine_for = lambda *a, fake=fake: fake
        st = env._reset_nc(dict(base, y0=torch.zeros(n, 1, m, 2)), x0, n, h, w, torch.device("cpu"))
        assert [c[0] for c in fake.calls] == ["nufft_plan", "offres_plan", f"reset_{single}"]
        fake.live_episode = 5                                                       # another episode ran in between
        del fake.calls[:]
        env._bind_episode(fake, st)
        assert [c[0] for c in fake.calls] == [f"set_kspace_{single}"] and fake.calls[0][-2:] == (st["_episode"], 5)
        del fake.calls[:]
        st = env._reset_nc(dict(base, y0=torch.zeros(n, C, m, 2), sens=sens), x0, n, h, w, torch.device("cpu"))
        assert fake.calls[-1][0] == f"reset_{multi}"
        fake.live_episode = 5
        del fake.calls[:]
        env._bind_episode(fake, st)
        assert [c[0] for c in fake.calls] == [f"set_kspace_{multi}"]
        env.nc_normal = "toeplitz"                                                  # the old refusal, word for word, whatever the new option says
        with pytest.raises(ValueError, match=re.escape("an off-resonance episode has no Toeplitz normal operator (nc_normal='toeplitz' with data['omega'])")):
            env._reset_nc(dict(base, y0=torch.zeros(n, 1, m, 2)), x0, n, h, w, torch.device("cpu"))


def test_cli_b0_normal_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    b0 = ["--traj", "spiral", "--b0", "50", "--readout-ms", "5"]
    tz = ["--b0-normal", "toeplitz"]
    for extra, mode, what in (
            (tz, "fixed", "--b0-normal toeplitz needs --b0"), (["--traj", "spiral"] + tz, "fixed", "--b0-normal toeplitz needs --b0"),
            (b0 + tz, "acquire", "acquire runs no CG: drop --b0-normal toeplitz"),
            (b0 + tz + ["--size", "640"], "fixed", re.escape("pnp_offres_tz_plan: the Toeplitz operator transforms a 2h x 2w grid, so it takes h, w up to 512 (got 640x640)")),
            (b0 + tz + ["--b0-interp", "ls", "--b0-segments", "17"], "fixed",
             re.escape("pnp_offres_tz_plan: 17 segments under a least-squares plan need 153 spectra, more than the limit of 136")),
            (b0 + tz + ["--b0-coils", "4", "--b0-interp", "ls", "--b0-segments", "32"], "fixed", "528 spectra, more than the limit of 136"),
            # the old refusals, word for word, with and without the new option
            (b0 + ["--nc-normal", "toeplitz"], "fixed", "--b0 with --nc-normal toeplitz: the off-resonance stage has no Toeplitz form"),
            (b0 + tz + ["--nc-normal", "toeplitz"], "fixed", "--b0 with --nc-normal toeplitz: the off-resonance stage has no Toeplitz form"),
            (b0 + ["--b0-coils", "4", "--nc-normal", "toeplitz"], "fixed", "--b0-coils with --nc-normal toeplitz: the off-resonance stage has no Toeplitz form"),
            (b0, "acquire", "--b0 is for eval / flex / mcts / fixed")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ([mode, "--max_iter", "2"] if mode == "fixed" else [mode, "--out", "unused"]))
    assert _lib.offres_tz_pairs_error("f", "linear", 32) is None and _lib.offres_tz_pairs_error("f", "ls", 16) is None
    assert "153 spectra" in _lib.offres_tz_pairs_error("f", "ls", 17)
    assert _lib.toeplitz_size_error("f", 512, 512) is None
    src = open(os.path.join(ROOT, "dt4image_restoration_amd", "cli.py")).read()
    assert src.count("offres_normal=getattr(args, \"b0_normal\", \"nufft\")") == 2   # both places an env is made
