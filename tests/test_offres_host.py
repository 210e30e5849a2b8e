"""CPU-only checks of the off-resonance correction: the entry points of include/pnpadmm_offres.h are declared, exported, bound from
`_lib.SIGNATURES_OFFRES` and classified in tests/offres_cases.py, while the four older headers and tables stay the sets they were; the header
compiles as C99 and links from C; every argument error that needs no handle comes back from ctypes without a GPU and leaves the outputs
untouched; the pure-host plan code (csrc/offres_plan.hip) is compiled into a stand-alone program with its own main (tests/asan_offres_host.cpp),
plain and with -fsanitize=address,undefined, refuses every invalid argument - a time that is not finite, a zero span with L > 1 - and gives
the bits of the restatement in tests/offres_ref.py, the per-(segment, tile) lists included; the derived bound holds for the float64
restatement; `offres_segments` returns the smallest L that meets its tolerance.

The rejections that read the handle - no NUFFT plan, no off-resonance plan, map_n not 1 or n - need a handle, and pnp_create needs a device:
tests/test_gpu_offres.py makes them.

The derived bound, on the CPU alone (16 x 16, spiral 4 x 96, 100 Hz, 10 ms): max_m |segmented - exact| / bound is printed per L and asserted
<= 1 + 1e-12; the bound is (1 - cos(omega_max D / 2)) ||p||_1 in the units of the orthonormal operator (1 / sqrt(H W))."""
import inspect
import math
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dcf_cases as DC  # noqa: E402
import handle_cases as HC  # noqa: E402
import ncsense_cases as NC  # noqa: E402
import nufft_ref as NR  # noqa: E402
import offres_cases as OC  # noqa: E402
import offres_ref as OR  # noqa: E402
import toeplitz_cases as TC  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ["pnp_acquire_offres", "pnp_offres_adjoint", "pnp_offres_cg_residual", "pnp_offres_forward", "pnp_offres_live", "pnp_offres_maps",
         "pnp_offres_normal", "pnp_offres_plan", "pnp_offres_segments", "pnp_reset_offres", "pnp_set_kspace_offres"]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


# ---- the table, the header, the binding -----------------------------------------------------------------------------------------------------

def test_the_new_header_the_table_and_the_binding_name_the_same_functions():
    text = _header(OC.HEADER)
    names = HC.header_functions(text)
    assert names == sorted(OC.ENTRY_POINTS) == sorted(_lib.SIGNATURES_OFFRES) == NAMES
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, (cls, nargs) in OC.ENTRY_POINTS.items():
        assert _nargs(src, name) == nargs == len(_lib.SIGNATURES_OFFRES[name][1]), name
        assert hasattr(lib, name), f"{name} declared in include/{OC.HEADER} but not exported"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_OFFRES[name][1]          # bound by _lib.load()'s loop
        assert cls in (HC.INTRUDER, HC.REPLACES, HC.STATELESS)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_offres.py")).read()
    for name, (cls, _) in OC.ENTRY_POINTS.items():
        if cls != HC.STATELESS:
            assert f"def {OC.COVERED_BY[name]}(" in gpu and name in gpu, name
    assert '#include "pnpadmm.h"' in text and 'extern "C"' in text
    for gone in OC.ENTRY_POINTS:                                                    # deleting any row of the table is noticed
        assert OC.missing(names, {k: v for k, v in OC.ENTRY_POINTS.items() if k != gone}) == [gone]
    assert OC.missing(names) == []
    for word in ("OUT OF SCOPE", "Toeplitz", "PNP_OFFRES_NAIVE", "PNP_OFFRES_SEG_BLOCK", "fma(b1"):
        assert word in text, word


def test_the_four_older_headers_and_tables_are_the_sets_they_were():
    old = HC.header_functions(_header("pnpadmm.h"))
    assert old == sorted(_lib.SIGNATURES) == sorted(HC.ENTRY_POINTS) and len(old) == 57
    ns = HC.header_functions(_header(NC.HEADER))
    assert ns == sorted(_lib.SIGNATURES_NCSENSE) == sorted(NC.ENTRY_POINTS) and len(ns) == 8
    tz = HC.header_functions(_header(TC.HEADER))
    assert tz == sorted(_lib.SIGNATURES_TOEPLITZ) == sorted(TC.ENTRY_POINTS) and len(tz) == 10
    dc = HC.header_functions(_header(DC.HEADER))
    assert dc == sorted(_lib.SIGNATURES_DCF) == sorted(DC.ENTRY_POINTS) and len(dc) == 2
    new = set(OC.ENTRY_POINTS)
    for older in (old, ns, tz, dc):
        assert not new & set(older)
    for h in ("pnpadmm.h", NC.HEADER, TC.HEADER, DC.HEADER):
        assert "offres" not in _header(h)


def test_build_files_the_units_and_the_python_layers():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\boffres_kernels\.o\b.*\boffres_plan\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_offres_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert len(re.findall(r"^(?:_asan/)?%\.o:.*offres_plan\.h.*pnpadmm_offres\.h", mk, flags=re.M)) == 2           # both dependency lists
    unit = open(os.path.join(CSRC, "offres_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit
    assert "atomic" not in unit.lower().replace("no atomics", "")
    assert "cooperative" not in unit.lower()                                       # a launch ends; the next starts
    plan_src = open(os.path.join(CSRC, "offres_plan.hip")).read() + open(os.path.join(CSRC, "offres_plan.h")).read()
    assert "hip_runtime" not in plan_src and "pnp_internal.h" not in plan_src          # pure host code: no HIP header, no HIP call
    for name, params in (("offres_plan", ["self", "times", "segments"]), ("offres_maps", ["self", "omega"]),
                         ("offres_forward", ["self", "img", "maps"]), ("offres_adjoint", ["self", "samples", "maps", "weights"]),
                         ("reset_offres", ["self", "x0", "y", "omega", "w", "cg_iters"]),
                         ("set_kspace_offres", ["self", "y", "omega", "w", "episode", "cg_iters"]), ("offres_normal", ["self", "p", "mu"]),
                         ("offres_cg_residual", ["self"]), ("acquire_offres", ["self", "gt", "omega", "sigma_n", "seed", "dcf"])):
        assert list(inspect.signature(getattr(engine.PnPEngine, name)).parameters) == params, name
    assert list(inspect.signature(acquisition.readout_times).parameters) == ["traj_kind", "m", "readout", "t_read", "te"]
    assert list(inspect.signature(acquisition.offres_segments).parameters) == ["omega_max", "span", "tol"]
    assert list(inspect.signature(synthetic.field_map).parameters) == ["h", "w", "max_hz", "seed"]
    sim = inspect.signature(acquisition.simulate).parameters
    assert sim["omega"].default is None and sim["times"].default is None and sim["segments"].default == "auto"


def test_the_new_header_is_plain_c_and_links_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm_offres.h"\n'
        "int main(void) {\n"
        "    double t[4] = {0.0, 1e-3, 2e-3, 3e-3};\n"
        "    float y[4] = {1.f, 2.f, 3.f, 4.f};\n"
        "    if (pnp_offres_plan(0, t, 0, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"segments\")) return 1;\n"
        "    if (pnp_offres_plan(0, t, PNP_MC_MAX_COILS + 1, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"segments\")) return 2;\n"
        "    if (pnp_offres_plan(0, t, 4, 1) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"flags\")) return 3;\n"
        "    if (pnp_offres_plan(0, 0, 4, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null t\")) return 4;\n"
        "    if (pnp_offres_plan(0, t, 4, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 5;\n"
        "    if (pnp_offres_maps(0, y, 0, y + 2, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"map_n\")) return 6;\n"
        "    if (pnp_offres_segments(0) != 0 || pnp_offres_live(0) != 0) return 7;\n"
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
    t = np.linspace(0.0, 1e-2, 16)
    out, out2, out3 = (np.full(64, 7.0, dtype=np.float32) for _ in range(3))
    pa, pb, pt, po, po2, po3 = (v.ctypes.data for v in (a, b, t, out, out2, out3))
    nan, inf = float("nan"), float("inf")
    cases = [
        (lambda: lib.pnp_offres_plan(None, pt, 4, 1), b"flags"),
        (lambda: lib.pnp_offres_plan(None, pt, 4, -1), b"flags"),
        (lambda: lib.pnp_offres_plan(None, pt, 0, 0), b"segments must be 1..32 (got 0)"),
        (lambda: lib.pnp_offres_plan(None, pt, 33, 0), b"segments must be 1..32 (got 33)"),
        (lambda: lib.pnp_offres_plan(None, None, -1, 0), b"segments"),                  # scalar ranges first
        (lambda: lib.pnp_offres_plan(None, None, 4, 0), b"null t"),
        (lambda: lib.pnp_offres_plan(None, pt, 1, 0), b"null handle"),
        (lambda: lib.pnp_offres_plan(None, pt, 32, 0), b"null handle"),
        (lambda: lib.pnp_offres_maps(None, pa, 0, po, None), b"map_n must be 1 or n (got 0)"),
        (lambda: lib.pnp_offres_maps(None, None, 1, po, None), b"null omega"),
        (lambda: lib.pnp_offres_maps(None, pa, 1, None, None), b"null maps"),
        (lambda: lib.pnp_offres_maps(None, pa, 1, pa, None), b"alias"),
        (lambda: lib.pnp_offres_maps(None, pa, 1, po, None), b"null handle"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 0, 1, po, None), b"map_n"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 1, 0, po, None), b"batch must be 1..n (got 0)"),
        (lambda: lib.pnp_offres_forward(None, None, pb, 1, 1, po, None), b"null img"),
        (lambda: lib.pnp_offres_forward(None, pa, None, 1, 1, po, None), b"null maps"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 1, 1, None, None), b"null samples"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 1, 1, pa, None), b"alias"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 1, 1, pb, None), b"alias"),
        (lambda: lib.pnp_offres_forward(None, pa, pb, 1, 1, po, None), b"null handle"),
        (lambda: lib.pnp_offres_adjoint(None, pa, None, pb, -3, 1, po, None), b"map_n"),
        (lambda: lib.pnp_offres_adjoint(None, pa, None, pb, 1, -1, po, None), b"batch"),
        (lambda: lib.pnp_offres_adjoint(None, None, None, pb, 1, 1, po, None), b"null samples"),
        (lambda: lib.pnp_offres_adjoint(None, pa, None, None, 1, 1, po, None), b"null maps"),
        (lambda: lib.pnp_offres_adjoint(None, pa, None, pb, 1, 1, None, None), b"null img"),
        (lambda: lib.pnp_offres_adjoint(None, pa, po, pb, 1, 1, po, None), b"alias"),
        (lambda: lib.pnp_offres_adjoint(None, pa, None, pb, 1, 1, po, None), b"null handle"),
        (lambda: lib.pnp_set_kspace_offres(None, pa, pb, 0, None, 8, None), b"map_n"),
        (lambda: lib.pnp_set_kspace_offres(None, pa, pb, 1, None, 0, None), b"cg_iters must be 1..64 (got 0)"),
        (lambda: lib.pnp_set_kspace_offres(None, pa, pb, 1, None, 65, None), b"cg_iters"),
        (lambda: lib.pnp_set_kspace_offres(None, None, pb, 1, None, 8, None), b"null y"),
        (lambda: lib.pnp_set_kspace_offres(None, pa, None, 1, None, 8, None), b"null omega"),
        (lambda: lib.pnp_set_kspace_offres(None, pa, pb, 1, None, 8, None), b"null handle"),
        (lambda: lib.pnp_reset_offres(None, None, pa, pb, 1, None, 8, po, po2, po3, None), b"null x0"),
        (lambda: lib.pnp_reset_offres(None, pa, None, pb, 1, None, 8, po, po2, po3, None), b"null y"),
        (lambda: lib.pnp_reset_offres(None, pa, pa, None, 1, None, 8, po, po2, po3, None), b"null omega"),
        (lambda: lib.pnp_reset_offres(None, pa, pa, pb, 1, None, 8, None, po2, po3, None), b"null x, z or u"),
        (lambda: lib.pnp_reset_offres(None, pa, pa, pb, 1, None, 8, po, po2, None, None), b"null x, z or u"),
        (lambda: lib.pnp_reset_offres(None, pa, pa, pb, 1, None, 8, po, po2, po3, None), b"null handle"),
        (lambda: lib.pnp_offres_cg_residual(None, po, None), b"null argument"),
        (lambda: lib.pnp_offres_normal(None, pa, pb, po, None), b"null argument"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, 0.0, 0, 1, po, po2, po3, None), b"flags"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, -1.0, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, nan, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, inf, 0, 0, po, po2, po3, None), b"sigma_n"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 0, None, 0.0, 0, 0, po, po2, po3, None), b"map_n"),
        (lambda: lib.pnp_acquire_offres(None, None, pb, 1, None, 0.0, 0, 0, po, po2, po3, None), b"null gt"),
        (lambda: lib.pnp_acquire_offres(None, pa, None, 1, None, 0.0, 0, 0, po, po2, po3, None), b"null omega"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, 0.0, 0, 0, None, po2, po3, None), b"null y"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, 0.0, 0, 0, po, po, po3, None), b"alias"),
        (lambda: lib.pnp_acquire_offres(None, pa, pb, 1, None, 0.0, 0, 0, po, None, None, None), b"null handle"),
    ]
    for i, (call, what) in enumerate(cases):
        assert call() == -1, i
        assert what in lib.pnp_last_error(), (i, what, lib.pnp_last_error())
    assert lib.pnp_offres_segments(None) == 0 and lib.pnp_offres_live(None) == 0
    for o in (out, out2, out3):
        assert (o == 7.0).all()
    assert np.array_equal(a, np.arange(64, dtype=np.float32)) and np.array_equal(b, np.arange(64, dtype=np.float32) + 100.0)


# ---- the pure-host plan code: the stand-alone program, plain and sanitized -------------------------------------------------------------------

def _build(workdir, sanitize):
    exe = os.path.join(workdir, "asan_offres_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-std=c++17", "--offload-arch=gfx950"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "tests", "asan_offres_host.cpp"), os.path.join(CSRC, "offres_plan.hip"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def plan_tools(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("offres_plan_host"))
    return d, _build(d, False), _build(d, True)


def test_plan_builder_refuses_every_invalid_argument(plan_tools):
    for exe in plan_tools[1:]:
        r = subprocess.run([exe, "--invalid"], capture_output=True, text=True)
        assert r.returncode == 0 and "asan_offres_host: invalid ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _bins(P):
    tiles = (P["gh"] // NR.TILE) * (P["gw"] // NR.TILE)
    lists = [[] for _ in range(tiles)]
    for s in range(P["m"]):
        for (a, b) in NR.tiles_of(P, s):
            lists[a * (P["gw"] // NR.TILE) + b].append(s)
    off = np.zeros(tiles + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(v) for v in lists])
    return tiles, off, np.array([s for v in lists for s in v], dtype=np.int32)


def _times_case(k, m):
    """sample times that hit the edges: t_max itself, exact centres, a repeated value, and unordered readouts"""
    if k == 0:                                                                     # three readouts of the same clock
        return acquisition.readout_times("spiral", m, m // 4, 8e-3, te=1e-3)
    if k == 1:                                                                     # dyadic: every centre of L = 2, 3, 5, 9 is hit exactly
        return (np.arange(m, dtype=np.float64) % 17) * 2.0 ** -10
    rng = np.random.default_rng(7)
    t = rng.random(m) * 5e-3 - 1e-3                                                 # negative times too
    t[3], t[5] = t.max(), t.min()
    return t


@pytest.mark.parametrize("k", range(3))
def test_plan_builder_gives_the_restatements_bits_and_complete_ascending_lists(plan_tools, k):
    d, *exes = plan_tools
    traj, m, _ = OR.case_traj("spiral", 32, 32)
    P = NR.plan(32, 32, 64, 64, 4, traj)
    tiles, off, idx = _bins(P)
    t = _times_case(k, m)
    path = os.path.join(d, f"in{k}.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<qi", m, tiles) + t.tobytes() + off.tobytes() + idx.tobytes())
    for L in (1, 2, 3, 8, 9, 32):
        Q = OR.plan(t, L)
        for exe in exes:
            outp = os.path.join(d, f"out{k}.bin")
            r = subprocess.run([exe, "--dump", path, str(L), outp], capture_output=True, text=True)
            assert r.returncode == 0 and "dump ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
            raw = open(outp, "rb").read()
            tau = np.frombuffer(raw, np.float64, L, 0)
            seg = np.frombuffer(raw, np.int32, m, 8 * L)
            b0 = np.frombuffer(raw, np.float32, m, 8 * L + 4 * m)
            b1 = np.frombuffer(raw, np.float32, m, 8 * L + 8 * m)
            loff = np.frombuffer(raw, np.int32, L * tiles + 1, 8 * L + 12 * m)
            lidx = np.frombuffer(raw, np.int32, -1, 8 * L + 12 * m + 4 * (L * tiles + 1))
            assert np.array_equal(tau.view(np.int64), Q["tau"].view(np.int64)), (k, L)
            assert np.array_equal(seg, Q["seg"]) and np.array_equal(b0.view(np.int32), Q["b0"].view(np.int32))
            assert np.array_equal(b1.view(np.int32), Q["b1"].view(np.int32))
            assert seg.min() >= 0 and seg.max() <= max(L - 2, 0) and (b0 >= 0).all() and (b1 >= 0).all() and (b0 <= 1).all() and (b1 <= 1).all()
            assert loff[0] == 0 and loff[-1] == lidx.size == (2 if L > 1 else 1) * idx.size
            for l in range(L):
                for tile in range(tiles):
                    want = [s for s in idx[off[tile]:off[tile + 1]] if Q["seg"][s] == l or (L > 1 and Q["seg"][s] == l - 1)]
                    got = lidx[loff[l * tiles + tile]:loff[l * tiles + tile + 1]]
                    assert list(got) == want and all(x < y for x, y in zip(want, want[1:])), (k, L, l, tile)
        if L > 1:
            i = int(np.argmax(t))
            # a sample at exactly t_max: b1 = 1; b0 = float32(1 - b) is 0 or the float64 rounding of tau and the division, below 2^-49
            assert Q["seg"][i] == L - 2 and Q["b1"][i] == 1.0 and 0.0 <= Q["b0"][i] <= 2.0 ** -49
        if k == 1 and L in (2, 3, 5, 9):                                            # samples at exactly a centre: one segment carries them
            on = np.isin(t, Q["tau"])
            assert on.any() and (((Q["b0"] == 1) & (Q["b1"] == 0)) | ((Q["b0"] == 0) & (Q["b1"] == 1)))[on].all()
        assert np.array_equal(OR.weights(Q).sum(axis=0) > 0, np.ones(m, bool)) and np.abs(OR.weights(Q).sum(axis=0) - 1).max() < 1e-7
    Q1, Q2 = OR.plan(t, 1), OR.plan(t, 2)
    assert Q1["tau"][0] == 0.5 * (t.min() + t.max()) and (Q1["b0"] == 1).all() and (Q1["b1"] == 0).all() and (Q1["seg"] == 0).all()
    assert (Q2["seg"] == 0).all() and Q2["tau"][0] == t.min() and Q2["tau"][1] == t.min() + (t.max() - t.min())


# ---- the model, the bound, the segment chooser -----------------------------------------------------------------------------------------------

def test_readout_times_field_map_and_the_segment_chooser():
    t = acquisition.readout_times("spiral", 4 * 96, 96, 10e-3, te=2e-3)
    assert t.shape == (384,) and t.dtype == np.float64 and t[0] == 2e-3 and t[96] == 2e-3 and t[95] == 2e-3 + 95 * 10e-3 / 96
    assert np.array_equal(acquisition.readout_times("rosette", 50, 50, 1.0), np.arange(50) / 50.0)
    for bad in (lambda: acquisition.readout_times("lissajous", 8, 4, 1.0), lambda: acquisition.readout_times("radial", 9, 4, 1.0),
                lambda: acquisition.readout_times("radial", 8, 4, 0.0), lambda: acquisition.readout_times("radial", 8, 4, 1.0, te=float("nan"))):
        with pytest.raises(ValueError):
            bad()
    f = synthetic.field_map(32, 48, 100.0, 3)
    assert f.shape == (32, 48) and f.dtype == np.float64 and abs(np.abs(f).max() - 100.0) < 1e-9
    assert np.abs(np.diff(f, axis=0)).max() < 25.0 and np.abs(np.diff(f, axis=1)).max() < 25.0      # smooth: no jump of a quarter of the range
    assert not np.array_equal(f, synthetic.field_map(32, 48, 100.0, 4))
    for om, span, tol in ((2 * math.pi * 100.0, 10e-3, 1e-3), (2 * math.pi * 100.0, 10e-3, 1e-2), (50.0, 3e-3, 1e-4), (3 * math.pi / 5e-3, 5e-3, 1e-3)):
        L = acquisition.offres_segments(om, span, tol)
        assert L == OR.segments_for(om, span, tol) and L >= 2
        assert 1.0 - math.cos(om * span / (L - 1) / 2.0) <= tol
        assert L == 2 or not 1.0 - math.cos(om * span / (L - 2) / 2.0) <= tol, (om, span, tol, L)      # the smallest
    assert acquisition.offres_segments(0.0, 1e-2) == 1 and acquisition.offres_segments(100.0, 0.0) == 1
    # the chooser is arithmetic: at tol = 1e-3 the linear interpolator needs 2 acos(0.999) = 0.0894 rad per segment, more than the library's
    # 32 segments give from omega_max span = 2.8 rad on; offres_bound says what 32 segments leave
    L100 = acquisition.offres_segments(2 * math.pi * 100.0, 10e-3)
    print(f"offres_segments(100 Hz, 10 ms, 1e-3) = {L100}; with {acquisition.OFFRES_MAX_SEGMENTS} segments the bound is "
          f"{acquisition.offres_bound(2 * math.pi * 100.0, 10e-3, 32):.3e}; offres_segments(3 pi) = {acquisition.offres_segments(3 * math.pi, 1.0)}")
    assert L100 == 72 and acquisition.offres_segments(3 * math.pi, 1.0) == 107 and acquisition.OFFRES_MAX_SEGMENTS == 32
    assert acquisition.offres_bound(2 * math.pi * 100.0, 10e-3, 32) == 1.0 - math.cos(2 * math.pi / 31 / 2.0)


@pytest.mark.parametrize("L", (2, 3, 8))
def test_the_derived_bound_holds_for_the_restatement(L):
    h = w = 16
    traj, m, R = OR.case_traj("spiral", h, w)
    t = acquisition.readout_times("spiral", m, R, 10e-3)
    om = OR.case_omega(h, w, 100.0, 1).astype(np.float64)
    om_max = float(np.abs(om).max())
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, h, w)) + 1j * rng.standard_normal((2, h, w))
    Q = OR.plan(t, L)
    seg, ex = OR.segmented_forward(traj, Q, om, x, unrounded=True), OR.exact_forward(traj, t, om, x)
    bnd = OR.bound(om_max, Q["step"], x)
    err = np.abs(seg - ex).max(axis=1)
    print(f"L = {L}: D = {Q['step']:.3e} s, omega_max D / 2 = {om_max * Q['step'] / 2:.3f} rad, max |segmented - exact| {err.tolist()}, bound {bnd.tolist()}, "
          f"ratio {(err / bnd).max():.3f}")
    assert (err <= bnd * (1.0 + 1e-12)).all()                                       # the float64 interpolator: the model the bound is derived for
    r32 = np.abs(OR.segmented_forward(traj, Q, om, x) - seg).max(axis=1)            # ... and what rounding b0, b1 to float32 adds: <= 2^-24 ||p||_1 each
    print(f"        float32 b0, b1 move a sample by at most {r32.tolist()}")
    assert (r32 <= 2.0 ** -23 * np.abs(x).reshape(2, -1).sum(axis=1) / math.sqrt(h * w)).all()
    # the adjoint of the restatement is the adjoint: <A p, q> = <p, A^H q> in float64
    q = rng.standard_normal((2, m)) + 1j * rng.standard_normal((2, m))
    for fwd, adj in ((OR.segmented_forward(traj, Q, om, x), OR.segmented_adjoint(traj, Q, om, q, h, w)), (ex, OR.exact_adjoint(traj, t, om, q, h, w))):
        a, b = np.vdot(q, fwd), np.vdot(adj, x)
        assert abs(a - b) <= 1e-12 * abs(a)


# ---- the correction corrects, in float64 on the CPU: the figures the GPU test is held to ---------------------------------------------------------

def test_the_restatement_alone_shows_that_the_correction_corrects():
    """offres_ref.CORRECTS in float64 on the NUFFT model: the off-resonance stage against the plain stage on the same y (from the exact
    operator); produces offres_ref.CORRECTS_PSNR"""
    import dcf_ref
    c = OR.CORRECTS
    traj, t, omega, gt, y, L = OR.corrects_problem()
    assert L == 32 and abs(float(np.abs(omega).max()) * float(t.max() - t.min()) - 3 * math.pi) < 1e-5
    P = NR.plan(c["h"], c["w"], c["grid"][0], c["grid"][1], c["J"], traj)
    dcf = dcf_ref.pipe(P, 30)[0]
    Q = OR.plan(t, L)
    E = OR.maps(omega, Q).astype(np.complex64).astype(np.complex128)
    corrected = OR.corrects_admm(P, lambda p: OR.model_forward(P, Q, E, p), lambda q: OR.model_adjoint(P, Q, E, q, dcf), y, gt, dcf)
    plain = OR.corrects_admm(P, lambda p: NR.forward(P, p), lambda q: NR.adjoint(P, q, dcf), y, gt, dcf)
    lim = math.sqrt(dcf.sum()) * (float(OR.bound(float(np.abs(omega).max()), Q["step"], gt[None])[0]) + (1e-6 + 2 * 1.327e-05) * np.abs(y).max())
    print(f"float64, L = {L}: off-resonance stage {corrected[0]:.4f} dB, plain stage {plain[0]:.4f} dB (recorded {OR.CORRECTS_PSNR}); DC at x = gt "
          f"{corrected[1]:.4e} / {plain[1]:.4e} around the bound {lim:.4e}")
    assert corrected[0] > plain[0] + 10.0 and corrected[1] < lim < plain[1]
    assert abs(corrected[0] - OR.CORRECTS_PSNR[0]) <= 2e-3 and abs(plain[0] - OR.CORRECTS_PSNR[1]) <= 2e-3


# ---- task_problem, PnPEnv, the CLI ---------------------------------------------------------------------------------------------------------------

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
        return self.offres is not None and np.array_equal(self.offres[0], np.asarray(times)) and self.offres[1] == segments

    def offres_plan(self, times, segments):
        self.calls.append(("offres_plan", tuple(times.shape), segments))
        self.offres, self.live_episode = (np.asarray(times).copy(), segments), 0

    def reset_offres(self, x0, y, omega, w=None, cg_iters=8):
        self.calls.append(("reset_offres", tuple(y.shape), tuple(omega.shape), w is not None, cg_iters))
        self.live_episode = 77
        return x0.real.clone(), x0.clone(), x0 * 0

    def set_kspace_offres(self, y, omega, w=None, episode=0, cg_iters=8):
        self.calls.append(("set_kspace_offres", tuple(y.shape), tuple(omega.shape), w is not None, episode, cg_iters))
        self.live_episode = episode

    def reset_nc(self, *a, **k):
        raise AssertionError("the plain stage was installed for an episode with a field map")

    set_kspace_nc = reset_ncsense = set_kspace_ncsense = reset_nc


def test_task_problem_builds_the_field_map_the_times_and_hands_them_to_simulate(monkeypatch):
    calls = []

    def fake_simulate(eng, gt, mask, sigma_n, seed, first_slice=0, **k):
        calls.append(k)
        return {}

    monkeypatch.setattr(acquisition, "simulate", fake_simulate)
    monkeypatch.setattr(acquisition, "pipe_dcf", lambda *a, **k: "PIPE")
    gt = np.zeros((2, 64, 64), dtype=np.float32)
    e = _FakeEngine()
    acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc")                 # without b0_hz: the call the parent made, word for word
    assert sorted(calls[-1]) == ["dcf", "nufft_grid", "nufft_width", "sens", "traj"]
    for kind, kw, m, readout in (("radial-nc", {}, 16 * 128, 128), ("spiral-nc", {}, 8 * 805, 805), ("spiral-nc", {"interleaves": 5}, 5 * 1408, 1408),
                                 ("rosette-nc", {}, 1710, 1710)):
        acquisition.task_problem("4x_10", gt, e, seed=4, mask_kind=kind, b0_hz=80.0, readout_ms=12.0, b0_segments=9, **kw)
        k = calls[-1]
        assert k["traj"].shape == (m, 2) and k["segments"] == 9 and "sens" not in k
        assert np.array_equal(k["times"], acquisition.readout_times(kind[:-3], m, readout, 12e-3))
        assert k["omega"].dtype == np.float32 and k["omega"].shape == (64, 64)
        assert np.array_equal(k["omega"], (2 * math.pi * synthetic.field_map(64, 64, 80.0, 4)).astype(np.float32))
    acquisition.task_problem("4x_10", gt, e, mask_kind="spiral-nc", b0_hz=80.0, readout_ms=12.0)
    assert calls[-1]["segments"] == "auto"
    for bad, what in ((dict(mask_kind="spiral-nc", b0_hz=80.0), "readout_ms"), (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=0.0), "readout_ms"),
                      (dict(mask_kind="spiral-nc", b0_hz=-1.0, readout_ms=5.0), "b0_hz"),
                      (dict(mask_kind="spiral-nc", b0_hz=80.0, readout_ms=5.0, coils=2), "single-coil"),
                      (dict(mask_kind="radial", b0_hz=80.0, readout_ms=5.0), "non-Cartesian"), (dict(mask_kind="radial", readout_ms=5.0), "non-Cartesian")):
        with pytest.raises(ValueError, match=what):
            acquisition.task_problem("4x_10", gt, e, **bad)
    names = list(inspect.signature(acquisition.task_problem).parameters)
    assert names[names.index("nufft_width") + 1:names.index("nufft_grid")] == ["b0_hz", "readout_ms", "b0_segments"]
    sig = inspect.signature(acquisition.task_problem).parameters
    assert sig["b0_hz"].default is None and sig["readout_ms"].default is None and sig["b0_segments"].default == "auto"


def test_the_environment_installs_and_rebinds_an_off_resonance_episode():
    import torch
    from dt4image_restoration_amd import env as envmod
    n, h, w, m = 2, 16, 16, 48
    fake = _FakeEngine()
    env = envmod.PnPEnv.__new__(envmod.PnPEnv)
    env.nc_normal, env.cg_iters, env.nufft_width, env.nufft_grid = "nufft", 5, 6, None
    env._engine_for = lambda *a: fake
    times = np.tile(np.arange(24) * 1e-4, 2)
    omega = torch.full((h, w), 2 * math.pi * 100.0)
    data = {"x0": torch.zeros(n, 1, h, w, 2), "y0": torch.zeros(n, 1, m, 2), "gt": torch.zeros(n, 1, h, w), "traj": torch.zeros(m, 2, dtype=torch.float64),
            "dcf": torch.ones(m), "omega": omega, "times": torch.from_numpy(times), "segments": 4}
    x0 = torch.zeros(n, 1, h, w, dtype=torch.complex64)
    st = env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    assert [c[0] for c in fake.calls] == ["nufft_plan", "offres_plan", "reset_offres"]
    assert fake.calls[1] == ("offres_plan", (m,), 4) and fake.calls[2] == ("reset_offres", (n, m), (h, w), True, 5)
    assert st["segments"] == 4 and st["_episode"] == 77 and torch.equal(st["omega"], omega) and st["times"].dtype == torch.float64 and st["sens"] is None
    del fake.calls[:]
    env._bind_episode(fake, st)                                                     # the live episode: nothing to do
    assert fake.calls == []
    fake.live_episode = 5                                                           # another episode ran in between
    env._bind_episode(fake, st)
    assert fake.calls == [("set_kspace_offres", (n, m), (h, w), True, 77, 5)]
    del fake.calls[:]
    fake.offres = None                                                              # ... or the plan was replaced
    env._bind_episode(fake, st)
    assert [c[0] for c in fake.calls] == ["offres_plan", "set_kspace_offres"]
    auto = dict(data)
    del auto["segments"]                                                            # the chooser: 2 pi 100 Hz over 2.3 ms = 1.45 rad -> 18 segments
    st = env._reset_nc(auto, x0, n, h, w, torch.device("cpu"))
    want = acquisition.offres_segments(2 * math.pi * 100.0, 23e-4)
    assert st["segments"] == want == OR.segments_for(2 * math.pi * 100.0, 23e-4) and 2 <= want <= 32
    big = dict(auto, omega=omega * 10.0)                                            # 14.5 rad asks for more than the library takes
    assert acquisition.offres_segments(2 * math.pi * 1000.0, 23e-4) > 32 and env._reset_nc(big, x0, n, h, w, torch.device("cpu"))["segments"] == 32
    for bad, what in (({k: v for k, v in data.items() if k != "times"}, "times"), (dict(data, times=torch.zeros(5, dtype=torch.float64)), "times"),
                      (dict(data, sens=torch.ones(2, h, w, dtype=torch.complex64), y0=torch.zeros(n, 2, m, 2)), "single-coil")):
        with pytest.raises(ValueError, match=what):
            env._reset_nc(bad, x0, n, h, w, torch.device("cpu"))
    env.nc_normal = "toeplitz"
    with pytest.raises(ValueError, match="Toeplitz"):
        env._reset_nc(data, x0, n, h, w, torch.device("cpu"))
    for name in ("reset", "set_kspace"):
        p = inspect.signature(getattr(engine.PnPEngine, name)).parameters
        assert [k for k in ("omega", "times", "segments", "w") if k in p] == ["omega", "times", "segments", "w"] and p["omega"].default is None
    assert list(inspect.signature(engine.PnPEngine.offres_planned).parameters) == ["self", "times", "segments"]


def test_cli_b0_choices_and_refusals():
    from dt4image_restoration_amd import cli
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--b0", "50"], "need --traj"), (["--readout-ms", "5"], "need --traj"), (["--b0-segments", "4"], "need --traj"),
                        (["--traj", "spiral", "--b0", "50"], "--b0 needs --readout-ms"),
                        (["--traj", "spiral", "--b0", "50", "--readout-ms", "0"], "--b0 needs --readout-ms"),
                        (["--traj", "spiral", "--b0", "-1", "--readout-ms", "5"], "--b0 must be"),
                        (["--traj", "spiral", "--readout-ms", "5"], "need --b0"), (["--traj", "radial", "--b0-segments", "4"], "need --b0"),
                        (["--traj", "radial", "--b0", "50", "--readout-ms", "5", "--nc-coils", "2"], "single-coil"),
                        (["--traj", "rosette", "--b0", "50", "--readout-ms", "5", "--nc-normal", "toeplitz"], "no Toeplitz form"),
                        (["--traj", "spiral", "--b0", "50", "--readout-ms", "5", "--b0-segments", "0"], "--b0-segments must be 1..32 or auto"),
                        (["--traj", "spiral", "--b0", "50", "--readout-ms", "5", "--b0-segments", "33"], "--b0-segments must be 1..32 or auto"),
                        (["--traj", "spiral", "--b0", "50", "--readout-ms", "5", "--b0-segments", "many"], "--b0-segments must be 1..32 or auto")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])

    class A:
        traj, spokes, nc_weights, nufft_width, nufft_grid, nc_coils, interleaves, petals, dcf_iters = "spiral", None, "dcf", 6, None, 0, 4, None, 30
        b0, readout_ms, b0_segments = None, None, "auto"
    assert sorted(cli._nc_kwargs(A)) == ["coils", "dcf_iters", "interleaves", "mask_kind", "nc_weights", "nufft_grid", "nufft_width", "petals", "spokes"]
    A.b0, A.readout_ms, A.b0_segments = 50.0, 5.0, 8
    kw = cli._nc_kwargs(A)
    assert (kw["b0_hz"], kw["readout_ms"], kw["b0_segments"]) == (50.0, 5.0, 8)
