"""CPU-only checks of the total-variation prior (pnp_tv_denoise, pnp_set_prior, pnp_get_prior): the three entry points are declared,
exported and bound; every argument error that needs no handle is reported without a GPU, from ctypes and from a C99 program, with the output
buffers untouched; `cli --prior tv` parses, refuses bad values and builds no U-Net; the float64 restatement the GPU tests compare against
(tests/tv_ref.py) checks itself; the fixture condition of the TV-ADMM checks holds; the float32 restatement is measured against the float64
one on every GPU case (tv_ref.F32_ERR is that measurement); the built code objects of the tv_* kernels have no scratch and no spills.

Figures of the reference, measured on the CPU: the TV-ADMM fixture (tv_ref.FIXTURE: 64 x 80, 4x, sigma 5/255, seed 1234, mu 0.3, sigma_d
50/255 -> 5/255 geometric over 30 iterations, tv_scale 1, tv_iters 20) goes from 28.256 dB (x0) to 35.884 dB.  The float32 restatement of
its first 10 iterations is within 3.374e-07 dB and max |dx| = 2.041e-07 of the float64 loop."""
import argparse
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tv_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, cli, denoiser, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("tv_fused_kernel", "tv_iter_kernel", "tv_close_kernel")


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "pnpadmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("pnp_tv_denoise", 6), ("pnp_set_prior", 4), ("pnp_get_prior", 4)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m is not None, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == nargs
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for name, val in (("PNP_TV_MAX_ITERS", 64), ("PNP_PRIOR_UNET", 0), ("PNP_PRIOR_TV", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src) and getattr(_lib, name) == val
    assert _lib.PRIORS == {"unet": 0, "tv": 1}
    mk = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\btv_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_tv_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    sig = inspect.signature(engine.PnPEngine.tv_denoise).parameters
    assert sig["iters"].default == R.ITERS == 20 and sig["out"].default is None
    sig = inspect.signature(engine.PnPEngine.set_prior).parameters
    assert (sig["tv_scale"].default, sig["tv_iters"].default) == (R.SCALE, R.ITERS) == (1.0, 20)
    assert isinstance(engine.PnPEngine.prior, property)
    sig = inspect.signature(denoiser.TVDenoiser2D.__init__).parameters
    assert (sig["scale"].default, sig["iters"].default) == (1.0, 20)
    for name in ("forward", "to", "eval", "engine_for", "__call__"):
        assert callable(getattr(denoiser.TVDenoiser2D, name)), name
    # the fusion depth the case table brackets is the one the kernels are built with
    internal = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "pnp_internal.h")).read()
    assert re.search(r"kTvT\s*=\s*%d\b" % R.FUSE_T, internal)
    assert R.FUSE_T in R.CASE_ITERS and R.FUSE_T + 1 in R.CASE_ITERS and {1, 7, 20, 64} <= set(R.CASE_ITERS)


# the errors that need no handle (every one is reported before the handle is looked at, and before any HIP call)
def _denoise(lib, a):
    return lib.pnp_tv_denoise(a["h"], a["x"], a["lam"], a["iters"], a["out"], None)


@pytest.mark.parametrize("key,val,what", [("h", None, b"null handle"), ("x", None, b"null x_in"), ("lam", None, b"null lam"),
                                          ("out", None, b"null out"), ("iters", 0, b"iters"), ("iters", 65, b"iters"), ("iters", -3, b"iters")])
def test_tv_denoise_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    buf, x = (C.c_float * 4)(), (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                      # never dereferenced: every case fails validation first
    a = dict(h=None, x=C.cast(x, C.c_void_p).value, lam=C.cast(x, C.c_void_p).value, iters=20, out=p)
    a[key] = val
    assert _denoise(lib, a) == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert list(buf) == [0.0] * 4


@pytest.mark.parametrize("prior,scale,iters,what", [(2, 1.0, 20, b"prior"), (-1, 1.0, 20, b"prior"), (1, -0.5, 20, b"tv_scale"),
                                                    (1, math.nan, 20, b"tv_scale"), (1, math.inf, 20, b"tv_scale"), (1, 1.0, 0, b"tv_iters"),
                                                    (1, 1.0, 65, b"tv_iters"), (1, 1.0, 20, b"null handle"), (0, 1.0, 20, b"null handle"),
                                                    (0, -1.0, 0, b"null handle")])
def test_set_prior_argument_errors_are_reported_without_a_gpu(prior, scale, iters, what):
    lib = _lib.load()
    assert lib.pnp_set_prior(None, prior, scale, iters) == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()


def test_get_prior_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    pr, sc, it = C.c_int(7), C.c_double(7.0), C.c_int(7)
    assert lib.pnp_get_prior(None, C.byref(pr), C.byref(sc), C.byref(it)) == -1 and b"null handle" in lib.pnp_last_error()
    for args in ((None, C.byref(sc), C.byref(it)), (C.byref(pr), None, C.byref(it)), (C.byref(pr), C.byref(sc), None)):
        assert lib.pnp_get_prior(None, *args) == -1 and b"null pointer" in lib.pnp_last_error()
    assert (pr.value, sc.value, it.value) == (7, 7.0, 7)


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    call = lambda expr, what, code: (
        "    if (%s != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"%s\")) return %d;\n" % (expr, what, code))
    src = tmp_path / "tv_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include <math.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float x[4] = {0};\n"
        "    float v[4] = {0};\n"
        "    int pr = 7, it = 7;\n"
        "    double sc = 7.0;\n"
        "    if (PNP_TV_MAX_ITERS != 64 || PNP_PRIOR_UNET != 0 || PNP_PRIOR_TV != 1) return 1;\n"
        + call("pnp_tv_denoise(0, x, x, 20, v, 0)", "null handle", 2)
        + call("pnp_tv_denoise(0, 0, x, 20, v, 0)", "null x_in", 3)
        + call("pnp_tv_denoise(0, x, 0, 20, v, 0)", "null lam", 4)
        + call("pnp_tv_denoise(0, x, x, 20, 0, 0)", "null out", 5)
        + call("pnp_tv_denoise(0, x, x, 0, v, 0)", "iters", 6)
        + call("pnp_tv_denoise(0, x, x, PNP_TV_MAX_ITERS + 1, v, 0)", "iters", 7)
        + call("pnp_set_prior(0, 2, 1.0, 20)", "prior", 8)
        + call("pnp_set_prior(0, PNP_PRIOR_TV, -1.0, 20)", "tv_scale", 9)
        + call("pnp_set_prior(0, PNP_PRIOR_TV, (double)NAN, 20)", "tv_scale", 10)
        + call("pnp_set_prior(0, PNP_PRIOR_TV, 1.0, 0)", "tv_iters", 11)
        + call("pnp_set_prior(0, PNP_PRIOR_TV, 1.0, 65)", "tv_iters", 12)
        + call("pnp_set_prior(0, PNP_PRIOR_TV, 1.0, 20)", "null handle", 13)
        + call("pnp_set_prior(0, PNP_PRIOR_UNET, 1.0, 20)", "null handle", 14)
        + call("pnp_get_prior(0, &pr, &sc, &it)", "null handle", 15)
        + call("pnp_get_prior(0, 0, &sc, &it)", "null pointer", 16) +
        "    if (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f || pr != 7 || it != 7 || sc != 7.0) return 17;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "tv_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_tv_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "tv_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur, lds = None, None                                                    # (the keys of a kernel come in alphabetical order: its LDS size before its name)
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                cur = m.group(2) if "tv_" in m.group(2) and "_kernel" in m.group(2) else None
                if cur:
                    meta[cur] = {"group_segment_fixed_size": lds}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    for k in KERNELS:
        assert sum(k in name for name in meta) == 2, k                           # the plane variant and the (z, u) variant of each
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        if "tv_fused_kernel" in name:
            assert m["group_segment_fixed_size"] == 64 * 1024, (name, m)          # the LDS footprint DESIGN.md states


# ---- the reference checks itself -------------------------------------------------------------------------------------------------

def test_lam_zero_is_the_clamp_and_a_constant_image_is_a_fixed_point():
    v, _ = R.case_input(1)
    for f32 in (False, True):
        assert np.array_equal(R.tv(v, np.zeros(3), 20, f32), np.clip(v.astype(np.float64), 0, 1))
        for c in (0.0, 0.3, 1.0, 1.7, -0.2):
            const = np.full((1, 16, 48), c, dtype=np.float32)
            for lam in (1e-6, 0.05, 10.0):
                out, p = R.tv(const, [lam], 9, f32, return_p=True)
                assert np.array_equal(out, np.clip(const.astype(np.float64), 0, 1))
                assert not p[0][0].any() and not p[0][1].any()


def test_the_divergence_is_the_negative_adjoint_and_the_mean_is_kept():
    rng = np.random.default_rng(3)
    a, py, px = rng.standard_normal((3, 1, 20, 28))
    gy, gx = R.grad(a)
    assert abs((gy * py + gx * px).sum() + (a * R.div_adjoint(py, px)).sum()) <= 1e-12 * np.abs(a).sum()
    for i in (1, 4):
        v, lam = R.case_input(i)
        _, ps = R.tv(v, lam, 20, return_p=True)
        for n, p in enumerate(ps):
            if p is None:
                continue
            assert not p[0][-1].any() and not p[1][:, -1].any()                  # what makes `div` the adjoint's end cases
            assert np.array_equal(R.div(*p), R.div_adjoint(*p))
            x = v[n].astype(np.float64) - float(lam[n]) * R.div(*p)              # before the clamp
            assert abs(x.mean() - v[n].astype(np.float64).mean()) <= 1e-12


def test_the_objective_falls_with_more_iterations_and_is_below_its_value_at_the_input():
    for i, n in ((1, 0), (4, 1), (5, 0)):
        v, lam = R.case_input(i)
        v = np.clip(v[n:n + 1].astype(np.float64), 0, 1)                         # inside [0, 1]: the clamp stays idle
        l = float(lam[n])
        o8, o64 = (R.objective(R.tv(v, [l], k)[0], v[0], l) for k in (8, 64))
        o0 = R.objective(v[0], v[0], l)
        print(f"case {i} slice {n} lam {l}: objective at x = v {o0:.6f}, K = 8 {o8:.6f}, K = 64 {o64:.6f}")
        assert o64 <= o8 <= o0


def test_the_transposed_input_gives_the_transposed_output():
    v, lam = R.case_input(1)
    for k in (1, 7, 20):
        a = R.tv(v, lam, k)
        b = R.tv(np.ascontiguousarray(v.transpose(0, 2, 1)), lam, k)
        assert np.array_equal(a, b.transpose(0, 2, 1))


def test_fixture_the_reference_tv_admm_ends_at_least_3_db_above_x0():
    d = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    assert len(sig) == 30 and abs(float(sig[0]) - 50 / 255) < 1e-7 and abs(float(sig[-1]) - 5 / 255) < 1e-7
    _, p0, p1 = R.admm_tv(d, mu, sig)
    print(f"TV-ADMM fixture: PSNR of x0 {p0[0]:.3f} dB, of the final x {p1[0]:.3f} dB")
    assert p1[0] - p0[0] >= 3.0
    k = R.FIXTURE["compare_iters"]
    mu, sig = R.fixture_schedules(k)
    x64, _, q64 = R.admm_tv(d, mu, sig)
    x32, _, q32 = R.admm_tv(d, mu, sig, f32=True)
    dp, dx = float(np.abs(q64 - q32).max()), float(np.abs(x64 - x32).max())
    print(f"float32 restatement of the first {k} iterations: |dPSNR| {dp:.3e} dB, max |dx| {dx:.3e} (tv_ref.ADMM_F32 = {R.ADMM_F32})")
    # the transform of the restatement is a library's float32 FFT: the recorded pair bounds it with a factor of two to spare for another build
    assert dp <= 2 * R.ADMM_F32[0] and dx <= 2 * R.ADMM_F32[1]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_the_float32_restatement_against_float64_is_the_recorded_table(i):
    assert len(R.CASES) == len(R.F32_ERR) == len(R.CASE_LAMS) and all(len(r) == len(R.CASE_ITERS) for r in R.F32_ERR)
    v, lam = R.case_input(i)
    assert v.shape == R.CASES[i] and lam.shape == (R.CASES[i][0],)
    assert v[0].min() < 0 and v[0].max() > 1                                    # one slice extends below 0 and above 1
    assert set(l for row in R.CASE_LAMS for l in row) == set(R.LAMS)
    for j, k in enumerate(R.CASE_ITERS):
        e = float(np.abs(R.case_ref(i, k, True) - R.case_ref(i, k)).max())
        print(f"case {i} {R.CASES[i]} lam {lam.tolist()} iters {k}: max |f32 - f64| = {e:.3e} (recorded {R.F32_ERR[i][j]:.3e})")
        assert abs(e - R.F32_ERR[i][j]) <= 2e-3 * R.F32_ERR[i][j]


# ---- Python and CLI surfaces -----------------------------------------------------------------------------------------------------------

def test_cli_takes_prior_tv_refuses_bad_values_and_builds_no_unet(monkeypatch):
    base = ["--block_size", "18", "--n_embeds", "9"]
    with pytest.raises(SystemExit, match="--tv-iters"):
        cli.main(base + ["--prior", "tv", "--tv-iters", "0", "eval"])
    with pytest.raises(SystemExit, match="--tv-iters"):
        cli.main(base + ["--prior", "tv", "--tv-iters", "65", "fixed"])
    with pytest.raises(SystemExit, match="--tv-scale"):
        cli.main(base + ["--prior", "tv", "--tv-scale", "-1", "mcts"])
    with pytest.raises(SystemExit, match="--tv-scale"):
        cli.main(base + ["--prior", "tv", "--tv-scale", "nan", "flex"])
    with pytest.raises(SystemExit, match="--denoiser-ckpt"):
        cli.main(base + ["--prior", "tv", "--denoiser-ckpt", "x.pt", "eval"])
    with pytest.raises(SystemExit):                                              # argparse: not a choice
        cli.main(base + ["--prior", "wavelet", "eval"])

    def no_unet(*_a, **_k):
        raise AssertionError("--prior tv must not build a U-Net")
    monkeypatch.setattr(denoiser.UNetDenoiser2D, "__init__", no_unet)
    monkeypatch.setattr(denoiser.UNetDenoiser2D, "seeded", classmethod(no_unet))
    den = cli._denoiser(argparse.Namespace(prior="tv", tv_scale=0.5, tv_iters=12, denoiser_ckpt=None, seed=0))
    assert isinstance(den, denoiser.TVDenoiser2D) and (den.scale, den.iters) == (0.5, 12) and den.to("cuda") is den and den.eval() is den

    class Parsed(Exception):
        pass
    seen = []

    def grab(args):
        seen.append((args.prior, args.tv_scale, args.tv_iters))
        raise Parsed
    monkeypatch.setattr(cli, "_denoiser", grab)
    for mode in ("eval", "flex", "mcts", "fixed"):
        with pytest.raises(Parsed):
            cli.main(base + ["--prior", "tv", "--tv-scale", "0.25", "--tv-iters", "40", mode])
    with pytest.raises(Parsed):
        cli.main(base + ["fixed"])
    assert seen == [("tv", 0.25, 40)] * 4 + [("unet", 1.0, 20)]
    with pytest.raises(ValueError, match="iters"):
        denoiser.TVDenoiser2D(iters=0)
    with pytest.raises(ValueError, match="scale"):
        denoiser.TVDenoiser2D(scale=float("inf"))
