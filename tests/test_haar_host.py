"""CPU-only checks of the Haar wavelet prior (pnp_haar_denoise, pnp_set_prior_haar, pnp_get_prior_haar): the three entry points are
declared, exported and bound; every argument error that needs no handle is reported without a GPU, from ctypes and from a C99 program, with
the output buffers untouched; `cli --prior haar` parses, refuses bad values and builds no U-Net; the float64 restatement the GPU tests
compare against (tests/haar_ref.py) checks itself; the fixture condition of the Haar-ADMM checks holds; the float32 restatement is measured
against the float64 one on every GPU case (haar_ref.F32_ERR is that measurement); the built code objects of the haar_* kernels have no
scratch and no spills.

Figures of the reference, measured on the CPU: the Haar-ADMM fixture (haar_ref.FIXTURE: 64 x 80, 4x, sigma 5/255, seed 1234, mu 0.3, sigma_d
50/255 -> 5/255 geometric over 30 iterations, haar_scale 1, 3 levels, TI) goes from 28.256 dB (x0) to 34.824 dB (the decimated transform with
the same settings: 28.647 dB).  The float32 restatement of its first 10 iterations is within 2.824e-07 dB and max |dx| = 2.303e-07 of the
float64 loop."""
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
import haar_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, cli, denoiser, engine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"haar_ti_fused_kernel": 2 * R.MAX_LEVELS, "haar_ti_down_kernel": 2, "haar_ti_up_kernel": 2, "haar_ortho_kernel": 2}
# LDS of the fused kernel as DESIGN.md states it: a_(j-1) with a margin of 8 all round (144^2 floats) and, from two levels on, r_j with a
# margin above and to the left (136^2 floats)
FUSED_LDS = {1: 144 * 144 * 4, 2: (144 * 144 + 136 * 136) * 4, 3: (144 * 144 + 136 * 136) * 4, 4: (144 * 144 + 136 * 136) * 4}


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "pnpadmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name, nargs in (("pnp_haar_denoise", 7), ("pnp_set_prior_haar", 4), ("pnp_get_prior_haar", 4)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m is not None, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == nargs
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    for name, val in (("PNP_PRIOR_HAAR", 2), ("PNP_HAAR_TI", 0), ("PNP_HAAR_ORTHO", 1), ("PNP_HAAR_MAX_LEVELS", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src) and getattr(_lib, name) == val
    assert _lib.HAAR_MODES == {"ti": 0, "ortho": 1} and _lib.PRIOR_NAMES == {0: "unet", 1: "tv", 2: "haar"}
    assert "haar" not in _lib.PRIORS                                             # pnp_set_prior does not take it
    mk = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bhaar_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_haar_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    assert re.search(r"^asan_haar:", mk, flags=re.M)
    unit = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "haar_kernels.hip")).read()
    assert "#pragma clang fp contract(off)" in unit and "fmaf" not in unit   # contraction off and no fused product anywhere
    sig = inspect.signature(engine.PnPEngine.haar_denoise).parameters
    assert (sig["levels"].default, sig["mode"].default, sig["out"].default) == (R.LEVELS, R.MODE, None) == (3, "ti", None)
    sig = inspect.signature(engine.PnPEngine.set_haar_prior).parameters
    assert (sig["scale"].default, sig["levels"].default, sig["mode"].default) == (R.SCALE, R.LEVELS, R.MODE) == (1.0, 3, "ti")
    assert callable(engine.PnPEngine.haar_settings)
    sig = inspect.signature(denoiser.HaarDenoiser2D.__init__).parameters
    assert (sig["scale"].default, sig["levels"].default, sig["mode"].default) == (1.0, 3, "ti")
    for name in ("forward", "to", "eval", "engine_for", "__call__"):
        assert callable(getattr(denoiser.HaarDenoiser2D, name)), name
    # the region the case table's seams are chosen for is the one the kernels are built with
    internal = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "pnp_internal.h")).read()
    assert re.search(r"kHaarRegion\s*=\s*%d\b" % R.REGION, internal) and re.search(r"kHaarMaxLevels\s*=\s*%d\b" % R.MAX_LEVELS, internal)
    assert [R.tile(j) for j in R.CASE_LEVELS] == [126, 122, 114, 98] and R.CASE_LEVELS == (1, 2, 3, 4)
    assert (1, 112, 128) in R.CASES and 0 < 112 - R.tile(4) < (1 << 4) - 1       # a second tile narrower than the halo


# the errors that need no handle (every one is reported before the handle is looked at, and before any HIP call)
def _denoise(lib, a):
    return lib.pnp_haar_denoise(a["h"], a["x"], a["lam"], a["levels"], a["mode"], a["out"], None)


@pytest.mark.parametrize("key,val,what", [("h", None, b"null handle"), ("x", None, b"null x_in"), ("lam", None, b"null lam"),
                                          ("out", None, b"null out"), ("levels", 0, b"levels"), ("levels", 5, b"levels"), ("levels", -3, b"levels"),
                                          ("mode", 2, b"mode"), ("mode", -1, b"mode")])
def test_haar_denoise_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    buf, x = (C.c_float * 4)(), (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                      # never dereferenced: every case fails validation first
    a = dict(h=None, x=C.cast(x, C.c_void_p).value, lam=C.cast(x, C.c_void_p).value, levels=3, mode=0, out=p)
    a[key] = val
    assert _denoise(lib, a) == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert list(buf) == [0.0] * 4


@pytest.mark.parametrize("scale,levels,mode,what", [(-0.5, 3, 0, b"haar_scale"), (math.nan, 3, 0, b"haar_scale"), (math.inf, 3, 0, b"haar_scale"),
                                                    (1.0, 0, 0, b"levels"), (1.0, 5, 0, b"levels"), (1.0, 3, 2, b"mode"), (1.0, 3, -1, b"mode"),
                                                    (1.0, 3, 0, b"null handle"), (0.0, 4, 1, b"null handle")])
def test_set_prior_haar_argument_errors_are_reported_without_a_gpu(scale, levels, mode, what):
    lib = _lib.load()
    assert lib.pnp_set_prior_haar(None, scale, levels, mode) == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()


def test_get_prior_haar_argument_errors_are_reported_without_a_gpu_and_set_prior_still_refuses_code_2():
    lib = _lib.load()
    sc, lv, md = C.c_double(7.0), C.c_int(7), C.c_int(7)
    assert lib.pnp_get_prior_haar(None, C.byref(sc), C.byref(lv), C.byref(md)) == -1 and b"null handle" in lib.pnp_last_error()
    for args in ((None, C.byref(lv), C.byref(md)), (C.byref(sc), None, C.byref(md)), (C.byref(sc), C.byref(lv), None)):
        assert lib.pnp_get_prior_haar(None, *args) == -1 and b"null pointer" in lib.pnp_last_error()
    assert (sc.value, lv.value, md.value) == (7.0, 7, 7)
    assert lib.pnp_set_prior(None, _lib.PNP_PRIOR_HAAR, 1.0, 20) == -1 and b"prior must be" in lib.pnp_last_error()


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    call = lambda expr, what, code: (
        "    if (%s != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"%s\")) return %d;\n" % (expr, what, code))
    src = tmp_path / "haar_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include <math.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float x[4] = {0};\n"
        "    float v[4] = {0};\n"
        "    int lv = 7, md = 7;\n"
        "    double sc = 7.0;\n"
        "    if (PNP_PRIOR_HAAR != 2 || PNP_HAAR_TI != 0 || PNP_HAAR_ORTHO != 1 || PNP_HAAR_MAX_LEVELS != 4) return 1;\n"
        + call("pnp_haar_denoise(0, x, x, 3, PNP_HAAR_TI, v, 0)", "null handle", 2)
        + call("pnp_haar_denoise(0, 0, x, 3, PNP_HAAR_TI, v, 0)", "null x_in", 3)
        + call("pnp_haar_denoise(0, x, 0, 3, PNP_HAAR_TI, v, 0)", "null lam", 4)
        + call("pnp_haar_denoise(0, x, x, 3, PNP_HAAR_ORTHO, 0, 0)", "null out", 5)
        + call("pnp_haar_denoise(0, x, x, 0, PNP_HAAR_TI, v, 0)", "levels", 6)
        + call("pnp_haar_denoise(0, x, x, PNP_HAAR_MAX_LEVELS + 1, PNP_HAAR_TI, v, 0)", "levels", 7)
        + call("pnp_haar_denoise(0, x, x, 3, 2, v, 0)", "mode", 8)
        + call("pnp_set_prior_haar(0, -1.0, 3, PNP_HAAR_TI)", "haar_scale", 9)
        + call("pnp_set_prior_haar(0, (double)NAN, 3, PNP_HAAR_TI)", "haar_scale", 10)
        + call("pnp_set_prior_haar(0, 1.0, 0, PNP_HAAR_TI)", "levels", 11)
        + call("pnp_set_prior_haar(0, 1.0, 5, PNP_HAAR_TI)", "levels", 12)
        + call("pnp_set_prior_haar(0, 1.0, 3, 7)", "mode", 13)
        + call("pnp_set_prior_haar(0, 1.0, 3, PNP_HAAR_ORTHO)", "null handle", 14)
        + call("pnp_get_prior_haar(0, &sc, &lv, &md)", "null handle", 15)
        + call("pnp_get_prior_haar(0, 0, &lv, &md)", "null pointer", 16)
        + call("pnp_set_prior(0, PNP_PRIOR_HAAR, 1.0, 20)", "prior must be", 17) +
        "    if (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f || lv != 7 || md != 7 || sc != 7.0) return 18;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "haar_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_haar_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "haar_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur, lds = None, None                                                    # (the keys of a kernel come in alphabetical order: its LDS size before its name)
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|vgpr_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "group_segment_fixed_size":
                lds = int(m.group(2))
            elif m.group(1) == "name":
                cur = m.group(2) if "haar_" in m.group(2) and "_kernel" in m.group(2) else None
                if cur:
                    assert "tv_" not in cur                                      # test_tv_host.py counts the kernels whose names hold it
                    meta[cur] = {"group_segment_fixed_size": lds}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    for k, count in KERNELS.items():
        assert sum(k in name for name in meta) == count, k                       # the plane variant and the (z, u) variant of each (and level count)
    for name, m in meta.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        fused = re.search(r"haar_ti_fused_kernelILi(\d)E", name)
        if fused:
            assert m["group_segment_fixed_size"] == FUSED_LDS[int(fused.group(1))] <= 160 * 1024, (name, m)
            assert m["vgpr_count"] <= 128, (name, m)                             # 1024 threads: the cap
        if "haar_ortho_kernel" in name:
            assert m["group_segment_fixed_size"] == 8 * 1024, (name, m)


# ---- the reference checks itself -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,levels", [(16, 16, 4), (32, 48, 3), (80, 16, 2), (16, 32, 1)])
def test_ti_is_the_mean_over_all_shifts_of_the_decimated_transform(h, w, levels):
    rng = np.random.default_rng(h + w + levels)
    v = rng.random((h, w)) * 1.3 - 0.15
    for lam in (0.03, 0.2):
        d = float(np.abs(R.haar(v[None], [lam], levels, "ti", clamp=False)[0] - R.shift_average(v, lam, levels)).max())
        print(f"{h} x {w}, J = {levels}, lam {lam}: max |cascade - shift average| = {d:.2e}")
        assert d <= 1e-12


def test_unclamped_ortho_minimises_its_objective():
    rng = np.random.default_rng(11)
    for levels, lam in ((1, 0.05), (3, 0.1), (4, 0.3)):
        v = rng.random((32, 48))
        x = R.haar(v[None], [lam], levels, "ortho", clamp=False)[0]
        o = R.objective(x, v, lam, levels)
        assert o <= R.objective(v, v, lam, levels)
        for eps in (1e-1, 1e-3, 1e-5):
            for _ in range(8):
                assert R.objective(x + eps * rng.standard_normal(x.shape), v, lam, levels) >= o


def test_lam_zero_is_the_clamp_and_a_constant_image_is_a_fixed_point():
    v, _ = R.case_input(3)
    for f32 in (False, True):
        for mode in R.MODES:
            for levels in R.CASE_LEVELS:
                assert np.array_equal(R.haar(v, np.zeros(3), levels, mode, f32), np.clip(v.astype(np.float64), 0, 1))
                for c in (0.0, 0.3, 1.0, 1.7, -0.2):
                    const = np.full((1, 16, 48), c, dtype=np.float32)
                    for lam in (1e-6, 0.05, 10.0):
                        assert np.array_equal(R.haar(const, [lam], levels, mode, f32), np.clip(const.astype(np.float64), 0, 1))


def test_a_threshold_above_every_detail_gives_the_block_mean_in_ortho():
    v, _ = R.case_input(3)
    v = np.clip(v.astype(np.float64), 0, 1)
    n, h, w = v.shape
    for levels in R.CASE_LEVELS:
        b = 1 << levels
        mean = v.reshape(n, h // b, b, w // b, b).mean(axis=(2, 4), keepdims=True)
        want = np.broadcast_to(mean, (n, h // b, b, w // b, b)).reshape(n, h, w)
        assert np.abs(R.haar(v, np.full(n, 100.0), levels, "ortho") - want).max() <= 1e-14


def test_ti_commutes_with_every_circular_shift_and_ortho_with_shifts_by_block_multiples():
    v, lam = R.case_input(3)
    for f32 in (False, True):
        for levels in (1, 3, 4):
            a = R.haar(v, lam, levels, "ti", f32)
            for s in ((1, 0), (0, 7), (15, 15), (33, 70)):
                assert np.array_equal(R.haar(np.roll(v, s, axis=(1, 2)), lam, levels, "ti", f32), np.roll(a, s, axis=(1, 2))), (levels, s)
            a = R.haar(v, lam, levels, "ortho", f32)
            b = 1 << levels
            for s in ((b, 0), (0, 3 * b), (2 * b, b)):
                assert np.array_equal(R.haar(np.roll(v, s, axis=(1, 2)), lam, levels, "ortho", f32), np.roll(a, s, axis=(1, 2))), (levels, s)
            assert not np.array_equal(R.haar(np.roll(v, 1, axis=2), lam, levels, "ortho", f32), np.roll(a, 1, axis=2))


def test_fixture_the_reference_haar_admm_ends_at_least_3_db_above_x0():
    d = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    assert len(sig) == 30 and abs(float(sig[0]) - 50 / 255) < 1e-7 and abs(float(sig[-1]) - 5 / 255) < 1e-7
    _, p0, p1 = R.admm_haar(d, mu, sig)
    print(f"Haar-ADMM fixture: PSNR of x0 {p0[0]:.3f} dB, of the final x {p1[0]:.3f} dB (gain {p1[0] - p0[0]:.3f} dB)")
    assert p1[0] - p0[0] >= 3.0
    k = R.FIXTURE["compare_iters"]
    mu, sig = R.fixture_schedules(k)
    x64, _, q64 = R.admm_haar(d, mu, sig)
    x32, _, q32 = R.admm_haar(d, mu, sig, f32=True)
    dp, dx = float(np.abs(q64 - q32).max()), float(np.abs(x64 - x32).max())
    print(f"float32 restatement of the first {k} iterations: |dPSNR| {dp:.3e} dB, max |dx| {dx:.3e} (haar_ref.ADMM_F32 = {R.ADMM_F32})")
    # the transform of the restatement is a library's float32 FFT: the recorded pair bounds it with a factor of two to spare for another build
    assert dp <= 2 * R.ADMM_F32[0] and dx <= 2 * R.ADMM_F32[1]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_the_float32_restatement_against_float64_is_the_recorded_table(i, mode):
    assert set(R.F32_ERR) == set(R.MODES)
    assert len(R.CASES) == len(R.F32_ERR[mode]) == len(R.CASE_LAMS) and all(len(r) == len(R.CASE_LEVELS) for r in R.F32_ERR[mode])
    v, lam = R.case_input(i)
    assert v.shape == R.CASES[i] and lam.shape == (R.CASES[i][0],)
    assert v[0].min() < 0 and v[0].max() > 1                                    # one slice extends below 0 and above 1
    assert set(l for row in R.CASE_LAMS for l in row) == set(R.LAMS)
    for j, k in enumerate(R.CASE_LEVELS):
        e = float(np.abs(R.case_ref(i, k, mode, True) - R.case_ref(i, k, mode)).max())
        print(f"case {i} {R.CASES[i]} lam {lam.tolist()} {mode} J {k}: max |f32 - f64| = {e:.3e} (recorded {R.F32_ERR[mode][i][j]:.3e})")
        assert abs(e - R.F32_ERR[mode][i][j]) <= 2e-3 * R.F32_ERR[mode][i][j]


# ---- Python and CLI surfaces -----------------------------------------------------------------------------------------------------------

def test_cli_takes_prior_haar_refuses_bad_values_and_builds_no_unet(monkeypatch):
    base = ["--block_size", "18", "--n_embeds", "9"]
    with pytest.raises(SystemExit, match="--haar-levels"):
        cli.main(base + ["--prior", "haar", "--haar-levels", "0", "eval"])
    with pytest.raises(SystemExit, match="--haar-levels"):
        cli.main(base + ["--prior", "haar", "--haar-levels", "5", "fixed"])
    with pytest.raises(SystemExit, match="--haar-scale"):
        cli.main(base + ["--prior", "haar", "--haar-scale", "-1", "mcts"])
    with pytest.raises(SystemExit, match="--haar-scale"):
        cli.main(base + ["--prior", "haar", "--haar-scale", "nan", "flex"])
    with pytest.raises(SystemExit, match="--haar-mode"):
        cli.main(base + ["--prior", "haar", "--haar-mode", "db4", "eval"])
    with pytest.raises(SystemExit, match="--denoiser-ckpt"):
        cli.main(base + ["--prior", "haar", "--denoiser-ckpt", "x.pt", "eval"])
    with pytest.raises(SystemExit, match="--prior haar"):
        cli.main(base + ["--prior", "haar", "acquire", "--out", "nowhere"])

    def no_unet(*_a, **_k):
        raise AssertionError("--prior haar must not build a U-Net")
    monkeypatch.setattr(denoiser.UNetDenoiser2D, "__init__", no_unet)
    monkeypatch.setattr(denoiser.UNetDenoiser2D, "seeded", classmethod(no_unet))
    den = cli._denoiser(argparse.Namespace(prior="haar", haar_scale=0.5, haar_levels=2, haar_mode="ortho", denoiser_ckpt=None, seed=0))
    assert isinstance(den, denoiser.HaarDenoiser2D) and (den.scale, den.levels, den.mode) == (0.5, 2, "ortho")
    assert den.to("cuda") is den and den.eval() is den and den.bf16_convs is False

    class Parsed(Exception):
        pass
    seen = []

    def grab(args):
        seen.append((args.prior, args.haar_scale, args.haar_levels, args.haar_mode))
        raise Parsed
    monkeypatch.setattr(cli, "_denoiser", grab)
    for mode in ("eval", "flex", "mcts", "fixed"):
        with pytest.raises(Parsed):
            cli.main(base + ["--prior", "haar", "--haar-scale", "0.25", "--haar-levels", "4", "--haar-mode", "ortho", mode])
    with pytest.raises(Parsed):
        cli.main(base + ["--prior", "haar", "fixed"])
    with pytest.raises(Parsed):                                                  # the Haar flags are read under --prior haar only
        cli.main(base + ["--prior", "tv", "--haar-levels", "9", "--haar-mode", "db4", "fixed"])
    assert seen == [("haar", 0.25, 4, "ortho")] * 4 + [("haar", 1.0, 3, "ti"), ("tv", 1.0, 9, "db4")]


def test_haar_denoiser_validates_its_arguments():
    with pytest.raises(ValueError, match="levels"):
        denoiser.HaarDenoiser2D(levels=0)
    with pytest.raises(ValueError, match="levels"):
        denoiser.HaarDenoiser2D(levels=5)
    with pytest.raises(ValueError, match="scale"):
        denoiser.HaarDenoiser2D(scale=-0.1)
    with pytest.raises(ValueError, match="scale"):
        denoiser.HaarDenoiser2D(scale=math.inf)
    with pytest.raises(ValueError, match="mode"):
        denoiser.HaarDenoiser2D(mode="db4")
    den = denoiser.HaarDenoiser2D(0.0, 4, "ortho")
    assert (den.scale, den.levels, den.mode) == (0.0, 4, "ortho")
    import torch
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        den(torch.zeros((2, 16, 16)), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        den(torch.zeros((2, 1, 16, 16)), torch.zeros(2))
