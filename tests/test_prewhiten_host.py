"""CPU-only checks of the coil noise pre-whitening (pnp_noise_cov, pnp_whiten_matrix, pnp_whiten_apply): the three entry points are
declared, exported and bound; every argument error that needs no GPU is reported with its message, from ctypes and from a C99 program, with
the output buffers untouched; the built code objects of the prewhiten_* kernels have no scratch and no spills; the float64 restatement the
GPU tests compare against (tests/prewhiten_ref.py) checks itself; `synthetic.noise_cov_model` is positive definite for every parameter the
command line accepts; the fixture of the reconstruction check gains what tests/test_gpu_prewhiten.py records; the stand-alone sanitizer
program (tests/asan_prewhiten_host.cpp, `make asan_pw`) passes.

Figures of the reference, measured on the CPU (prewhiten_ref.FIXTURE): 26.304 dB with pre-whitening, 24.505 dB without, a gain of 1.799 dB."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prewhiten_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, cli, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
KERNELS = ("prewhiten_cov_kernel", "prewhiten_cov_sum_kernel", "prewhiten_chol_kernel", "prewhiten_apply_kernel")
APPLY_BUCKETS = 8                                            # C rounded up to a multiple of 8


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",") if p.strip()])


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("pnp_noise_cov", 8), ("pnp_whiten_matrix", 9), ("pnp_whiten_apply", 7)):
        assert _nargs(src, name) == nargs
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"#define\s+PNP_PW_MAX_COILS\s+64\b", src) and _lib.PNP_PW_MAX_COILS == 64 == R.MAX_COILS
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bprewhiten_kernels\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_prewhiten_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    unit = open(os.path.join(CSRC, "prewhiten_kernels.hip")).read()
    assert "atomic" not in unit.lower().replace("no atomics", "")
    for fn in ("noise_cov", "whiten_matrix", "whiten_apply"):
        assert callable(getattr(engine.PnPEngine, fn))
    assert inspect.signature(engine.PnPEngine.whiten_apply).parameters["out"].default is None
    sig = inspect.signature(acquisition.prewhiten).parameters
    assert list(sig) == ["engine_or_env", "y0", "noise", "sens", "inplace"] and sig["inplace"].default is True and sig["sens"].default is None
    assert list(inspect.signature(acquisition.noise_scan).parameters) == ["engine_or_env", "coils", "samples", "noise_cov", "sigma_n", "seed"]
    assert "noise_cov" in inspect.signature(acquisition.simulate).parameters
    assert list(inspect.signature(synthetic.noise_cov_model).parameters) == ["c", "rho", "gains", "seed"]


def _bufs():
    bufs = {k: (C.c_float * 4)() for k in ("noise", "wmat", "lmat")}
    bufs["psi"] = (C.c_double * 4)()
    bufs["info"] = (C.c_int32 * 4)()
    bufs["planes"] = (C.c_float * 8192)()                    # in and out 16 KiB apart: no overlap for any handle at 4 coils of 16 x 16
    ptr = {k: C.cast(v, C.c_void_p).value for k, v in bufs.items()}            # never dereferenced: every case fails validation first
    ptr["in"], ptr["out"] = ptr["planes"], ptr["planes"] + 16384
    return bufs, ptr


def _untouched(bufs):
    return not any(any(v) for v in bufs.values())


COV_CASES = [("h", None, b"null handle"), ("noise", None, b"null noise"), ("psi", None, b"null psi"), ("coils", 0, b"coils"),
             ("coils", 65, b"coils"), ("coils", -1, b"coils"), ("samples", 0, b"samples"), ("samples", -5, b"samples"),
             ("noise_n", 0, b"noise_n"), ("noise_n", 65536, b"noise_n"), ("flags", 1, b"flags"), ("flags", -1, b"flags")]


@pytest.mark.parametrize("key,val,what", COV_CASES)
def test_noise_cov_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    bufs, p = _bufs()
    a = dict(h=None, noise=p["noise"], noise_n=1, coils=2, samples=1, flags=0, psi=p["psi"])
    a[key] = val
    assert lib.pnp_noise_cov(a["h"], a["noise"], a["noise_n"], a["coils"], a["samples"], a["flags"], a["psi"], None) == -1
    assert what in lib.pnp_last_error() and b"pnp_noise_cov" in lib.pnp_last_error(), lib.pnp_last_error()
    assert _untouched(bufs)


MATRIX_CASES = [("h", None, b"null handle"), ("psi", None, b"null psi"), ("wmat", None, b"null wmat"), ("info", None, b"null info"),
                ("coils", 0, b"coils"), ("coils", 65, b"coils"), ("psi_n", 0, b"psi_n"), ("psi_n", 65536, b"psi_n"), ("flags", 2, b"flags")]


@pytest.mark.parametrize("key,val,what", MATRIX_CASES)
def test_whiten_matrix_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    bufs, p = _bufs()
    a = dict(h=None, psi=p["psi"], psi_n=1, coils=1, flags=0, wmat=p["wmat"], lmat=p["lmat"], info=p["info"])
    a[key] = val
    assert lib.pnp_whiten_matrix(a["h"], a["psi"], a["psi_n"], a["coils"], a["flags"], a["wmat"], a["lmat"], a["info"], None) == -1
    assert what in lib.pnp_last_error() and b"pnp_whiten_matrix" in lib.pnp_last_error(), lib.pnp_last_error()
    assert _untouched(bufs)


APPLY_CASES = [("h", None, b"null handle"), ("in", None, b"null in"), ("wmat", None, b"null wmat"), ("out", None, b"null out"),
               ("coils", 0, b"coils"), ("coils", 65, b"coils"), ("wmat_n", 0, b"wmat_n"), ("wmat_n", -1, b"wmat_n")]


@pytest.mark.parametrize("key,val,what", APPLY_CASES)
def test_whiten_apply_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    bufs, p = _bufs()
    a = {"h": None, "in": p["in"], "coils": 4, "wmat": p["wmat"], "wmat_n": 1, "out": p["out"]}
    a[key] = val
    assert lib.pnp_whiten_apply(a["h"], a["in"], a["coils"], a["wmat"], a["wmat_n"], a["out"], None) == -1
    assert what in lib.pnp_last_error() and b"pnp_whiten_apply" in lib.pnp_last_error(), lib.pnp_last_error()
    assert _untouched(bufs)


def test_forbidden_aliasing_is_refused_and_in_place_is_not():
    lib = _lib.load()
    bufs, p = _bufs()
    big = (C.c_float * 8192)()
    b = C.cast(big, C.c_void_p).value
    # partial overlap of in and out: any offset below the planes of the smallest handle (16 x 16) is refused before the handle is looked at
    for off in (8, 2040, 2048 * 4 - 8):
        assert lib.pnp_whiten_apply(None, b, 4, p["wmat"], 1, b + off, None) == -1 and b"overlap" in lib.pnp_last_error()
        assert lib.pnp_whiten_apply(None, b + off, 4, p["wmat"], 1, b, None) == -1 and b"overlap" in lib.pnp_last_error()
    assert lib.pnp_whiten_apply(None, b, 4, p["wmat"], 1, b, None) == -1 and b"null handle" in lib.pnp_last_error()      # exactly in place
    assert lib.pnp_whiten_apply(None, b, 4, p["wmat"], 1, b + 2048 * 4, None) == -1 and b"null handle" in lib.pnp_last_error()
    assert lib.pnp_whiten_apply(None, p["in"], 4, p["out"], 1, p["out"], None) == -1 and b"alias" in lib.pnp_last_error()
    assert lib.pnp_whiten_apply(None, p["in"], 4, p["in"], 1, p["out"], None) == -1 and b"alias" in lib.pnp_last_error()
    assert lib.pnp_noise_cov(None, p["noise"], 1, 2, 1, 0, p["noise"], None) == -1 and b"alias" in lib.pnp_last_error()
    for args in ((p["psi"], p["psi"], p["lmat"], p["info"]), (p["psi"], p["wmat"], p["wmat"], p["info"]),
                 (p["psi"], p["wmat"], p["lmat"], p["wmat"]), (p["psi"], p["wmat"], p["info"], p["info"])):
        assert lib.pnp_whiten_matrix(None, args[0], 1, 1, 0, args[1], args[2], args[3], None) == -1 and b"alias" in lib.pnp_last_error()
    assert lib.pnp_whiten_matrix(None, p["psi"], 1, 1, 0, p["wmat"], None, p["info"], None) == -1 and b"null handle" in lib.pnp_last_error()
    assert _untouched(bufs) and not any(big)


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    call = lambda fn, args, what, code: (
        "    if (%s(%s) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"%s\")) return %d;\n" % (fn, args, what, code))
    n, m, a = "pnp_noise_cov", "pnp_whiten_matrix", "pnp_whiten_apply"
    src = tmp_path / "prewhiten_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    static float x[8192] = {0}, w[4] = {0}, l[4] = {0};\n"
        "    float* o = x + 4096;\n"
        "    double p[4] = {0};\n"
        "    int32_t f[4] = {0};\n"
        "    if (PNP_PW_MAX_COILS != 64) return 1;\n"
        + call(n, "0, x, 1, 2, 8, 0, p, 0", "null handle", 2)
        + call(n, "0, 0, 1, 2, 8, 0, p, 0", "null noise", 3)
        + call(n, "0, x, 1, 2, 8, 0, 0, 0", "null psi", 4)
        + call(n, "0, x, 1, 0, 8, 0, p, 0", "coils", 5)
        + call(n, "0, x, 1, PNP_PW_MAX_COILS + 1, 8, 0, p, 0", "coils", 6)
        + call(n, "0, x, 1, 2, 0, 0, p, 0", "samples", 7)
        + call(n, "0, x, 0, 2, 8, 0, p, 0", "noise_n", 8)
        + call(n, "0, x, 65536, 2, 8, 0, p, 0", "noise_n", 9)
        + call(n, "0, x, 1, 2, 8, 4, p, 0", "flags", 10)
        + call(m, "0, p, 1, 2, 0, w, l, f, 0", "null handle", 11)
        + call(m, "0, p, 1, 2, 0, w, 0, f, 0", "null handle", 12)
        + call(m, "0, 0, 1, 2, 0, w, l, f, 0", "null psi", 13)
        + call(m, "0, p, 1, 2, 0, 0, l, f, 0", "null wmat", 14)
        + call(m, "0, p, 1, 2, 0, w, l, 0, 0", "null info", 15)
        + call(m, "0, p, 1, 65, 0, w, l, f, 0", "coils", 16)
        + call(m, "0, p, 0, 2, 0, w, l, f, 0", "psi_n", 17)
        + call(m, "0, p, 1, 2, 1, w, l, f, 0", "flags", 18)
        + call(m, "0, p, 1, 2, 0, w, w, f, 0", "alias", 19)
        + call(a, "0, x, 2, w, 1, o, 0", "null handle", 20)
        + call(a, "0, x, 2, w, 1, x, 0", "null handle", 21)
        + call(a, "0, 0, 2, w, 1, o, 0", "null in", 22)
        + call(a, "0, x, 2, 0, 1, o, 0", "null wmat", 23)
        + call(a, "0, x, 2, w, 1, 0, 0", "null out", 24)
        + call(a, "0, x, 0, w, 1, o, 0", "coils", 25)
        + call(a, "0, x, 65, w, 1, o, 0", "coils", 26)
        + call(a, "0, x, 2, w, 0, o, 0", "wmat_n", 27)
        + call(a, "0, x, 2, w, 1, x + 2, 0", "overlap", 28)
        + call(a, "0, x, 2, o, 1, o, 0", "alias", 29)
        + call(a, "0, x, 2, w, 1, o - 1, 0", "null handle", 31) +
        "    for (int i = 0; i < 4; ++i) if (w[i] != 0.f || l[i] != 0.f || o[i] != 0.f || x[i] != 0.f || p[i] != 0.0 || f[i] != 0) return 30;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "prewhiten_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_prewhiten_kernels_have_no_scratch_and_no_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "prewhiten_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":                               # (the three fields sort after .name within a kernel's entry)
                cur = m.group(2) if "prewhiten_" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    for k in KERNELS:
        assert any(k in name for name in meta), k
    assert sum("prewhiten_apply_kernel" in name for name in meta) == APPLY_BUCKETS
    assert len(meta) == 3 + APPLY_BUCKETS
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)


# ---- the reference checks itself -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.COV_COILS)
def test_the_factorisation_whitens_and_inverts_in_float64(c):
    psi = R.case_psi(c)
    cond = float(np.linalg.cond(psi))
    W, L, info = R.factor(psi)
    eye = np.eye(c)
    f = dict(cond=cond, whiten=float(np.abs(W @ psi @ W.conj().T - eye).max()), inverse=float(np.abs(L @ W - eye).max()),
             chol=float(np.abs(L - np.linalg.cholesky(psi)).max() / np.abs(L).max()))
    print(c, R.MATRIX_PARAMS[c], f)
    assert info == 0 and cond <= 1e4 and (c < 32 or cond >= 1e3)                # the cases reach a condition number of 1e3 .. 1e4
    assert f["whiten"] <= cond * c * 2.0 ** -52 and f["inverse"] <= cond * c * 2.0 ** -52 and f["chol"] <= cond * c * 2.0 ** -52
    assert not np.triu(W, 1).any() and not np.triu(L, 1).any() and not np.diagonal(L).imag.any()
    assert np.array_equal(R.factor(np.stack([psi, psi]))[0][1], W)


def test_the_factorisation_flags_what_is_not_positive_definite_and_reads_the_lower_triangle_only():
    psi = R.case_psi(8)
    bad = psi.copy()
    bad[5, 5] = -1.0
    W, L, info = R.factor_one(bad)
    assert info == 6 and np.array_equal(W, np.eye(8)) and np.array_equal(L, np.eye(8))
    assert R.factor_one(np.zeros((3, 3)))[2] == 1
    nan = psi.copy()
    nan[3, 1] = np.nan
    assert R.factor_one(nan)[2] > 0 and np.isfinite(R.factor_one(nan)[0]).all()
    junk = psi.copy()
    junk[np.triu_indices(8, 1)] = 1e30
    junk[np.arange(8), np.arange(8)] += 5j
    assert np.array_equal(R.factor_one(junk)[0], R.factor_one(psi)[0])
    W, L, info = R.factor_one(np.eye(5))
    assert info == 0 and np.array_equal(R.rounded(W), np.eye(5, dtype=np.complex64)) and np.array_equal(R.rounded(L), np.eye(5, dtype=np.complex64))


def test_the_covariance_is_hermitian_and_its_bound_is_the_summation_bound():
    x = R.case_noise(2, 5, 1024)
    p = R.cov(x)
    assert np.array_equal(p, p.conj().transpose(0, 2, 1)) and not p[:, np.arange(5), np.arange(5)].imag.any()
    assert np.allclose(p[1], x[1].astype(np.complex128) @ x[1].astype(np.complex128).conj().T / 1024, rtol=1e-13, atol=0)
    assert (R.cov_bound(x) >= (1 - 1e-12) * 4 * 1024 * 2.0 ** -53 * np.abs(p)).all()          # Cauchy-Schwarz; equality on the diagonal
    assert [R.chunk_samples(s) for s in (1, 1024, 5000, 65536, 65537, 10 ** 6)] == [1024, 1024, 1024, 1024, 1056, 15648]
    assert R.workspace_bytes(2, 8, 5000) == 16 * 2 * 64 * 5


@pytest.mark.parametrize("i", range(len(R.APPLY_CASES)))
def test_the_float32_apply_against_float64(i):
    x, wm = R.case_planes(i)
    n, c, h, w = R.APPLY_CASES[i]
    assert x.shape == (n, c, h, w) and wm.shape == (n, c, c) and not np.triu(wm, 1).any()
    ref = R.apply(wm, x)
    e = float(np.abs(R.apply_f32(wm, x) - ref).max())
    print(R.APPLY_CASES[i], f"max |f32 - f64| = {e:.3e}")
    assert 0 < e <= 4 * c * 2.0 ** -24 * float(np.abs(ref).max())
    assert not ref.reshape(n, c, -1)[:, :, 5].any()
    junk = wm.copy()
    junk[:, np.triu_indices(c, 1)[0], np.triu_indices(c, 1)[1]] = np.nan
    assert np.array_equal(R.apply(junk, x), ref)


# ---- the model, the fixture and the command line ---------------------------------------------------------------------------------------

def test_noise_cov_model_is_hermitian_positive_definite_for_what_the_command_line_accepts():
    for c in (1, 2, 8, 32, 64):
        for rho in (0.0, 0.4, 0.9, 0.99):
            for spread in (1.0, 3.0, 100.0):
                for seed in (0, 7):
                    p = synthetic.noise_cov_model(c, rho, spread, seed)
                    assert p.dtype == np.complex128 and np.array_equal(p, p.conj().T) and not np.diagonal(p).imag.any()
                    assert np.linalg.eigvalsh(p).min() > 0 and R.factor_one(p)[2] == 0, (c, rho, spread, seed)
    p = synthetic.noise_cov_model(4, 0.5, [1.0, 2.0, 0.5, 3.0], 1)
    assert np.allclose(np.diagonal(p).real, [1.0, 4.0, 0.25, 9.0]) and abs(abs(p[1, 0]) - 1.0) < 1e-15 and abs(abs(p[3, 0]) - 3 * 0.125) < 1e-15
    for bad in (dict(c=0), dict(c=4, rho=1.0), dict(c=4, rho=-0.1), dict(c=4, gains=0.5), dict(c=4, gains=[1.0, 2.0]), dict(c=4, gains=[1, 1, 0, 1])):
        with pytest.raises(ValueError):
            synthetic.noise_cov_model(**bad)
    assert abs(acquisition.unit_scan_sigma(p) ** 2 * 2 * np.diagonal(p).real.mean() - 1) < 1e-14 and abs(acquisition.unit_scan_sigma() - 0.5 ** 0.5) < 1e-15


def test_fixture_pre_whitening_gains_what_the_gpu_test_records():
    xw, pw, _ = R.pipeline(True)
    xr, pr, _ = R.pipeline(False)
    gain = float((pw - pr)[0])
    print(f"reference pipeline: {pw[0]:.3f} dB with pre-whitening, {pr[0]:.3f} dB without, gain {gain:.3f} dB")
    assert gain >= 0.5 and abs(gain - 1.799) <= 2e-3
    x32, p32, _ = R.pipeline(True, True)
    dp, dx = float(np.abs(p32 - pw).max()), float(np.abs(x32 - xw).max())
    print(f"float32 restatement of the whitened pipeline: |dPSNR| {dp:.3e} dB, max |dx| {dx:.3e}")
    # the transform of the restatement is a library's float32 FFT: the recorded pair bounds it with a factor of two to spare for another build
    assert dp <= 2 * 8.508e-07 and dx <= 2 * 2.598e-06
    d = R.fixture()
    W = R.factor_one(R.cov(d["scan"]))[0]
    assert abs(np.real(np.diagonal(R.cov(d["scan"]))).mean() - 1.0) < 0.05           # the scan's level keeps the data's scale


def test_cli_takes_noise_cov_and_prewhiten_and_refuses_bad_values(monkeypatch):
    base = ["--block_size", "18", "--n_embeds", "9"]
    for bad in ("1.0", "-0.1", "0.4,0.5", "a", "0.4,2,3", "0.4,inf"):
        with pytest.raises(SystemExit, match="--noise-cov"):
            cli.main(base + ["--coils", "8", "--noise-cov", bad, "fixed"])
    with pytest.raises(SystemExit, match="--noise-cov needs --coils"):
        cli.main(base + ["--noise-cov", "0.4", "eval"])
    with pytest.raises(SystemExit, match="--prewhiten needs --coils"):
        cli.main(base + ["--prewhiten", "flex"])
    with pytest.raises(SystemExit, match="--prewhiten applies to"):
        cli.main(base + ["--coils", "8", "--prewhiten", "acquire", "--gt", "x", "--out", "y"])

    class Parsed(Exception):
        pass
    seen = []

    def grab(args):
        seen.append((args.noise_cov, args.prewhiten))
        raise Parsed
    monkeypatch.setattr(cli, "_denoiser", grab)
    for mode in ("eval", "flex", "mcts", "fixed"):
        with pytest.raises(Parsed):
            cli.main(base + ["--coils", "8", "--noise-cov", "0.4,3", "--prewhiten", mode])
    with pytest.raises(Parsed):
        cli.main(base + ["--coils", "8", "--noise-cov", "0.25", "fixed"])
    assert seen == [((0.4, 3.0), True)] * 4 + [((0.25, 1.0), False)]


def test_the_sanitizer_program_of_the_argument_validation_passes():
    """`make asan_pw`: the instrumented host build of the library (host code only) and tests/asan_prewhiten_host.cpp, a program with its own
    main, run directly."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "asan_pw"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "_asan", "asan_prewhiten_host")], capture_output=True, text=True)
    assert r.returncode == 0 and "asan_prewhiten_host: ok" in r.stdout, r.stdout + r.stderr
