"""CPU-only checks of the multi-coil (SENSE) data-fidelity stage: the entry points are declared, exported and bound; every argument
error is reported without a GPU, from ctypes and from a C99 program; the built code objects of the new kernels have no scratch, no
spills and no flagged packed-FP32 operand; and the float64 restatement the GPU tests compare against (tests/sense_ref.py) checks
itself: adjointness, the closed form at C = 1 with S = 1, unit-RSS maps, a non-increasing residual history."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sense_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, cli, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"pnp_set_kspace_mc": 9, "pnp_reset_mc": 13, "pnp_mc_coils": 1, "pnp_mc_cg_residual": 3, "pnp_mc_normal": 5, "pnp_acquire_mc": 14}


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m is not None, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == nargs, name
        assert hasattr(lib, name) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert re.search(r"#define\s+PNP_MC_MAX_COILS\s+32\b", src) and re.search(r"#define\s+PNP_MC_MAX_CG\s+64\b", src)
    assert (_lib.PNP_MC_MAX_COILS, _lib.PNP_MC_MAX_CG) == (32, 64)
    mk = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bsense_kernels\.o\b", mk, flags=re.M)                 # asan / stamps / diag build it too
    assert re.search(r"^CXXFLAGS_sense_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)   # compiled like the mixed-radix unit
    assert lib.pnp_mc_coils(None) == 0
    # pnp_config and the existing entry points keep their shapes
    assert [f[0] for f in _lib.pnp_config._fields_] == ["n", "h", "w", "device", "flags"]
    assert len(_lib.SIGNATURES["pnp_reset"][1]) == 9 and len(_lib.SIGNATURES["pnp_acquire"][1]) == 11


def _call(lib, fn, a):
    p = a["p"]
    if fn == "pnp_set_kspace_mc":
        return lib.pnp_set_kspace_mc(a["h"], a["y0"], a["sens"], a["coils"], a["sens_n"], a["mask"], a["mask_n"], a["cg"], None)
    if fn == "pnp_reset_mc":
        return lib.pnp_reset_mc(a["h"], a["x0"], a["y0"], a["sens"], a["coils"], a["sens_n"], a["mask"], a["mask_n"], a["cg"], a["x"], p, p, None)
    return lib.pnp_acquire_mc(a["h"], a["gt"], a["sens"], a["coils"], a["sens_n"], a["mask"], a["mask_n"], a["sigma"], 5, a["flags"],
                              a["y0"], p, p, None)


CASES = [("coils", 0, b"coils"), ("coils", 33, b"coils"), ("coils", -1, b"coils"), ("sens_n", 0, b"sens_n"), ("mask_n", 0, b"mask_n"),
         ("sens", None, b"null sens"), ("mask", None, b"null mask"), ("y0", None, b"null y0"), ("h", None, b"null handle")]


OWN = {"pnp_set_kspace_mc": [("cg", 0, b"cg_iters"), ("cg", 65, b"cg_iters")],
       "pnp_reset_mc": [("cg", 0, b"cg_iters"), ("cg", 65, b"cg_iters"), ("x0", None, b"null x0"), ("x", None, b"null x")],
       "pnp_acquire_mc": [("gt", None, b"null gt"), ("sigma", -0.01, b"sigma_n"), ("sigma", math.nan, b"sigma_n"),
                          ("sigma", math.inf, b"sigma_n"), ("flags", 1, b"flags")]}


@pytest.mark.parametrize("fn,key,val,what", [(fn, *c) for fn in OWN for c in CASES + OWN[fn]])
def test_argument_errors_are_reported_without_a_gpu(fn, key, val, what):
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                      # never dereferenced: every case fails validation first
    a = dict(h=None, p=p, y0=p, sens=p, mask=p, x0=p, x=p, gt=p, coils=4, sens_n=1, mask_n=1, cg=8, sigma=0.04, flags=0)
    a[key] = val
    assert _call(lib, fn, a) == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert list(buf) == [0.0] * 4


def test_queries_reject_null_arguments():
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value
    assert lib.pnp_mc_cg_residual(None, p, None) == -1 and b"null" in lib.pnp_last_error()
    assert lib.pnp_mc_normal(None, p, p, p, None) == -1 and b"null" in lib.pnp_last_error()


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    src = tmp_path / "sense_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include <math.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float v[4] = {0};\n"
        "    unsigned char m[4] = {0};\n"
        "    if (PNP_MC_MAX_COILS != 32 || PNP_MC_MAX_CG != 64) return 1;\n"
        "    if (pnp_set_kspace_mc(0, v, v, 33, 1, m, 1, 8, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 2;\n"
        "    if (pnp_set_kspace_mc(0, v, v, 4, 1, m, 1, 65, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"cg_iters\")) return 3;\n"
        "    if (pnp_set_kspace_mc(0, v, v, 4, 0, m, 1, 8, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"sens_n\")) return 4;\n"
        "    if (pnp_set_kspace_mc(0, v, v, 4, 1, m, 0, 8, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"mask_n\")) return 5;\n"
        "    if (pnp_set_kspace_mc(0, v, 0, 4, 1, m, 1, 8, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null sens\")) return 6;\n"
        "    if (pnp_reset_mc(0, v, v, v, 4, 1, m, 1, 0, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"cg_iters\")) return 7;\n"
        "    if (pnp_reset_mc(0, 0, v, v, 4, 1, m, 1, 8, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null x0\")) return 8;\n"
        "    if (pnp_reset_mc(0, v, v, v, 4, 1, m, 1, 8, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 9;\n"
        "    if (pnp_acquire_mc(0, v, v, 4, 1, m, 1, -1.0, 5, 0, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"sigma_n\")) return 10;\n"
        "    if (pnp_acquire_mc(0, v, v, 4, 1, m, 1, (double)NAN, 5, 0, v, v, v, 0) != PNP_ERR_INVALID) return 11;\n"
        "    if (pnp_acquire_mc(0, v, v, 0, 1, m, 1, 0.0, 5, 0, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"coils\")) return 12;\n"
        "    if (pnp_acquire_mc(0, v, v, 4, 1, m, 1, 0.0, 5, 0, v, v, v, 0) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"null handle\")) return 13;\n"
        "    if (pnp_mc_coils(0) != 0) return 14;\n"
        "    if (pnp_mc_cg_residual(0, v, 0) != PNP_ERR_INVALID) return 15;\n"
        "    if (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f) return 16;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "sense_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_sense_kernels_have_no_scratch_spills_or_flagged_packed_ops():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "sense_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "sense_" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "sense_" in name:
                rows[name] = (n_pk, n_lohi, flagged)
    for k in ("sense_expand_kernel", "sense_mask_kernel", "sense_combine_kernel", "sense_cg_init_kernel", "sense_scalar_kernel",
              "sense_cg_update_kernel", "sense_cg_dir_kernel", "sense_dual_kernel", "sense_cgres_kernel", "sense_misfit_kernel",
              "sense_install_kernel", "sense_iterate_kernel"):
        assert any(k in name for name in meta), k
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi, flagged) in rows.items():
        assert n_lohi == 0 and not flagged, name


# ---- the reference checks itself -------------------------------------------------------------------------------------------------

def _rand(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("h,w,c,per_slice", [(64, 64, 4, False), (80, 160, 3, True), (128, 128, 8, False)])
def test_reference_operators_are_adjoint(h, w, c, per_slice):
    n = 2
    sens = synthetic.coil_maps(c, h, w)
    mask = synthetic.radial_mask(h, w, 4)
    if per_slice:
        sens = np.stack([sens, synthetic.coil_maps(c, h, w, radius=1.5)])
        mask = np.stack([mask, synthetic.radial_mask(h, w, 8)])
    p, q = _rand((n, h, w), 1), _rand((n, c, h, w), 2)
    lhs, rhs = np.vdot(q, R.A(p, sens, mask)), np.vdot(R.AH(q, sens, mask), p)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_two_cg_iterations_equal_the_closed_form_at_one_coil_with_unit_map():
    n, h, w = 2, 64, 64
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=5)
    y0 = (d["y0"][:, 0, ..., 0].astype(np.float64) + 1j * d["y0"][:, 0, ..., 1])
    x = d["gt"][:, 0].astype(np.float64)
    z = d["x0"][:, 0, ..., 0].astype(np.float64) + 1j * d["x0"][:, 0, ..., 1]
    u = 0.1 * _rand((n, h, w), 3)
    mu = np.array([0.05, 0.6])
    zc, uc = R.closed_form_single(x, z, u, y0, d["mask"], mu)
    z2, u2, res = R.prox_dual(x, z, u, y0[:, None], np.ones((1, h, w), dtype=np.complex128), d["mask"], mu, 2)
    print("max |z_cg2 - z_closed| = %.3e, cg_res = %s" % (np.abs(z2 - zc).max(), res))
    assert np.abs(z2 - zc).max() <= 1e-12 and np.abs(u2 - uc).max() <= 1e-12
    assert res.max() <= 1e-12


@pytest.mark.parametrize("c", [1, 2, 8, 15, 32])
def test_coil_maps_have_unit_rss(c):
    s = synthetic.coil_maps(c, 64, 80)
    assert s.shape == (c, 64, 80) and s.dtype == np.complex128
    assert np.abs((np.abs(s) ** 2).sum(axis=0) - 1).max() <= 1e-14
    if c == 8:
        assert abs(np.abs(synthetic.coil_maps(8, 128, 128)).min() - 0.035) < 0.002
    with pytest.raises(ValueError):
        synthetic.coil_maps(0, 16, 16)


@pytest.mark.parametrize("mu", [0.05, 0.3, 0.6])
def test_residual_history_is_non_increasing_and_frozen_slices_stay_finite(mu):
    cs = R.solve_case(64, 64, 4, True, "radial", 8)
    m = np.full(2, mu)
    z, res, hist, kept = R.cg_solve(cs["z0"], cs["x"], cs["u"], cs["aty"], cs["sens"], cs["mask"], m, 8, record=(1, 4, 8))
    assert hist.shape == (9, 2) and np.all(np.diff(hist, axis=0) <= 1e-12), hist
    assert np.array_equal(kept[8][0], z) and np.array_equal(hist[-1], res)
    # b = 0 and z0 = 0: rs = 0 from the start, alpha = beta = 0, nothing moves and nothing is NaN
    zero = np.zeros_like(cs["z0"])
    z, res, hist, _ = R.cg_solve(zero, zero.real, zero, zero, cs["sens"], cs["mask"], m, 3)
    assert np.array_equal(z, zero) and np.array_equal(res, np.zeros(2)) and np.isfinite(hist).all()
    # the float32 restatement follows the float64 one
    z64 = R.cg_solve(cs["z0"], cs["x"], cs["u"], cs["aty"], cs["sens"], cs["mask"], m, 8)[0]
    z32 = R.cg_solve_f32(cs["z0"], cs["x"], cs["u"], cs["aty"], cs["sens"], cs["mask"], m, 8)[0]
    assert R.solve_errors(z32, z64)[0] < 1e-4


def test_make_problem_mc_matches_the_reference_acquisition_and_make_problem_is_untouched():
    n, h, w, c = 2, 32, 48, 3
    d = synthetic.make_problem_mc(n, h, w, c, accel=4.0, seed=11)
    assert d["y0"].shape == (n, c, h, w, 2) and d["sens"].shape == (c, h, w) and d["sens"].dtype == np.complex64
    assert d["x0"].shape == (n, 1, h, w, 2) and d["ATy0"].shape == (n, 1, h, w, 2)
    y, aty, x0 = R.acquire(d["gt"][:, 0], synthetic.coil_maps(c, h, w), d["mask"], 10.0 / 255.0, 11)
    assert np.abs(d["y0"][..., 0] + 1j * d["y0"][..., 1] - y).max() < 1e-6
    assert np.abs(d["ATy0"][:, 0, ..., 0] + 1j * d["ATy0"][:, 0, ..., 1] - aty).max() < 1e-6
    assert np.abs(d["x0"][:, 0, ..., 0] + 1j * d["x0"][:, 0, ..., 1] - x0).max() < 1e-6
    # one coil with a unit map draws make_problem's noise: coil 0 uses the streams 9001 / 9003
    s = synthetic.make_problem(n, h, w, accel=4.0, seed=11)
    y1 = R.acquire(s["gt"][:, 0], np.ones((1, h, w)), s["mask"], 10.0 / 255.0, 11)[0]
    assert np.abs(s["y0"][:, 0, ..., 0] + 1j * s["y0"][:, 0, ..., 1] - y1[:, 0]).max() < 1e-6
    assert "sens" not in s


def test_cli_refuses_acquire_with_coils_and_bad_ranges():
    base = ["--block_size", "18", "--n_embeds", "9"]
    with pytest.raises(SystemExit, match="no coil axis"):
        cli.main(base + ["--coils", "4", "acquire", "--gt", "/nonexistent", "--out", "/nonexistent"])
    with pytest.raises(SystemExit, match="--coils"):
        cli.main(base + ["--coils", "33", "eval"])
    with pytest.raises(SystemExit, match="--cg-iters"):
        cli.main(base + ["--coils", "4", "--cg-iters", "0", "eval"])
