"""CPU-only checks of the coil compression (pnp_coil_compress_matrix, pnp_coil_compress_apply): both entry points are declared, exported
and bound; every argument error is reported without a GPU, from ctypes and from a C99 program, with the output buffers untouched; the
built code objects of the coilcomp_* kernels have no scratch, no spills and no flagged packed-FP32 operand; the float64 restatement the
GPU tests compare against (tests/coilcomp_ref.py) checks itself - eigh and the restated Jacobi solver against each other, and the
rank-3 construction; `acquisition.compress_coils` / `coils_for_energy` handle their arguments; the CLI refuses --compress without --coils."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coilcomp_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, cli, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("coilcomp_gram_kernel", "coilcomp_gram_sum_kernel", "coilcomp_eig_kernel", "coilcomp_apply_kernel")


def _nargs(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("pnp_coil_compress_matrix", 10), ("pnp_coil_compress_apply", 8)):
        assert _nargs(src, name) == nargs
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"#define\s+PNP_CC_MAX_COILS\s+64\b", src) and _lib.PNP_CC_MAX_COILS == 64 == R.MAX_COILS
    mk = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bcoilcomp_kernels\.o\b", mk, flags=re.M)                 # asan / stamps / diag build it too
    assert re.search(r"^CXXFLAGS_coilcomp_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)   # compiled like the SENSE and coil-map units
    internal = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "pnp_internal.h")).read()
    for fn in ("launch_coilcomp_gram", "launch_coilcomp_eig", "launch_coilcomp_apply"):
        assert fn in internal
    # the entry points this one stands beside keep their shapes
    assert len(_lib.SIGNATURES["pnp_estimate_sens"][1]) == 11 == _nargs(src, "pnp_estimate_sens")
    assert re.search(r"#define\s+PNP_MC_MAX_COILS\s+32\b", src)


def _bufs():
    bufs = {k: (C.c_float * 4)() for k in ("y0", "cmat", "eig", "out")}
    gram = (C.c_double * 4)()
    ptr = {k: C.cast(v, C.c_void_p).value for k, v in bufs.items()}     # never dereferenced: every case fails validation first
    ptr["gram"] = C.cast(gram, C.c_void_p).value
    return bufs, gram, ptr


def _untouched(bufs, gram):
    return all(list(v) == [0.0] * 4 for v in bufs.values()) and list(gram) == [0.0] * 4


MATRIX_CASES = [("h", None, b"null handle"), ("y0", None, b"null y0"), ("cmat", None, b"null cmat"), ("eig", None, b"null eig"),
                ("coils", 0, b"coils"), ("coils", 65, b"coils"), ("coils", -1, b"coils"),
                ("acs_h", 3, b"acs_h"), ("acs_h", 0, b"acs_h"), ("acs_h", -2, b"acs_h"), ("acs_w", 5, b"acs_w"), ("acs_w", 1, b"acs_w"),
                ("flags", 1, b"flags"), ("flags", -1, b"flags")]


@pytest.mark.parametrize("key,val,what", MATRIX_CASES)
def test_matrix_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    bufs, gram, p = _bufs()
    a = dict(h=None, y0=p["y0"], coils=4, acs_h=8, acs_w=8, flags=0, cmat=p["cmat"], eig=p["eig"], gram=p["gram"])
    a[key] = val
    rc = lib.pnp_coil_compress_matrix(a["h"], a["y0"], a["coils"], a["acs_h"], a["acs_w"], a["flags"], a["cmat"], a["eig"], a["gram"], None)
    assert rc == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert _untouched(bufs, gram)


APPLY_CASES = [("h", None, b"null handle"), ("in", None, b"null in"), ("cmat", None, b"null cmat"), ("out", None, b"null out"),
               ("coils", 0, b"coils"), ("coils", 65, b"coils"),
               ("out_coils", 0, b"out_coils"), ("out_coils", 5, b"out_coils"), ("out_coils", 33, b"out_coils"),
               ("cmat_n", 0, b"cmat_n"), ("cmat_n", -1, b"cmat_n")]


@pytest.mark.parametrize("key,val,what", APPLY_CASES)
def test_apply_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    bufs, gram, p = _bufs()
    a = {"h": None, "in": p["y0"], "coils": 64 if (key, val) == ("out_coils", 33) else 4, "cmat": p["cmat"], "cmat_n": 1, "out_coils": 2,
         "out": p["out"]}
    a[key] = val
    rc = lib.pnp_coil_compress_apply(a["h"], a["in"], a["coils"], a["cmat"], a["cmat_n"], a["out_coils"], a["out"], None)
    assert rc == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert _untouched(bufs, gram)


def test_aliased_buffers_are_refused():
    lib = _lib.load()
    bufs, gram, p = _bufs()
    assert lib.pnp_coil_compress_apply(None, p["y0"], 4, p["cmat"], 1, 2, p["y0"], None) == -1 and b"alias" in lib.pnp_last_error()     # out == in
    assert lib.pnp_coil_compress_apply(None, p["y0"], 4, p["cmat"], 1, 2, p["cmat"], None) == -1 and b"alias" in lib.pnp_last_error()   # out == cmat
    assert lib.pnp_coil_compress_matrix(None, p["y0"], 4, 8, 8, 0, p["y0"], p["eig"], None, None) == -1 and b"alias" in lib.pnp_last_error()
    assert lib.pnp_coil_compress_matrix(None, p["y0"], 4, 8, 8, 0, p["cmat"], p["cmat"], None, None) == -1 and b"alias" in lib.pnp_last_error()
    assert _untouched(bufs, gram)


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    call = lambda fn, args, what, code: (
        "    if (%s(%s) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"%s\")) return %d;\n" % (fn, args, what, code))
    m, a = "pnp_coil_compress_matrix", "pnp_coil_compress_apply"
    src = tmp_path / "coilcomp_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float y[4] = {0}, c[4] = {0}, e[4] = {0}, o[4] = {0};\n"
        "    double g[4] = {0};\n"
        "    if (PNP_CC_MAX_COILS != 64) return 1;\n"
        + call(m, "0, y, 4, 8, 8, 0, c, e, g, 0", "null handle", 2)
        + call(m, "0, 0, 4, 8, 8, 0, c, e, g, 0", "null y0", 3)
        + call(m, "0, y, 4, 8, 8, 0, 0, e, g, 0", "null cmat", 4)
        + call(m, "0, y, 4, 8, 8, 0, c, 0, g, 0", "null eig", 5)
        + call(m, "0, y, 0, 8, 8, 0, c, e, g, 0", "coils", 6)
        + call(m, "0, y, PNP_CC_MAX_COILS + 1, 8, 8, 0, c, e, 0, 0", "coils", 7)
        + call(m, "0, y, 4, 7, 8, 0, c, e, g, 0", "acs_h", 8)
        + call(m, "0, y, 4, 8, 0, 0, c, e, g, 0", "acs_w", 9)
        + call(m, "0, y, 4, 8, 8, 2, c, e, g, 0", "flags", 10)
        + call(a, "0, y, 4, c, 1, 2, o, 0", "null handle", 11)
        + call(a, "0, 0, 4, c, 1, 2, o, 0", "null in", 12)
        + call(a, "0, y, 4, 0, 1, 2, o, 0", "null cmat", 13)
        + call(a, "0, y, 4, c, 1, 2, 0, 0", "null out", 14)
        + call(a, "0, y, 65, c, 1, 2, o, 0", "coils", 15)
        + call(a, "0, y, 4, c, 1, 0, o, 0", "out_coils", 16)
        + call(a, "0, y, 4, c, 1, 5, o, 0", "out_coils", 17)
        + call(a, "0, y, 64, c, 1, PNP_MC_MAX_COILS + 1, o, 0", "out_coils", 18)
        + call(a, "0, y, 4, c, 0, 2, o, 0", "cmat_n", 19)
        + call(a, "0, y, 4, c, 1, 2, y, 0", "alias", 20) +
        "    for (int i = 0; i < 4; ++i) if (c[i] != 0.f || e[i] != 0.f || o[i] != 0.f || g[i] != 0.0) return 21;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "coilcomp_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_coilcomp_kernels_have_no_scratch_spills_or_flagged_packed_ops():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "coilcomp_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":                               # (the three fields sort after .name within a kernel's entry)
                cur = m.group(2) if "coilcomp_" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "coilcomp_" in name:
                rows[name] = (n_pk, n_lohi, flagged)
    for k in KERNELS:
        assert any(k in name for name in meta), k
    assert sum("coilcomp_apply_kernel" in name for name in meta) == 3                      # the three V buckets
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi, flagged) in rows.items():
        assert n_lohi == 0 and not flagged, name


# ---- the reference checks itself -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_reference_invariants(i):
    y, g, cm, ev = R.case_ref(i)
    f = R.invariants(cm, g, ev)
    print(R.CASES[i], f)
    assert np.array_equal(g, g.conj().transpose(0, 2, 1)) and not g[:, np.arange(g.shape[1]), np.arange(g.shape[1])].imag.any()
    assert f["finite"] and f["descending"] and f["phase"]
    assert f["unit"] <= 1e-12 and f["diag"] <= 1e-12 and f["eig"] <= 1e-12


@pytest.mark.parametrize("i", [0, 1, 3, 5, 6])
def test_restated_jacobi_solver_agrees_with_eigh(i):
    y, g, cm, ev = R.case_ref(i)
    cj, ej, ran = R.jacobi(g)
    f = R.invariants(cj, g, ej)
    print(R.CASES[i], "sweeps", ran, f)
    assert max(ran) < R.SWEEPS                                   # the stop test ended it, not the cap
    assert f["finite"] and f["descending"] and f["phase"]
    assert f["unit"] <= 1e-12 and f["diag"] <= 1e-12 and f["eig"] <= 1e-12
    assert np.abs(ej - ev).max() <= 1e-12 * ev.max()


def test_jacobi_rotation_is_overflow_safe_and_zero_gives_the_identity():
    cm, ev, ran = R.jacobi(np.zeros((1, 5, 5), dtype=np.complex128))
    assert np.array_equal(cm[0], np.eye(5)) and not ev.any() and ran == [0]
    with np.errstate(over="raise", invalid="raise", divide="raise"):   # a vanishing off-diagonal entry: tau overflows, t = 0, no tau * tau
        t, cs, sg, ab, on = R.rotation([1.0, 2.0, 1.0, 1.0], [2.0, 1.0, 1.0, 1e300], [1e-310 + 1e-310j, 5e-324, 0.0, 1e-200j])
    assert np.array_equal(t, [0.0, -0.0, 0.0, 0.0]) and np.array_equal(cs, [1.0] * 4) and not sg.any() and list(on) == [True, True, False, True]
    t, cs, sg, ab, on = R.rotation([1.0, 3.0], [1.0, 1.0], [2.0j, 1e200])          # equal diagonal: t = 1; a huge beta: tau -> -0
    assert t[0] == 1.0 and abs(sg[0] - 1j / np.sqrt(2)) <= 1e-16 and t[1] == -1.0 and np.isfinite(sg).all()
    cm, ev, _ = R.jacobi(np.array([[[2.0, 1.0 - 1.0j], [1.0 + 1.0j, 3.0]]]))
    assert np.abs(ev[0] - [4.0, 1.0]).max() <= 1e-15
    cm, ev, _ = R.jacobi(np.array([[[3.0, 0.0], [0.0, 3.0]]], dtype=np.complex128))   # equal eigenvalues: the stable sort keeps the order
    assert np.array_equal(cm[0], np.eye(2))


def test_rank3_data_compresses_without_loss():
    p = R.rank3_problem()
    y, sens, gt = p["y"], p["sens"], p["gt"]
    n, c, h, w = y.shape
    g = R.gram(y.astype(np.complex64), (24, 24))
    cm, ev = R.matrix(g)
    print("eig / eig[0]:", ev / ev[:, :1])
    assert (ev[:, 3:] <= 1e-12 * ev[:, :1]).all()                # float32 input data, float64 Gram: the rank shows to 1e-12
    yc, sc = R.apply(cm, y, 3), R.apply(cm, np.broadcast_to(sens, (n, c, h, w)), 3)
    full = (sens.conj()[None] * synthetic.ifft2c_np(y)).sum(axis=1)
    comp = (sc.conj() * synthetic.ifft2c_np(yc)).sum(axis=1)
    err = np.abs(comp - full).max() / np.abs(full).max()
    print(f"A^H y of the compressed problem against the full one: {err:.3e}")
    assert err <= 1e-10
    # the leading 3 rows span the mix's column space
    q = R.rank3_mix()
    assert np.abs(R.projector(cm, 3) - (q @ q.conj().T)[None]).max() <= 1e-6


def test_apply_restatements_agree():
    y, g, cm, ev = R.case_ref(1)
    a = R.rounded(cm, ev)[0]
    for v in (1, 3, 5):
        d = np.abs(R.apply_f32(a, y, v) - R.apply(a, y, v)).max() / np.abs(y).max()
        assert d <= 1e-6, (v, d)
    eye = np.eye(5, dtype=np.complex64)
    assert np.array_equal(R.apply_f32(eye, y, 5), y) and np.array_equal(R.apply_f32(eye[[2, 0, 4, 1, 3]], y, 5), y[:, [2, 0, 4, 1, 3]])


# ---- acquisition.compress_coils ------------------------------------------------------------------------------------------------------

def test_coils_for_energy_on_a_hand_made_spectrum():
    eig = np.array([[8.0, 1.0, 0.5, 0.5], [4.0, 3.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    assert acquisition.coils_for_energy(eig[:1], 0.8) == 1       # 8 / 10 reaches 0.8 exactly
    assert acquisition.coils_for_energy(eig[:1], 0.81) == 2
    assert acquisition.coils_for_energy(eig[:1], 0.95) == 3
    assert acquisition.coils_for_energy(eig[:1], 1.0) == 4
    assert acquisition.coils_for_energy(eig[1:2], 0.65) == 2
    assert acquisition.coils_for_energy(eig[:2], 0.8) == 3       # slice 0 needs 1, slice 1 needs 3: the batch takes the maximum
    assert acquisition.coils_for_energy(eig[2:], 0.9) == 1       # no energy at all
    assert acquisition.coils_for_energy(eig, 0.8) == 3
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            acquisition.coils_for_energy(eig, bad)
    with pytest.raises(ValueError):
        acquisition.coils_for_energy(np.zeros(4), 0.5)


def test_compress_coils_argument_handling():
    y = np.zeros((1, 4, 16, 16), dtype=np.complex64)
    mask = np.ones((16, 16), dtype=bool)
    with pytest.raises(ValueError, match="exactly one"):
        acquisition.compress_coils(None, y, mask=mask)
    with pytest.raises(ValueError, match="exactly one"):
        acquisition.compress_coils(None, y, mask=mask, out_coils=2, energy=0.9)
    with pytest.raises(ValueError, match="energy"):
        acquisition.compress_coils(None, y, mask=mask, energy=1.5)
    for bad in (0, 5):
        with pytest.raises(ValueError, match="out_coils"):
            acquisition.compress_coils(None, y, mask=mask, out_coils=bad)
    with pytest.raises(ValueError, match="out_coils"):
        acquisition.compress_coils(None, np.zeros((1, 40, 16, 16), dtype=np.complex64), mask=mask, out_coils=33)
    with pytest.raises(ValueError, match="acs"):
        acquisition.compress_coils(None, y, out_coils=2)         # neither a block nor a mask
    with pytest.raises(ValueError, match="y0"):
        acquisition.compress_coils(None, np.zeros((1, 4, 16, 16, 3), dtype=np.float32), mask=mask, out_coils=2)
    with pytest.raises(ValueError, match="sens"):
        acquisition.compress_coils(None, y, mask=mask, out_coils=2, sens=np.zeros((3, 16, 16), dtype=np.complex64))
    hole = mask.copy()
    hole[8, 8] = False
    with pytest.raises(ValueError):
        acquisition.compress_coils(None, y, mask=hole, out_coils=2)


def test_cli_refuses_compress_without_coils_and_out_of_range():
    base = ["--block_size", "18", "--n_embeds", "9"]
    with pytest.raises(SystemExit, match="--compress needs --coils"):
        cli.main(base + ["--compress", "4", "eval"])
    for v in ("9", "-1"):
        with pytest.raises(SystemExit, match="--compress must be 1"):
            cli.main(base + ["--coils", "8", "--compress", v, "eval"])
    with pytest.raises(SystemExit, match="--acs"):
        cli.main(base + ["--coils", "8", "--compress", "4", "--acs", "3", "4", "eval"])
    with pytest.raises(SystemExit, match="--coils must be 1..32"):
        cli.main(base + ["--coils", "64", "--compress", "8", "eval"])
