"""CPU-only checks of the coil map estimate (pnp_estimate_sens): the entry point is declared, exported and bound; every argument error is
reported without a GPU, from ctypes and from a C99 program, with the output buffer untouched; the built code objects of the coilmap_*
kernels have no scratch, no spills and no flagged packed-FP32 operand; the float64 restatement the GPU tests compare against
(tests/coilmap_ref.py) checks itself; `acquisition.acs_block` meets its specification; the CLI refuses --sens estimate without --coils.

Quality figure of the reference (test_reference_quality_on_a_noisy_problem): the rms over coils and pixels of |S_est - S_true| on
{kept and gt > 0.1}, 1 x 256 x 256, 8 coils, sigma_n = 10/255, fully sampled, block 24 x 24, Hann, thresh 0.05, measured on the CPU:
1.165e-2 (seed 11) and 1.223e-2 (seed 12); asserted <= 3e-2."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coilmap_ref as R  # noqa: E402

from dt4image_restoration_amd import _lib, acquisition, cli, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("coilmap_window_kernel", "coilmap_rss_kernel", "coilmap_max_kernel", "coilmap_normalise_kernel")


def test_entry_point_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    lib = _lib.load()
    m = re.search(r"\bint\s+pnp_estimate_sens\s*\(([^)]*)\)", src)
    assert m is not None
    assert len([p for p in m.group(1).split(",") if p.strip()]) == 11
    assert hasattr(lib, "pnp_estimate_sens") and len(_lib.SIGNATURES["pnp_estimate_sens"][1]) == 11
    assert re.search(r"#define\s+PNP_SENS_BOX\s+0\b", src) and re.search(r"#define\s+PNP_SENS_HANN\s+1\b", src)
    assert (_lib.PNP_SENS_BOX, _lib.PNP_SENS_HANN) == (0, 1)
    mk = open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bcoilmap_kernels\.o\b", mk, flags=re.M)                 # asan / stamps / diag build it too
    assert re.search(r"^CXXFLAGS_coilmap_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)   # compiled like the mixed-radix unit
    # pnp_config and the multi-coil entry points keep their shapes
    assert [f[0] for f in _lib.pnp_config._fields_] == ["n", "h", "w", "device", "flags"]
    assert len(_lib.SIGNATURES["pnp_reset_mc"][1]) == 13 and len(_lib.SIGNATURES["pnp_acquire_mc"][1]) == 14
    for name, nargs in (("pnp_reset_mc", 13), ("pnp_acquire_mc", 14)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert len([p for p in m.group(1).split(",") if p.strip()]) == nargs, name


# the errors that need no handle (every one is reported before the handle is looked at, and before any HIP call)
CASES = [("h", None, b"null handle"), ("y0", None, b"null y0"), ("sens", None, b"null sens"),
         ("coils", 0, b"coils"), ("coils", 33, b"coils"), ("coils", -1, b"coils"),
         ("acs_h", 3, b"acs_h"), ("acs_h", 0, b"acs_h"), ("acs_h", -2, b"acs_h"), ("acs_w", 5, b"acs_w"), ("acs_w", 1, b"acs_w"),
         ("window", 2, b"window"), ("window", -1, b"window"),
         ("thresh", -0.01, b"thresh"), ("thresh", 1.0, b"thresh"), ("thresh", math.nan, b"thresh"), ("thresh", math.inf, b"thresh"),
         ("flags", 1, b"flags")]


@pytest.mark.parametrize("key,val,what", CASES)
def test_argument_errors_are_reported_without_a_gpu(key, val, what):
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                      # never dereferenced: every case fails validation first
    y = (C.c_float * 4)()
    a = dict(h=None, y0=C.cast(y, C.c_void_p).value, coils=4, acs_h=8, acs_w=8, window=1, thresh=0.05, flags=0, sens=p)
    a[key] = val
    rc = lib.pnp_estimate_sens(a["h"], a["y0"], a["coils"], a["acs_h"], a["acs_w"], a["window"], a["thresh"], a["flags"], a["sens"], p, None)
    assert rc == -1
    assert what in lib.pnp_last_error(), lib.pnp_last_error()
    assert list(buf) == [0.0] * 4


def test_aliased_input_and_output_are_refused():
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value
    assert lib.pnp_estimate_sens(None, p, 4, 8, 8, 1, 0.05, 0, p, None, None) == -1 and b"alias" in lib.pnp_last_error()


def test_header_compiles_as_c99_and_the_errors_come_back_from_c(tmp_path):
    call = lambda args, what, code: (
        "    if (pnp_estimate_sens(%s) != PNP_ERR_INVALID || !strstr(pnp_last_error(), \"%s\")) return %d;\n" % (args, what, code))
    src = tmp_path / "coilmap_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include <math.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float y[4] = {0};\n"
        "    float v[4] = {0};\n"
        "    if (PNP_SENS_BOX != 0 || PNP_SENS_HANN != 1) return 1;\n"
        + call("0, y, 4, 8, 8, PNP_SENS_HANN, 0.05, 0, v, v, 0", "null handle", 2)
        + call("0, 0, 4, 8, 8, PNP_SENS_HANN, 0.05, 0, v, v, 0", "null y0", 3)
        + call("0, y, 4, 8, 8, PNP_SENS_HANN, 0.05, 0, 0, v, 0", "null sens", 4)
        + call("0, y, 0, 8, 8, PNP_SENS_HANN, 0.05, 0, v, v, 0", "coils", 5)
        + call("0, y, PNP_MC_MAX_COILS + 1, 8, 8, PNP_SENS_HANN, 0.05, 0, v, v, 0", "coils", 6)
        + call("0, y, 4, 7, 8, PNP_SENS_HANN, 0.05, 0, v, v, 0", "acs_h", 7)
        + call("0, y, 4, 8, 0, PNP_SENS_HANN, 0.05, 0, v, v, 0", "acs_w", 8)
        + call("0, y, 4, 8, 8, 2, 0.05, 0, v, v, 0", "window", 9)
        + call("0, y, 4, 8, 8, PNP_SENS_BOX, -0.5, 0, v, v, 0", "thresh", 10)
        + call("0, y, 4, 8, 8, PNP_SENS_BOX, 1.0, 0, v, v, 0", "thresh", 11)
        + call("0, y, 4, 8, 8, PNP_SENS_BOX, (double)NAN, 0, v, v, 0", "thresh", 12)
        + call("0, y, 4, 8, 8, PNP_SENS_BOX, 0.0, 4, v, v, 0", "flags", 13)
        + call("0, y, 4, 8, 8, PNP_SENS_BOX, 0.0, 0, y, 0, 0", "alias", 14) +
        "    if (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f || v[3] != 0.f) return 15;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "coilmap_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_coilmap_kernels_have_no_scratch_spills_or_flagged_packed_ops():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") and os.path.exists(_lib.LIB_PATH)
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "coilmap_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "coilmap_" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "coilmap_" in name:
                rows[name] = (n_pk, n_lohi, flagged)
    for k in KERNELS:
        assert any(k in name for name in meta), k
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi, flagged) in rows.items():
        assert n_lohi == 0 and not flagged, name


# ---- the reference checks itself -------------------------------------------------------------------------------------------------

def _clean_kspace(n, c, h, w, seed):
    gt = np.stack([synthetic.phantom(h, w, seed + i) for i in range(n)])
    sens = synthetic.coil_maps(c, h, w)
    return gt, sens, synthetic.fft2c_np(sens[None] * gt[:, None])


@pytest.mark.parametrize("n,c,h,w", [(2, 4, 64, 64), (1, 8, 32, 80)])
def test_full_plane_box_window_recovers_the_maps_of_a_noise_free_acquisition(n, c, h, w):
    gt, sens, y = _clean_kspace(n, c, h, w, 21)
    maps, rss, kept, smax = R.estimate(y, (h, w), "box", 0.0)
    on = gt > 0
    assert on.any() and (~on).any()
    err = np.abs(maps - sens[None])[np.broadcast_to(on[:, None], maps.shape)].max()
    power = (np.abs(maps) ** 2).sum(axis=1)
    print(f"max |S - coil_maps| on gt > 0: {err:.3e}; max |sum |S|^2 - 1| on the kept set: {np.abs(power[kept] - 1).max():.3e}")
    assert err <= 1e-12                                        # l_c = S_c gt, rss = gt: the unit-RSS maps themselves
    assert np.abs(power[kept] - 1).max() <= 1e-14 and not power[~kept].any()
    assert np.abs(rss - gt)[on].max() <= 1e-12
    # with a threshold the kept set is a level set of rss, and the maps vanish exactly off it
    maps_t, _, kept_t, _ = R.estimate(y, (h, w), "box", 0.2)
    assert np.array_equal(kept_t, rss > np.float64(np.float32(0.2)) * smax[:, None, None]) and 0 < kept_t.mean() < kept.mean() + 1e-12
    assert not maps_t[np.broadcast_to(~kept_t[:, None], maps_t.shape)].any()
    assert np.array_equal(maps_t[np.broadcast_to(kept_t[:, None], maps_t.shape)], maps[np.broadcast_to(kept_t[:, None], maps.shape)])


def test_hann_window_vanishes_on_the_lower_edge_and_is_one_at_the_centre():
    for (h, w, ah, aw) in ((64, 64, 24, 24), (32, 80, 16, 6), (16, 16, 2, 2), (128, 160, 24, 160)):
        win = R.window(h, w, ah, aw, "hann")
        box = R.window(h, w, ah, aw, "box")
        assert win[h // 2, w // 2] == 1.0
        assert not win[h // 2 - ah // 2, :].any() and not win[:, w // 2 - aw // 2].any()      # cos(-pi) = -1 exactly
        assert box.sum() == ah * aw and set(np.unique(box)) <= {0.0, 1.0}
        assert not win[box == 0].any() and (win >= 0).all() and (win <= 1).all()
        inner = win[h // 2 - ah // 2 + 1:h // 2 + ah // 2, w // 2 - aw // 2 + 1:w // 2 + aw // 2]
        assert (inner > 0).all()
        assert np.array_equal(win, win.astype(np.float32).astype(np.float64))                  # float32 values
        assert np.array_equal(inner, inner[::-1, ::-1])                                        # symmetric about the centre bin
    for bad in ((3, 4), (4, 0), (66, 4), (4, 66)):
        with pytest.raises(ValueError):
            R.window(64, 64, bad[0], bad[1], "hann")


@pytest.mark.parametrize("seed", [11, 12])
def test_reference_quality_on_a_noisy_problem(seed):
    h = w = 256
    d = synthetic.make_problem_mc(1, h, w, 8, sigma_n=10.0 / 255.0, seed=seed, mask=np.ones((h, w), dtype=bool))
    y = (d["y0"][..., 0] + 1j * d["y0"][..., 1]).astype(np.complex64)
    maps, rss, kept, _ = R.estimate(y, (24, 24), "hann", 0.05)
    sel = kept[0] & (d["gt"][0, 0] > 0.1)
    rms = float(np.sqrt((np.abs(maps[0] - synthetic.coil_maps(8, h, w)) ** 2)[:, sel].mean()))
    print(f"seed {seed}: rms map error on kept and gt > 0.1 ({sel.mean():.3f} of the slice): {rms:.3e}")
    assert sel.mean() > 0.2
    assert rms <= 3e-2


def test_float32_restatement_follows_the_float64_one():
    for i in range(len(R.CASES)):
        n, c, h, w, acs, kind, thresh = R.CASES[i]
        y, ref = R.case_ref(i)
        m, r, _, _ = R.estimate_f32(y, acs, kind, thresh)
        f = R.compare(m, r, ref, thresh)
        print(R.CASES[i], f)
        assert f["finite"] and f["off_zero"] and f["flips"] == 0 and f["near"] <= 1e-4
        assert f["rss"] <= 1e-6 and f["maps"] <= 1e-5 and f["unit"] <= 1e-6


# ---- acs_block --------------------------------------------------------------------------------------------------------------------

def test_acs_block_of_a_cartesian_mask_is_full_height_by_the_centred_column_run():
    m = acquisition.cartesian_mask(64, 64, 4)
    cols = m.all(axis=0)
    right = next(i for i in range(33) if i == 32 or not cols[32 + i])
    left = next(i for i in range(33) if i == 32 or not cols[31 - i])
    assert min(left, right) >= 1
    assert acquisition.acs_block(m) == (64, 2 * min(left, right)) == R.acs_block_spec(m)
    assert acquisition.acs_block(m.T.copy()) == (2 * min(left, right), 64) == R.acs_block_spec(m.T)
    assert acquisition.acs_block(np.ones((16, 32), dtype=bool)) == (16, 32)
    for h, w, accel, seed in ((64, 80, 8, 0), (128, 128, 4, 3), (32, 160, 2, 1)):
        m = acquisition.cartesian_mask(h, w, accel, seed=seed)
        assert acquisition.acs_block(m) == R.acs_block_spec(m)


@pytest.mark.parametrize("h,w,accel", [(64, 64, 4), (128, 160, 8), (80, 32, 4)])
def test_acs_block_of_a_radial_mask_is_the_largest_sampled_square(h, w, accel):
    m = synthetic.radial_mask(h, w, accel)
    a, b = acquisition.acs_block(m)
    assert a == b and a >= 2 and a % 2 == 0 and (a, b) == R.acs_block_spec(m)
    assert R.block_sampled(m, a, a) and not R.block_sampled(m, a + 2, a + 2)


def test_acs_block_raises_without_a_sampled_centre_and_intersects_per_slice_masks():
    m = synthetic.radial_mask(64, 64, 4)
    hole = m.copy()
    hole[32, 32] = False
    with pytest.raises(ValueError):
        acquisition.acs_block(hole)
    with pytest.raises(ValueError):
        R.acs_block_spec(hole)
    with pytest.raises(ValueError):
        acquisition.acs_block(np.zeros((16, 16), dtype=bool))
    a = acquisition.cartesian_mask(64, 64, 4, center_fraction=0.2)
    b = acquisition.cartesian_mask(64, 64, 4, center_fraction=0.1, seed=5)
    both = np.stack([a, b])
    want = R.acs_block_spec(a & b)
    assert acquisition.acs_block(both) == want == R.acs_block_spec(both)
    assert want[1] <= min(acquisition.acs_block(a)[1], acquisition.acs_block(b)[1])
    assert acquisition.acs_block(np.stack([a, m])) == R.acs_block_spec(a & m)                 # columns and lines: a square


def test_cli_refuses_sens_estimate_without_coils_and_bad_options():
    base = ["--block_size", "18", "--n_embeds", "9"]
    with pytest.raises(SystemExit, match="--sens estimate needs --coils"):
        cli.main(base + ["--sens", "estimate", "eval"])
    with pytest.raises(SystemExit, match="--sens-thresh"):
        cli.main(base + ["--coils", "4", "--sens", "estimate", "--sens-thresh", "1.0", "eval"])
    with pytest.raises(SystemExit, match="--acs"):
        cli.main(base + ["--coils", "4", "--sens", "estimate", "--acs", "3", "4", "eval"])
