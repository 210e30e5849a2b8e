"""CPU-only checks of the k-space stage for sides of 2^a * 5^b: the built mixed-radix kernels (fft_mixed_kernels.hip) are free of
scratch, spills and low-reads-high packed-f32 ops, the size rule is documented where callers read it, and the G10 fixture has its
documented keys and shapes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dt4image_restoration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED_KERNELS = ("fft_rows_mixed_kernelILi0E", "fft_rows_mixed_kernelILi1E", "fft_rows_mixed_kernelILi2E",
                 "fft_cols_mixed_kernelILi0E", "fft_cols_mixed_kernelILi1E")


def _mixed_code_object_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no llvm tools / library")
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "radix5_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "_mixed_kernel" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, _flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "_mixed_kernel" in name:
                rows[name] = (n_pk, n_lohi)
    return meta, rows


def test_mixed_radix_kernels_have_no_scratch_spills_or_low_reads_high_ops():
    meta, rows = _mixed_code_object_kernels()
    for k in MIXED_KERNELS:
        assert sum(k in name for name in meta) == 1, (k, sorted(meta))
    assert len(meta) == len(MIXED_KERNELS)
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi) in rows.items():
        assert n_lohi == 0, name


def test_header_names_the_kspace_sizes():
    src = open(os.path.join(ROOT, "include", "pnpadmm.h")).read()
    assert "16, 32, 64, 80, 128, 160, 256, 320, 400, 512, 640, 800, 1024" in src
    assert "power-of-two h, w" not in src


def test_g10_fixture_keys_and_shapes(golden_dir):
    path = os.path.join(golden_dir, "g10_radix5.npz")
    assert os.path.getsize(path) < 1024 * 1024
    g = np.load(path)
    assert set(g.files) == {"iters", "psnr_320", "mu_tab_320", "sig_tab_320", "x_final_320",
                            "psnr_640x320", "mu_tab_640x320", "sig_tab_640x320", "x_sum_640x320", "x_l2_640x320"}
    it = int(g["iters"])
    assert it == 20
    assert g["psnr_320"].shape == (2, it) and g["mu_tab_320"].shape == (2, it) and g["sig_tab_320"].shape == (2, it)
    assert g["x_final_320"].shape == (2, 320, 320) and g["x_final_320"].dtype == np.float32
    assert g["psnr_640x320"].shape == (1, it) and g["mu_tab_640x320"].shape == (1, it) and g["sig_tab_640x320"].shape == (1, it)
    assert g["x_sum_640x320"].shape == (1,) and g["x_l2_640x320"].shape == (1,)
    assert np.isfinite(g["psnr_320"]).all() and np.isfinite(g["psnr_640x320"]).all()
    assert 20 < g["psnr_320"].min() and g["psnr_320"].max() < 45
    # the final image is in [0, 1] (the denoiser clamps), so its L2 norm is bounded by its sum
    assert 0 < g["x_l2_640x320"][0] <= np.sqrt(g["x_sum_640x320"][0])


def test_tables_are_the_param_table_rows():
    from dt4image_restoration_amd import synthetic
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_radix5.npz"))
    for tag, n in (("320", 2), ("640x320", 1)):
        mu, sg = synthetic.param_table(n, int(g["iters"]), seed=77)
        np.testing.assert_array_equal(g[f"mu_tab_{tag}"], mu)
        np.testing.assert_array_equal(g[f"sig_tab_{tag}"], sg)
