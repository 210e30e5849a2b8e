"""CPU-only checks of the simulated acquisition (pnp_acquire and acquisition.py): the entry point is exported, declared and bound
and rejects bad arguments before any HIP call; the built acquire kernels are free of scratch, spills and low-reads-high packed-f32
ops; `cartesian_mask` counts, centre block, determinism and seed sensitivity for both kinds; the task parser; `data.load_gt_dir`
round trip, ranges and refusals; the `acquire` sub-command's file names parse back to their tasks."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dt4image_restoration_amd import _lib, acquisition, cli, data as D, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pnp_acquire_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pnp_acquire\s*\(([^)]*)\)", src)
    assert m is not None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11 and "double sigma_n" in params and "uint64_t seed" in params and params[-1] == "void* stream"
    lib = _lib.load()
    assert hasattr(lib, "pnp_acquire") and "pnp_acquire" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pnp_acquire"]
    assert res is C.c_int and len(args) == 11 and args[4] is C.c_double and args[5] is C.c_uint64
    assert "acquire_kernels.o" in open(os.path.join(ROOT, "dt4image_restoration_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("case,what", [("flags", b"flags"), ("neg", b"sigma_n"), ("nan", b"sigma_n"), ("inf", b"sigma_n"),
                                       ("gt", b"null gt"), ("mask", b"null mask"), ("y0", b"null y0"), ("handle", b"null handle")])
def test_pnp_acquire_rejects_bad_arguments_without_a_gpu(case, what):
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                      # never dereferenced: every case fails validation first
    a = dict(gt=p, mask=p, sigma=0.04, flags=0, y0=p)
    if case == "flags":
        a["flags"] = 1
    elif case in ("neg", "nan", "inf"):
        a["sigma"] = {"neg": -0.01, "nan": math.nan, "inf": math.inf}[case]
    elif case != "handle":
        a[case] = None
    rc = lib.pnp_acquire(None, a["gt"], a["mask"], 1, a["sigma"], 5, a["flags"], a["y0"], p, p, None)
    assert rc == -1
    assert what in lib.pnp_last_error()
    assert list(buf) == [0.0] * 4


def _acquire_code_object_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no llvm tools / library")
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "acquire_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "acquire" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "acquire" in name:
                rows[name] = (n_pk, n_lohi, flagged)
    return meta, rows


def test_acquire_kernels_have_no_scratch_spills_or_low_reads_high_ops():
    meta, rows = _acquire_code_object_kernels()
    assert any("acquire_epilogue_kernel" in k for k in meta) and any("acquire_clamp_kernel" in k for k in meta)
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi, flagged) in rows.items():
        assert n_lohi == 0 and not flagged, name


# ---- cartesian_mask ---------------------------------------------------------------------------------------------------------

WIDTHS, ACCELS = (16, 320, 1024), (2, 4, 8)


@pytest.mark.parametrize("kind", ["random", "equispaced"])
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("w", WIDTHS)
def test_cartesian_mask_counts_centre_block_and_columns(w, accel, kind):
    h = 32
    m = acquisition.cartesian_mask(h, w, accel, seed=3, kind=kind)
    assert m.shape == (h, w) and m.dtype == np.bool_
    assert bool((m == m[:1]).all())                        # constant along H: whole columns
    cols = m[0]
    nc = int(round(w * 0.08))
    lo = (w - nc) // 2
    assert bool(cols[lo:lo + nc].all())                    # the centred block is always sampled
    assert abs((lo + (nc - 1) / 2) - (w - 1) / 2) <= 0.5   # ... and centred to within half a column
    if kind == "random":
        assert int(cols.sum()) == math.ceil(w / accel)
    else:
        assert cols.sum() / w >= 1 / accel
        # gaps between consecutive sampled outer columns on either side of the centre block (the pair straddling it left out)
        idx = np.flatnonzero(cols)
        gaps = np.concatenate([np.diff(idx[idx < lo]), np.diff(idx[idx >= lo + nc])])
        if len(gaps):
            assert int(gaps.max()) - int(gaps.min()) <= 1, gaps
    # deterministic
    assert np.array_equal(m, acquisition.cartesian_mask(h, w, accel, seed=3, kind=kind))
    # other sizes along H give the same columns
    assert np.array_equal(acquisition.cartesian_mask(16, w, accel, seed=3, kind=kind)[0], cols)


@pytest.mark.parametrize("w", (320, 1024))
def test_cartesian_mask_random_columns_follow_the_seed_and_the_hash(w):
    from dt4image_restoration_amd.weights import hash_uniform
    a = acquisition.cartesian_mask(16, w, 4, seed=0)
    b = acquisition.cartesian_mask(16, w, 4, seed=1)
    assert not np.array_equal(a, b) and a.sum() == b.sum()
    # the outer columns are those with the smallest keys of hash_uniform(seed, 9101, w)
    nc = int(round(w * 0.08))
    lo = (w - nc) // 2
    outer = np.array([c for c in range(w) if not lo <= c < lo + nc])
    keys = hash_uniform(0, 9101, w)[outer]
    k = math.ceil(w / 4) - nc
    chosen = outer[a[0][outer]]
    assert len(chosen) == k
    assert keys[a[0][outer]].max() <= np.sort(keys)[k - 1]
    # equispaced ignores the seed
    assert np.array_equal(acquisition.cartesian_mask(16, w, 4, seed=0, kind="equispaced"),
                          acquisition.cartesian_mask(16, w, 4, seed=9, kind="equispaced"))


def test_cartesian_mask_refuses_bad_arguments_and_radial_mask_is_unchanged():
    with pytest.raises(ValueError, match="kind"):
        acquisition.cartesian_mask(16, 16, 4, kind="spiral")
    with pytest.raises(ValueError, match="accel"):
        acquisition.cartesian_mask(16, 16, 0.5)
    with pytest.raises(ValueError, match="mask kind"):
        acquisition.make_mask(16, 16, 4, kind="spiral")
    assert np.array_equal(acquisition.make_mask(64, 64, 4, "radial"), synthetic.radial_mask(64, 64, 4))
    assert np.array_equal(acquisition.make_mask(64, 64, 4, "cartesian", seed=2), acquisition.cartesian_mask(64, 64, 4, seed=2))


# ---- tasks --------------------------------------------------------------------------------------------------------------------

def test_task_parser_accepts_all_optimal_tasks():
    for t in D.OPTIMAL_TASKS:
        accel, sigma_n = acquisition.parse_task(t)
        a, s = t.split("x_")
        assert accel == int(a) and sigma_n == int(s) / 255.0
        # the same parse as data.task_from_filename: a file named after the pair reads back as the task
        assert D.task_from_filename(f"img_{accel}_{int(s)}_.mat") == t
    for bad in ("4_10", "x_10", "4x", "4x_", "rtg_3", ""):
        with pytest.raises(ValueError):
            acquisition.parse_task(bad)


@pytest.mark.parametrize("image", ["brain", "file1000123-0007", "12_34", "7", "a_1_2_b"])
def test_acquired_file_names_parse_back_to_their_tasks(image):
    for t in D.OPTIMAL_TASKS:
        fn = cli.acquired_name(t, image)
        a, s = t.split("x_")
        assert fn.endswith(".mat") and f"_{a}_{s}_" in fn and image in fn
        assert D.task_from_filename(os.path.join("/some/12_7/dir", fn)) == t


def test_simulate_refuses_to_run_without_a_gpu_instead_of_falling_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="GPU"):
        acquisition.simulate(object(), np.zeros((1, 16, 16), np.float32), np.ones((16, 16), bool), 0.0, 0)


# ---- load_gt_dir ----------------------------------------------------------------------------------------------------------------

def _gt_folder(tmp_path):
    from scipy.io import savemat
    rng = np.random.default_rng(4)
    imgs = rng.random((6, 32, 48)).astype(np.float32)
    np.save(tmp_path / "a_single.npy", imgs[0])                       # [H,W]
    np.save(tmp_path / "b_stack.npy", imgs[1:4].astype(np.float64))   # [n,H,W], another float type
    savemat(str(tmp_path / "c_one.mat"), {"gt": imgs[4][None]})       # [1,H,W] as the reference stores it
    savemat(str(tmp_path / "d_flat.mat"), {"gt": imgs[5]})            # [H,W]
    (tmp_path / "notes.txt").write_text("ignored")
    return imgs


def test_load_gt_dir_round_trip_ranges_and_names(tmp_path):
    imgs = _gt_folder(tmp_path)
    gt, names = D.load_gt_dir(str(tmp_path))
    assert gt.shape == (6, 1, 32, 48) and gt.dtype == np.float32
    assert np.array_equal(gt[:, 0], imgs)
    assert names == ["a_single", "b_stack-0000", "b_stack-0001", "b_stack-0002", "c_one", "d_flat"]
    assert D.count_gt_dir(str(tmp_path)) == 6 and D.count_gt_dir(str(tmp_path), 3) == 3
    # a rank's range, cutting through the stack
    part, pn = D.load_gt_dir(str(tmp_path), start=2, stop=5)
    assert np.array_equal(part[:, 0], imgs[2:5]) and pn == names[2:5]
    # limit first, then the range
    part, pn = D.load_gt_dir(str(tmp_path), limit=3, start=1)
    assert np.array_equal(part[:, 0], imgs[1:3]) and pn == names[1:3]
    with pytest.raises(FileNotFoundError):
        D.load_gt_dir(str(tmp_path), limit=3, start=3)


def test_load_gt_dir_opens_only_the_files_of_its_range(tmp_path):
    imgs = _gt_folder(tmp_path)
    np.save(tmp_path / "e_bad.npy", np.full((32, 48), 2.0, np.float32))     # values are checked when a file is read
    part, _ = D.load_gt_dir(str(tmp_path), start=0, stop=6)
    assert np.array_equal(part[:, 0], imgs)
    assert D.count_gt_dir(str(tmp_path)) == 7
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        D.load_gt_dir(str(tmp_path), start=6, stop=7)


def test_load_gt_dir_refusals(tmp_path):
    with pytest.raises(FileNotFoundError):
        D.load_gt_dir(str(tmp_path))
    np.save(tmp_path / "a.npy", np.full((16, 16), 0.5, np.float32))
    np.save(tmp_path / "b.npy", np.full((16, 32), 0.5, np.float32))
    with pytest.raises(ValueError, match="share one size"):
        D.load_gt_dir(str(tmp_path))
    os.remove(tmp_path / "b.npy")
    for bad, what in ((np.full((16, 16), 1.5, np.float32), r"\[0, 1\]"), (np.full((16, 16), -0.1, np.float32), r"\[0, 1\]"),
                      (np.full((16, 16), np.nan, np.float32), r"\[0, 1\]"), (np.ones((16, 16), np.uint8), "float"),
                      (np.zeros((2, 1, 16, 16), np.float32), "expected")):
        np.save(tmp_path / "b.npy", bad)
        with pytest.raises(ValueError, match=what):
            D.load_gt_dir(str(tmp_path))
    os.remove(tmp_path / "b.npy")
    from scipy.io import savemat
    savemat(str(tmp_path / "c.mat"), {"x0": np.zeros((16, 16), np.float32)})
    with pytest.raises(KeyError, match="gt"):
        D.load_gt_dir(str(tmp_path))


def test_cli_parses_the_new_options_and_keeps_the_old_defaults():
    ap_err = pytest.raises(SystemExit)
    with ap_err:
        cli.main(["--block_size", "18", "--n_embeds", "9", "--mask", "spiral", "eval"])
    with ap_err:
        cli.main(["--block_size", "18", "--n_embeds", "9", "--acquire", "host", "eval"])
    with ap_err:
        cli.main(["--block_size", "18", "--n_embeds", "9", "acquire"])          # --out is required
    with pytest.raises(ValueError, match="task"):
        cli._tasks(type("A", (), {"tasks": "4x_10,fast"})())
    assert cli._tasks(type("A", (), {"tasks": None})()) == D.OPTIMAL_TASKS
    assert cli._tasks(type("A", (), {"tasks": "8x_15,2x_5"})()) == ["8x_15", "2x_5"]
