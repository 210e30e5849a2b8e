"""CPU-only checks of the non-Cartesian stage: the entry points are declared, exported and bound; the float64 restatement the GPU tests
compare against (tests/nufft_ref.py) checks itself against the exact NDFT and the single-coil closed form; the plan builder
(csrc/nufft_plan.hip, pure host code) is compiled into a stand-alone program (tests/nufft_plan_host.cpp), plain and with
-fsanitize=address,undefined, and gives the restatement's bits; the stand-alone sanitizer program of the argument validation
(tests/asan_nufft_host.cpp, `make asan_nufft`) passes.

Model against the exact NDFT: relative l2 error on a complex Gaussian image (energy up to the image edge: the worst case), 13 golden-angle
spokes of 2 max(H, W) samples, 128-node quadrature, measured on the CPU (nufft_ref.case_image seeds); the test asserts twice each figure,
the factor covering a change of seed and quadrature:

      grid             J = 4       J = 6       J = 8
      16 -> 32         1.138e-03   1.327e-05   9.728e-08
      64 -> 80         1.224e-02   5.938e-04   3.231e-05
      32x16 -> 64x32   1.239e-03   1.237e-05   1.230e-07
      64x32 -> 80x64   8.618e-03   4.018e-04   2.371e-05

Data-fidelity model: on the Cartesian-bin trajectory of a mask (w = 1, J = 8, 16 -> 32) A^H A is the mask's projector to the model error, so
two CG iterations reproduce the closed form of pnp_prox_dual: measured max |dz| / max |z| = 1.418e-07 at mu = 0.3 (twice that is asserted).

End-to-end fixture (nufft_ref.FIXTURE: one 64 x 64 phantom, 24 golden-angle spokes, noise 5/255, density-compensated, mu 0.3, sigma_d
50/255 -> 5/255 over 20 iterations, K = 8, TV): the float64 restatement goes from 16.572 dB (x0) to 36.812 dB; spokes and mu were chosen so
that this gain is at least 1 dB (16 spokes: 15.776 -> 35.153, 32 spokes: 16.980 -> 37.728, mu 1.0 at 24 spokes: -> 37.508).

Which tests need the library: the tests of the model against the exact NDFT, of its adjointness, of the closed form, of the default grids
and of the fixture exercise tests/nufft_ref.py alone - they are the self-checks of the reference the GPU tests lean on, and pass
without the feature; the default-grid test also compares the restatement's grid and beta with the plan builder's (the stand-alone
program).  Every other test here needs the new symbols, the new source files or the new Python functions."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nufft_ref as R  # noqa: E402
import sense_ref  # noqa: E402

from dt4image_restoration_amd import _lib, engine, synthetic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dt4image_restoration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

MODEL_ERR = {0: (1.138e-03, 1.327e-05, 9.728e-08), 1: (1.224e-02, 5.938e-04, 3.231e-05), 2: (1.239e-03, 1.237e-05, 1.230e-07),
             3: (8.618e-03, 4.018e-04, 2.371e-05)}
CLOSED_FORM_ERR = 1.418e-07


def _nargs(src, name):
    m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)" % name, src)
    assert m is not None, name
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",") if p.strip()])


def test_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in (("pnp_nufft_plan", 7), ("pnp_nufft_samples", 1), ("pnp_nufft_grid", 3), ("pnp_nufft_forward", 5), ("pnp_nufft_adjoint", 6),
                        ("pnp_set_kspace_nc", 5), ("pnp_reset_nc", 9), ("pnp_nc_cg_residual", 3), ("pnp_nc_normal", 5), ("pnp_acquire_nc", 10)):
        assert _nargs(src, name) == nargs
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    assert re.search(r"#define\s+PNP_NUFFT_MAX_SAMPLES\s+\(1 << 22\)", src)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*=.*\bnufft_kernels\.o\b.*\bnufft_plan\.o\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS_nufft_kernels\s*=.*-fno-slp-vectorize", mk, flags=re.M)
    unit = open(os.path.join(CSRC, "nufft_kernels.hip")).read()
    assert "atomic" not in unit.lower().replace("no atomics", "")
    plan_src = open(os.path.join(CSRC, "nufft_plan.hip")).read() + open(os.path.join(CSRC, "nufft_plan.h")).read()
    assert "hip_runtime" not in plan_src and "pnp_internal.h" not in plan_src          # pure host code: no HIP header, no HIP call
    for name, params in (("nufft_plan", ["self", "traj", "grid", "width"]), ("nufft_forward", ["self", "img"]),
                         ("nufft_adjoint", ["self", "samples", "weights"]), ("reset_nc", ["self", "x0", "y", "w", "cg_iters"]),
                         ("set_kspace_nc", ["self", "y", "w", "episode", "cg_iters"]), ("nc_normal", ["self", "p", "mu"]),
                         ("nc_cg_residual", ["self"]), ("acquire_nc", ["self", "gt", "sigma_n", "seed", "dcf"])):
        assert list(inspect.signature(getattr(engine.PnPEngine, name)).parameters) == params, name
    sig = inspect.signature(engine.PnPEngine.nufft_plan).parameters
    assert sig["grid"].default is None and sig["width"].default == 6


def test_null_handle_calls_are_refused_from_ctypes():
    lib = _lib.load()
    t = np.zeros((4, 2))
    assert lib.pnp_nufft_plan(None, t.ctypes.data, 4, 0, 0, 6, 0) == -1 and b"null handle" in lib.pnp_last_error()
    assert lib.pnp_nufft_plan(None, t.ctypes.data, 4, 0, 0, 5, 0) == -1 and b"width" in lib.pnp_last_error()
    assert lib.pnp_nufft_samples(None) == 0


@pytest.mark.parametrize("i", range(4))
def test_model_against_the_exact_ndft(i):
    n, h, w, gh, gw, _ = R.CASES[i]
    traj, x = R.case_traj(i), R.case_image(i)
    exact = R.ndft(traj, x)
    for J, measured in zip((4, 6, 8), MODEL_ERR[i]):
        P = R.plan(h, w, gh, gw, J, traj)
        err = float(np.linalg.norm(R.forward(P, x) - exact) / np.linalg.norm(exact))
        print(f"{h}x{w} -> {gh}x{gw} J={J}: model against the exact NDFT, relative l2 {err:.3e} (recorded {measured:.3e})")
        assert err <= 2 * measured


def test_the_model_is_exactly_adjoint_and_cartesian_bins_are_fft2c_bins():
    i = 4
    n, h, w, gh, gw, J = R.CASES[i]
    traj = R.case_traj(i)
    P = R.plan(h, w, gh, gw, J, traj)
    x, y = R.case_image(i), R.case_samples(i, P["m"])
    wgt = 0.5 + np.abs(R.case_samples(i, P["m"], seed=1)[0].real)
    for wv in (None, wgt):
        lhs = np.vdot(R.forward(P, x) * (1.0 if wv is None else wv), y)
        rhs = np.vdot(x, R.adjoint(P, y, wv))
        print(f"<W A x, y> - <x, A^H W y> = {abs(lhs - rhs):.3e}")
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    d = abs(np.vdot(R.ndft(traj, x), y) - np.vdot(x, R.ndft_adjoint(traj, y, h, w)))
    assert d <= 1e-12 * abs(np.vdot(R.ndft(traj, x), y))
    mask = np.ones((h, w), dtype=bool)
    tj, (jj, ll) = R.mask_traj(mask)
    full = R.ndft(tj, x).reshape(n, h, w)
    assert np.abs(full - synthetic.fft2c_np(x)).max() <= 1e-12
    k = R.chain_lengths(P)
    assert k.sum() == P["m"] * J * J and k.max() >= 2                              # the duplicated pair alone gives chains of two


def test_two_cg_iterations_on_cartesian_bins_give_the_closed_form():
    n, h, w, J = 2, 16, 16, 8
    d = synthetic.make_problem(n, h, w, accel=4.0, seed=5)
    mask = np.asarray(d["mask"]).astype(bool).reshape(h, w)
    traj, (jj, ll) = R.mask_traj(mask)
    y0 = np.asarray(d["y0"], dtype=np.float64).reshape(n, h, w, 2)
    y0c = y0[..., 0] + 1j * y0[..., 1]
    P = R.plan(h, w, 32, 32, J, traj)
    rng = np.random.default_rng(3)
    x = rng.random((n, h, w))
    u = 0.1 * (rng.standard_normal((n, h, w)) + 1j * rng.standard_normal((n, h, w)))
    mu = np.full(n, 0.3)
    y = y0c[:, jj, ll]
    zr, ur = sense_ref.closed_form_single(x, None, u, y0c * mask, mask, mu)
    z, un, res = R.prox_dual(P, x, x + u, u, R.adjoint(P, y), mu, 2)
    err = float(np.abs(z - zr).max() / np.abs(zr).max())
    print(f"two CG iterations against the closed form: max |dz| / max |z| = {err:.3e} (recorded {CLOSED_FORM_ERR:.3e}), cg_res {res}")
    assert err <= 2 * CLOSED_FORM_ERR and float(np.abs(un - ur).max() / np.abs(zr).max()) <= 2 * CLOSED_FORM_ERR
    z8, _, res8 = R.prox_dual(P, x, x + u, u, R.adjoint(P, y), mu, 8)
    assert float(np.abs(z8 - zr).max() / np.abs(zr).max()) <= 2 * CLOSED_FORM_ERR   # more iterations stay there (no NaN from rs -> 0)
    zf, uf, resf = R.prox_dual(P, np.zeros((n, h, w)), np.zeros((n, h, w), dtype=complex), np.zeros((n, h, w), dtype=complex),
                               np.zeros((n, h, w), dtype=complex), mu, 3)
    assert not zf.any() and not uf.any() and not resf.any()                         # the frozen case


def _build(workdir, sanitize):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = os.path.join(workdir, "nufft_plan_host" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-std=c++17", "--offload-arch=gfx950"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "tests", "nufft_plan_host.cpp"), os.path.join(CSRC, "nufft_plan.hip"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def plan_tools(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("nufft_plan_host"))
    return _build(d, False), _build(d, True)


def test_plan_builder_refuses_every_invalid_argument(plan_tools):
    for exe in plan_tools:
        r = subprocess.run([exe, "--invalid"], capture_output=True, text=True)
        assert r.returncode == 0 and "nufft_plan_host: invalid ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_plan_builder_gives_the_restatements_bits_and_complete_ascending_bins(plan_tools, i):
    n, h, w, gh, gw, J = R.CASES[i]
    traj = R.case_traj(i)
    P = R.plan(h, w, gh, gw, J, traj)
    text = f"{h} {w} {gh} {gw} {J} {len(traj)}\n" + "".join(f"{float(a).hex()} {float(b).hex()}\n" for a, b in traj)
    outs = []
    for exe in plan_tools:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and "nufft_plan_host: bins ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert lines[0] == f"grid {gh} {gw}"
    rows = [l.split() for l in lines[1:1 + len(traj)]]
    i0 = np.array([[int(f[1]), int(f[2])] for f in rows]).T
    wts = np.array([[int(v, 16) for v in f[3:]] for f in rows], dtype=np.uint32).T
    cy = np.array([int(v, 16) for v in lines[1 + len(traj)].split()[1:]], dtype=np.uint32)
    cx = np.array([int(v, 16) for v in lines[2 + len(traj)].split()[1:]], dtype=np.uint32)
    dw = int((wts != P["wts"].view(np.uint32)).sum())
    dc = int((cy != P["cy"].view(np.uint32)).sum() + (cx != P["cx"].view(np.uint32)).sum())
    print(f"case {i}: {len(traj)} samples, weight words differing {dw}, factor words differing {dc}, wrapped footprints "
          f"{int(((i0 < 0) | (i0 + J > np.array([[gh], [gw]]))).any(axis=0).sum())}")
    assert np.array_equal(i0, P["i0"]) and dw == 0
    # the factors come from two quadrature codes (Newton nodes there, numpy's here): the same float32 unless a value sits on a rounding
    # boundary of the two float64 results, which differ by a few ulps - at most one float32 ulp, and rarely
    assert np.abs(cy.astype(np.int64) - P["cy"].view(np.uint32).astype(np.int64)).max() <= 1
    assert np.abs(cx.astype(np.int64) - P["cx"].view(np.uint32).astype(np.int64)).max() <= 1


def test_default_grids_and_the_grid_rule(plan_tools):
    want = {16: 32, 32: 64, 64: 80, 80: 128, 128: 160, 160: 256, 256: 320, 320: 400, 400: 512, 512: 640, 640: 800, 800: 1024, 1024: 0}
    assert {s: R.default_grid(s) for s in R.SIDES} == want
    assert abs(R.beta_of(6, 32, 16) - 13.8) < 1e-12 and abs(R.beta_of(6, 80, 64) - 0.97 * np.pi * 6 * 0.6) < 1e-12
    # ... and the plan builder's: grid sides 0 select the same grid, and its weights (which carry beta) are the restatement's
    traj = np.array([[0.0, 0.0], [0.21, -0.37], [-0.5, 0.5]])
    for h, w in ((16, 32), (64, 80), (128, 400), (800, 16)):
        text = f"{h} {w} 0 0 6 3\n" + "".join(f"{float(a).hex()} {float(b).hex()}\n" for a, b in traj)
        r = subprocess.run([plan_tools[0]], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        P = R.plan(h, w, 0, 0, 6, traj)
        assert lines[0] == f"grid {want[h]} {want[w]}" == f"grid {P['gh']} {P['gw']}"
        wts = np.array([[int(v, 16) for v in l.split()[3:]] for l in lines[1:4]], dtype=np.uint32).T
        assert np.array_equal(wts, P["wts"].view(np.uint32))


def test_the_sanitizer_program_of_the_argument_validation_passes():
    """`make asan_nufft`: the instrumented host build of the library (host code only) and tests/asan_nufft_host.cpp, a program with its own
    main, run directly."""
    subprocess.run(["make", "-C", CSRC, "-j", "4", "asan_nufft"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(CSRC, "_asan", "asan_nufft_host")], capture_output=True, text=True)
    assert r.returncode == 0 and "asan_nufft_host: ok" in r.stdout, r.stdout + r.stderr


def test_radial_trajectory_dcf_and_the_float64_problem():
    from dt4image_restoration_amd import acquisition
    h, w, spokes = 16, 32, 5
    t = acquisition.radial_trajectory(h, w, spokes)
    assert t.shape == (spokes * 64, 2) and t.dtype == np.float64 and np.array_equal(t, R.radial(h, w, spokes))
    assert np.array_equal(t[0], [-0.0, -0.5]) and np.array_equal(t[32], [0.0, 0.0]) and np.abs(t).max() == 0.5
    u = acquisition.radial_trajectory(h, w, 4, readout=8, golden=False)
    assert u.shape == (32, 2) and np.allclose(u[8 * 2 + 0], [-0.5, 0.0], atol=1e-16)          # spoke 2 of 4 runs along ky
    d = acquisition.radial_dcf(t, h, w)
    r = np.hypot(t[:, 0], t[:, 1])
    assert d.dtype == np.float32 and abs(float(d.astype(np.float64).sum()) - h * w) <= 1e-4 * h * w
    assert np.allclose(d / d.max(), np.maximum(r, 1 / 128) / 0.5, rtol=1e-6)
    p = synthetic.make_problem_nc(2, h, w, t, dcf=d, sigma_n=0.0, seed=3)
    assert p["y0"].shape == (2, 1, t.shape[0], 2) and p["ATy0"].shape == (2, 1, h, w, 2) and p["gt"].shape == (2, 1, h, w)
    y = p["y0"][..., 0].astype(np.float64) + 1j * p["y0"][..., 1]
    assert np.abs(y[:, 0] - R.ndft(t, p["gt"][:, 0].astype(np.float64))).max() <= 1e-6          # float32 storage of an O(1) value
    assert np.array_equal(p["x0"], np.clip(p["ATy0"], 0, None))
    one = synthetic.make_problem_nc(1, h, w, t, dcf=d, sigma_n=0.1, seed=3, first_slice=1)
    two = synthetic.make_problem_nc(2, h, w, t, dcf=d, sigma_n=0.1, seed=3)
    assert np.array_equal(one["y0"][0], two["y0"][1])                                          # a slice depends on (seed, its index) only


def test_the_end_to_end_fixture_gains_what_the_gpu_test_records():
    t = R.FIXTURE
    d, P = R.fixture_problem()
    mu, sig = R.fixture_schedules()
    x, p0, p1 = R.admm_tv_nc(d, P, mu, sig, t["cg_iters"], t["tv_scale"], t["tv_iters"])
    print(f"float64 TV-ADMM on {t['spokes']} golden spokes: PSNR of x0 {p0[0]:.3f} dB, final {p1[0]:.3f} dB, gain {p1[0] - p0[0]:.3f} dB")
    assert p1[0] - p0[0] >= 1.0
    assert abs(p0[0] - R.FIXTURE_PSNR[0]) <= 2e-3 and abs(p1[0] - R.FIXTURE_PSNR[1]) <= 2e-3
    assert (P["gh"], P["gw"], P["m"]) == (80, 80, t["spokes"] * 128)


def test_task_problem_and_cli_refuse_what_the_non_cartesian_path_cannot_do():
    from dt4image_restoration_amd import acquisition, cli
    assert "radial-nc" in acquisition.NC_KINDS
    sig = inspect.signature(acquisition.task_problem).parameters
    assert sig["spokes"].default is None and sig["nc_weights"].default == "dcf" and sig["nufft_width"].default == 6
    assert list(inspect.signature(acquisition.radial_dcf).parameters) == ["traj", "h", "w"]
    t = acquisition.radial_trajectory(16, 16, 3, readout=40)                       # the readout is read from the trajectory
    d = acquisition.radial_dcf(t, 16, 16)
    assert np.allclose(d / d.max(), np.maximum(np.hypot(t[:, 0], t[:, 1]), 1 / 80) / 0.5, rtol=1e-6)
    with pytest.raises(ValueError):
        acquisition.radial_dcf(np.zeros((4, 2)), 16, 16)
    base = ["--block_size", "6", "--n_embeds", "9", "--prior", "tv"]
    for extra, what in ((["--traj", "radial", "--coils", "4"], "--traj with --coils"), (["--spokes", "8"], "need --traj radial"),
                        (["--nufft-width", "8"], "need --traj radial"), (["--nc-weights", "none"], "need --traj radial"),
                        (["--traj", "radial", "--spokes", "0"], "--spokes must be"), (["--traj", "radial", "--mask", "cartesian"], "--traj takes no --mask")):
        with pytest.raises(SystemExit, match=what):
            cli.main(base + extra + ["fixed", "--max_iter", "2"])
    with pytest.raises(SystemExit):                                                # argparse: 5 is no kernel width
        cli.main(base + ["--traj", "radial", "--nufft-width", "5", "fixed"])
