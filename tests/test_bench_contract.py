"""bench.py's output contract (one JSON line: metric / value / roofline / cpu_baseline ...), on a small problem."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    # (a child process: the test runner itself has initialised the GPU and must not exec)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "128", "--batch", "8", "--steps", "3", "--warmup", "1",
                          "--full", "--reps", "2", "--cpu-slices", "1", "--cpu-iters", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "pnp_admm_iterations_per_sec" and d["unit"] == "batch-iterations/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0 < r["frac"] <= 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1
    assert abs(d["psnr_delta_vs_oracle_db"]) < 0.01          # BASELINE's parity bar, on the baseline sample


@pytest.mark.gpu
def test_plain_bench_times_one_episode_and_dumps_what_it_computed(tmp_path):
    """A plain run (no --full): one episode of exactly --steps timed steps, the headline fields and nothing of the --full record;
    --dump-outputs holds the iterate after the last timed step (its PSNR is the line's psnr_mean_db)."""
    import numpy as np
    import torch
    from dt4image_restoration_amd import synthetic
    from oracle import pnp_oracle as O
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "128", "--batch", "8", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["repetitions"]["n"] == 1 and d["dtype"] == "f32"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    for k in ("cpu_baseline", "greedy", "config4", "psnr_delta_vs_oracle_db"):
        assert k not in d, k
    arrays = {name: np.load(tmp_path / f"{name}.npy") for name in ("x", "z", "u")}
    assert arrays["x"].shape == (8, 1, 128, 128) and arrays["z"].shape == arrays["u"].shape == (8, 1, 128, 128, 2)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
    gt = torch.from_numpy(synthetic.make_problem(8, 128, 128, accel=4.0, sigma_n=10.0 / 255.0, seed=1234)["gt"])
    assert abs(float(O.psnr(torch.from_numpy(arrays["x"]), gt).mean()) - d["psnr_mean_db"]) < 1e-3


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path):
    """bench.dump_outputs: float32 files; an array above DUMP_CAP scalars becomes a fixed seeded sample (same elements every run),
    so the headline's x, z, u (64 x 256 x 256, f32 + 2 x complex64) stay under 64 MB together."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    x = torch.rand(64, 1, 256, 256, generator=g)
    z = torch.complex(torch.rand(64, 1, 256, 256, generator=g), torch.rand(64, 1, 256, 256, generator=g))
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"x": x, "z": z, "u": z.to(torch.complex128)})
    xa, za, ua = (np.load(tmp_path / "a" / f"{n}.npy") for n in "xzu")
    assert xa.dtype == za.dtype == ua.dtype == np.float32
    assert np.array_equal(xa, x.numpy())                                  # 4 Mi scalars: written whole
    assert za.shape == (bench.DUMP_CAP // 2, 2) and np.array_equal(za, ua)
    flat = torch.view_as_real(z).reshape(-1, 2).numpy()
    assert np.isin(za[:, 0], flat[:, 0]).all() and not np.array_equal(za, flat[:len(za)])    # a sample, not a prefix
    for n in "xzu":
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
