"""CPU-only checks of the SSIM metric (pnp_ssim): the entry point is exported, declared and bound, rejects bad arguments
before any HIP call (from Python and from C), the G9 fixture agrees with a float64 restatement of scipy's Gaussian-window
SSIM kept in this file, the built ssim kernels are free of scratch, spills and low-reads-high packed-f32 ops, and the
sharded greedy driver gathers SSIM exactly like PSNR (two gloo ranks, CPU oracle env)."""
import ctypes as C
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dt4image_restoration_amd import _lib, sharding, synthetic, weights
from oracle import pnp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ((11, 1.0), (11, 255.0), (7, 1.0))
PAIRS = ("p128_x0", "p128_blur", "p96x80_x0", "p256_blur", "p16_x0")


# ---- float64 restatement of calculate_ssim (scipy gaussian_filter(sigma=1.5, truncate=win//2), mode 'reflect') -------------
def gaussian_taps(win_size):
    r = int(1.5 * (win_size // 2) + 0.5)
    t = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (1.5 * 1.5) * t * t)
    return w / w.sum()


def gfilter(a, w):
    """Separable correlation over the last two axes; numpy's 'symmetric' pad is scipy's 'reflect' (d c b a | a b c d)."""
    r = (len(w) - 1) // 2
    h, wd = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode="symmetric")
    p = sum(w[k] * p[..., k:k + h, :] for k in range(len(w)))
    return sum(w[k] * p[..., :, k:k + wd] for k in range(len(w)))


def ssim_ref(x, y, k1=0.01, k2=0.03, win_size=11, L=255.0):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = gaussian_taps(win_size)
    c1, c2 = (k1 * L) ** 2, (k2 * L) ** 2
    mx, my = gfilter(x, w), gfilter(y, w)
    vx, vy, cxy = gfilter(x * x, w) - mx * mx, gfilter(y * y, w) - my * my, gfilter(x * y, w) - mx * my
    smap = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return smap, smap.mean(axis=(-2, -1))


def test_pnp_ssim_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnpadmm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pnp_ssim\s*\(", src) and "#define PNP_SSIM_CLAMP_X 1" in src
    lib = _lib.load()
    assert hasattr(lib, "pnp_ssim") and "pnp_ssim" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pnp_ssim"][1]) == 11 and _lib.PNP_SSIM_CLAMP_X == 1


@pytest.mark.parametrize("radius,data_range,flags,what", [(0, 1.0, 1, b"radius"), (17, 1.0, 0, b"radius"),
                                                         (8, 0.0, 1, b"data_range"), (8, -1.0, 0, b"data_range"),
                                                         (8, 1.0, 2, b"flag"), (8, 1.0, 1, b"null")])
def test_pnp_ssim_rejects_bad_arguments_without_a_gpu(radius, data_range, flags, what):
    lib = _lib.load()
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value                    # never dereferenced: every case fails validation first
    rc = lib.pnp_ssim(None, p, p, data_range, 0.01, 0.03, radius, flags, p, None, None)
    assert rc == -1
    assert what in lib.pnp_last_error()


def test_pnp_ssim_rejects_from_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "ssim_abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <string.h>\n#include "pnpadmm.h"\n'
        "int main(void) {\n"
        "    float v[4] = {0};\n"
        "    if (pnp_ssim(0, v, v, 1.0f, 0.01f, 0.03f, 8, PNP_SSIM_CLAMP_X, v, 0, 0) != PNP_ERR_INVALID) return 1;  /* null handle */\n"
        "    if (!strstr(pnp_last_error(), \"null\")) return 2;\n"
        "    if (pnp_ssim(0, v, v, 1.0f, 0.01f, 0.03f, 0, 0, v, 0, 0) != PNP_ERR_INVALID) return 3;\n"
        "    if (!strstr(pnp_last_error(), \"radius\")) return 4;\n"
        "    if (pnp_ssim(0, v, v, 1.0f, 0.01f, 0.03f, 17, 0, v, 0, 0) != PNP_ERR_INVALID) return 5;\n"
        "    if (pnp_ssim(0, v, v, 0.0f, 0.01f, 0.03f, 8, 0, v, 0, 0) != PNP_ERR_INVALID) return 6;\n"
        "    if (!strstr(pnp_last_error(), \"data_range\")) return 7;\n"
        '    printf("ok\\n");\n'
        "    return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "ssim_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-lpnpadmm", f"-Wl,-rpath,{libdir}"], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip() == "ok"


def test_g9_fixture_matches_the_float64_restatement(golden_dir):
    z = np.load(os.path.join(golden_dir, "g9_ssim.npz"))
    assert [str(p) for p in z["pairs"]] == list(PAIRS)
    assert os.path.getsize(os.path.join(golden_dir, "g9_ssim.npz")) < 512 * 1024
    maps = 0
    for name in PAIRS:
        x, gt = z[f"{name}_x"].astype(np.float64), z[f"{name}_gt"].astype(np.float64)
        for j, (win, L) in enumerate(PARAMS):
            smap, score = ssim_ref(x, gt, win_size=win, L=L)
            assert abs(float(z[f"{name}_score{j}"]) - float(score)) <= 1e-12, (name, win, L)
            if f"{name}_map{j}" in z.files:
                maps += 1
                assert np.abs(z[f"{name}_map{j}"] - smap).max() <= 1e-6      # stored as float32
    assert maps == 9                                            # 128 x 128 (2 pairs) and 16 x 16, three parameter sets


def _ssim_code_object_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no llvm tools / library")
    meta = {}
    for i, co in enumerate(isa_audit.code_objects(_lib.LIB_PATH)):
        f = os.path.join(isa_audit.TMP, "ssim_co%d.o" % i)
        open(f, "wb").write(co)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        cur = None
        for line in notes.split("\n"):
            m = re.match(r"^    \.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = m.group(2) if "ssim" in m.group(2) else None
                if cur:
                    meta[cur] = {}
            elif cur:
                meta[cur][m.group(1)] = int(m.group(2))
    rows = {}
    for path in isa_audit.disassemble(_lib.LIB_PATH):
        for name, n_pk, n_lohi, _mf, _flagged in isa_audit.audit_asm(path, verbose=False)[1]:
            if "ssim" in name:
                rows[name] = (n_pk, n_lohi)
    return meta, rows


def test_ssim_kernels_have_no_scratch_spills_or_low_reads_high_ops():
    meta, rows = _ssim_code_object_kernels()
    tiles = [k for k in meta if "ssim_tile_kernel" in k]
    assert len(tiles) == 16 and any("ssim_reduce_kernel" in k for k in meta)     # radius 1..16, and the reduce
    for name, m in meta.items():
        assert m == {"private_segment_fixed_size": 0, "sgpr_spill_count": 0, "vgpr_spill_count": 0}, (name, m)
    assert set(rows) == set(meta)
    for name, (_n_pk, n_lohi) in rows.items():
        assert n_lohi == 0, name


# ---- run_sharded_greedy(ssim=True) under 2 gloo ranks (pattern of tests/test_sharding_gloo.py) ------------------------------
GT, GH, GSTEPS = 3, 128, 4


def _greedy_parts():
    from dt4image_restoration_amd import data as D
    from dt4image_restoration_amd.drivers.greedy import GreedyEvaluator
    from dt4image_restoration_amd.policy import DecisionTransformer, DecisionTransformerConfig

    class OracleEnv:                                        # PnPEnv-shaped wrapper over the CPU oracle (tests only)
        def __init__(self):
            self.sd = O.torch_weights(weights.generate_unet_weights(0, "unit_gain"))

        def reset(self, mat, device):
            return O.reset({k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in mat.items()})

        def step(self, st, action):
            with torch.no_grad():
                return O.admm_step(self.sd, st, action["mu"], action["sigma_d"], action["T"])

        def compute_reward(self, x, gt):
            return O.psnr(x, gt)

        def compute_ssim(self, x, gt):
            h, w = gt.shape[-2:]
            xr = (x.real if x.is_complex() else x).double().clamp(0, 1).reshape(-1, h, w).numpy()
            return torch.from_numpy(ssim_ref(xr, gt.double().reshape(-1, h, w).numpy(), L=1.0)[1]).float().reshape(-1, 1)

    m = DecisionTransformer(DecisionTransformerConfig(block_size=18, n_embeds=9, mode="norm"))
    m.load_state_dict(weights.generate_policy_weights(m, 7, t_bias=-1.0, head_gain=8.0))
    ev = GreedyEvaluator(m, OracleEnv(), max_timesteps=GSTEPS, block_size=18, device_type="cpu", sync_every=2, ssim=True)

    def load_shard(a, b):
        p = synthetic.make_problem(b - a, GH, GH, accel=4.0, seed=77, first_slice=a)
        mat = {k: torch.from_numpy(np.asarray(v)) for k, v in p.items()}
        return mat, torch.full((b - a,), D.normalised_rtg(10.0)), torch.full((b - a,), 4)
    return ev, load_shard


def _greedy_worker(rank, world, port, out_dir):
    from dt4image_restoration_amd.drivers.sharded import run_sharded_greedy
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ev, load_shard = _greedy_parts()
    r = run_sharded_greedy(ev, GT, load_shard)
    assert r.local_range == sharding.shard_range(GT, rank, world)
    np.savez(os.path.join(out_dir, f"s{rank}.npz"), ssim=r.ssim.numpy(), init=r.initial_ssim.numpy(), reward=r.reward.numpy())
    dist.destroy_process_group()


def test_two_rank_sharded_greedy_gathers_ssim_like_psnr(tmp_path):
    from dt4image_restoration_amd.drivers.sharded import run_sharded_greedy
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_greedy_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    ev, load_shard = _greedy_parts()
    want = run_sharded_greedy(ev, GT, load_shard)          # no process group: world size 1
    assert want.ssim.shape == (GT, 1) and want.initial_ssim.shape == (GT, 1)
    assert bool(((want.ssim > 0) & (want.ssim <= 1)).all())
    # the unsharded result is the per-slice SSIM of the run's own images
    res = ev.run(*load_shard(0, GT))
    np.testing.assert_array_equal(res.ssim.numpy(), want.ssim.numpy())
    np.testing.assert_array_equal(res.initial_ssim.numpy(), want.initial_ssim.numpy())
    for r in range(2):                                     # ragged shards: 2 + 1 slices
        got = np.load(tmp_path / f"s{r}.npz")
        assert got["ssim"].shape == (GT, 1)
        np.testing.assert_array_equal(got["init"], want.initial_ssim.numpy())       # x0 is shard-consistent: exact
        # FLOAT TOLERANCE: a slice alone or in a batch of 2 takes another oneDNN blocking of the same f32 convolutions
        np.testing.assert_allclose(got["ssim"], want.ssim.numpy(), rtol=0, atol=1e-5)


def test_greedy_evaluator_leaves_ssim_off_by_default():
    from dt4image_restoration_amd.drivers.greedy import GreedyEvaluator, GreedyResult
    from dt4image_restoration_amd.drivers.sharded import ShardedResult
    import inspect
    assert inspect.signature(GreedyEvaluator).parameters["ssim"].default is False
    r = GreedyResult(reward=torch.zeros(1, 1), initial_reward=torch.zeros(1, 1), stop_time=torch.zeros(1), actions=torch.zeros(1, 1, 3),
                     x=torch.zeros(1, 1, 16, 16))
    assert r.ssim is None and r.initial_ssim is None
    assert ShardedResult.__dataclass_fields__["ssim"].default is None


def test_calculate_ssim_refuses_bad_shapes_and_cpu_only_use():
    from dt4image_restoration_amd.transformations import calculate_ssim
    with pytest.raises(ValueError, match="multiples of 16"):
        calculate_ssim(np.zeros((20, 32)), np.zeros((20, 32)))
    with pytest.raises(ValueError):
        calculate_ssim(np.zeros((32, 32)), np.zeros((16, 32)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            calculate_ssim(np.zeros((32, 32)), np.zeros((32, 32)))
