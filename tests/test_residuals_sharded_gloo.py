"""drivers/sharded.run_sharded_fixed under two gloo ranks on the CPU (pattern of tests/test_sharding_gloo.py): every rank runs
FixedScheduleSolver on its contiguous shard of the slices - the CPU oracle stands in for the per-rank engine - and the per-slice
PSNR, stop iteration, final delta / primal and data misfit are gathered; the result equals the single-process run."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dt4image_restoration_amd import sharding, synthetic
import residual_ref as R

TOTAL, H, ITERS, TOL = 3, 32, 6, 0.02        # ragged on purpose: shards of 2 and 1 slices


def _parts():
    from dt4image_restoration_amd.drivers.fixed import FixedScheduleSolver
    solver = FixedScheduleSolver(R.OracleEnv(), max_iter=ITERS, tol=TOL, sync_every=2, dc=True, device_type="cpu")
    mu, sg = synthetic.param_table(TOTAL, ITERS, seed=5)

    def load_shard(a, b):
        p = synthetic.make_problem(b - a, H, H, accel=4.0, seed=42, first_slice=a)
        return {k: torch.from_numpy(np.asarray(v)) for k, v in p.items()}, mu[a:b], sg[a:b]
    return solver, load_shard


def _worker(rank, world, port, out_dir):
    from dt4image_restoration_amd.drivers.sharded import run_sharded_fixed
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    solver, load_shard = _parts()
    r = run_sharded_fixed(solver, TOTAL, load_shard)
    assert r.local_range == sharding.shard_range(TOTAL, rank, world)
    np.savez(os.path.join(out_dir, f"f{rank}.npz"), psnr=r.psnr.numpy(), init=r.initial_psnr.numpy(), iters=r.iterations.numpy(),
             delta=r.delta.numpy(), primal=r.primal.numpy(), dc=r.dc.numpy())
    dist.destroy_process_group()


def test_two_rank_sharded_fixed_equals_single_process(tmp_path):
    from dt4image_restoration_amd.drivers.sharded import run_sharded_fixed
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    solver, load_shard = _parts()
    want = run_sharded_fixed(solver, TOTAL, load_shard)       # no process group: world size 1
    assert want.psnr.shape == (TOTAL, 1) and want.iterations.shape == (TOTAL,) and want.dc.shape == (TOTAL,)
    assert want.local_range == (0, TOTAL) and 1 <= want.steps <= ITERS
    res = solver.run(*load_shard(0, TOTAL))                    # the unsharded result is the solver's own
    np.testing.assert_array_equal(res.psnr.numpy(), want.psnr.numpy())
    np.testing.assert_array_equal(res.iterations.numpy(), want.iterations.numpy())
    for r in range(2):
        got = np.load(tmp_path / f"f{r}.npz")
        np.testing.assert_array_equal(got["init"], want.initial_psnr.numpy())       # x0 is shard-consistent: exact
        np.testing.assert_array_equal(got["iters"], want.iterations.numpy())
        # FLOAT TOLERANCE: a slice alone or in a batch of 2 takes another oneDNN blocking of the same f32 convolutions
        np.testing.assert_allclose(got["psnr"], want.psnr.numpy(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(got["delta"], want.delta.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["primal"], want.primal.numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(got["dc"], want.dc.numpy(), rtol=0, atol=1e-5)
