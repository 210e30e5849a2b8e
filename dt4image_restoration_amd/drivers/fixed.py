"""Plain PnP-ADMM with a fixed or scheduled (mu, sigma_d), stopped by the iterates themselves: the baseline every learned policy is
compared with, and the way to drive sizes the 128 x 128-trained policy has not seen (policy.py).

The reference has no such driver: its loops (`Evaluator.run_greedy` evaluation/eval.py:189-220, `run_mcts`
mcts.py:212-258) stop when the policy says so.  Here the stop is the fixed-point criterion of Chan, Wang, Elgendy, "Plug-and-Play ADMM
for image restoration: fixed-point convergence" (2017): with (x_p, z_p, u_p) the iterate before the step,

    delta = (||x - x_p|| + ||z - z_p|| + ||u - u_p||) / sqrt(H W)  <=  tol

per slice, computed on the device by `pnp_residuals` (`PnPEnv.residuals`).  Each iteration is  snapshot -> env.step -> residuals; a
slice whose delta has met the tolerance is handed T = 1 from the next step on, so the engine leaves it untouched (env.py:79-81) - the
same mechanism as a policy stop - and the decision never leaves the device.  The loop's only host synchronisation is the
all-stopped check every `sync_every` iterations, as in `GreedyEvaluator`.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Optional

import torch

# columns of PnPEnv.residuals (engine.RESIDUAL_COLUMNS)
_PRIMAL, _DELTA, _DC = 0, 4, 5


@dataclass
class FixedResult:
    psnr: torch.Tensor          # [N,1] final PSNR (CPU), env.compute_reward
    initial_psnr: torch.Tensor  # [N,1] PSNR of x0
    iterations: torch.Tensor    # [N] int64 (CPU): first iteration (1-based) at which delta <= tol held, max_iter if never
    delta: torch.Tensor         # [N, max_iter] (CPU) delta after every iteration; a stopped slice's last value repeated
    primal: torch.Tensor        # [N, max_iter] (CPU) ||x - z|| after every iteration, likewise
    x: torch.Tensor             # [N,1,H,W] final images (device)
    z: Optional[torch.Tensor] = None    # [N,1,H,W] complex64 final z (device)
    u: Optional[torch.Tensor] = None    # [N,1,H,W] complex64 final u (device)
    dc: Optional[torch.Tensor] = None   # [N] (CPU) data misfit ||where(mask, fft_c(x) - y0, 0)|| of the final iterate (dc=True)
    ssim: Optional[torch.Tensor] = None          # [N,1] final SSIM (ssim=True)
    initial_ssim: Optional[torch.Tensor] = None  # [N,1]
    steps: int = 0              # iterations the loop ran (<= max_iter: it ends early once every slice has stopped)


class FixedScheduleSolver:
    def __init__(self, env, max_iter: int = 30, tol: Optional[float] = None, sync_every: int = 1, dc: bool = False,
                 device_type="cuda", ssim: bool = False):
        if max_iter < 1:
            raise ValueError(f"max_iter must be >= 1 (got {max_iter})")
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError(f"tol must be >= 0 or None (got {tol})")
        self.env = env
        self.max_iter = int(max_iter)
        self.tol = None if tol is None else float(tol)
        self.sync_every = max(1, int(sync_every))
        self.dc = bool(dc)
        self.ssim = bool(ssim)
        self.device = torch.device(device_type)

    def _table(self, tab, n: int, name: str) -> torch.Tensor:
        t = torch.as_tensor(tab, dtype=torch.float32)
        if t.dim() == 1:                                       # one schedule for every slice
            t = t.reshape(1, -1).expand(n, -1)
        if t.dim() != 2 or t.shape[0] != n or t.shape[1] < self.max_iter:
            raise ValueError(f"{name}: expected a table [{n}, >= {self.max_iter}], got {tuple(t.shape)}")
        # one contiguous row of parameters per iteration
        return t[:, :self.max_iter].t().contiguous().to(self.device)

    @torch.no_grad()
    def run(self, mat: Dict[str, torch.Tensor], mu_tab, sigma_tab) -> FixedResult:
        """mat: collated `.mat` dict (x0, y0, ATy0, mask, gt); mu_tab, sigma_tab: per-slice tables [N, max_iter] (what
        `synthetic.param_table` returns; a 1-D schedule is shared by all slices), column t - 1 drives iteration t."""
        env, dev, K = self.env, self.device, self.max_iter
        states = env.reset(mat, dev)
        n = states["z"].shape[0]
        mu_t, sg_t = self._table(mu_tab, n, "mu_tab"), self._table(sigma_tab, n, "sigma_tab")
        initial = env.compute_reward(states["x"], states["gt"])
        initial_ssim = env.compute_ssim(states["x"], states["gt"]) if self.ssim else None
        stopped = torch.zeros(n, dtype=torch.bool, device=dev)
        iterations = torch.full((n,), K, dtype=torch.int64, device=dev)
        hist = torch.zeros((K, 2, n), dtype=torch.float32, device=dev)      # [iteration, (delta, primal), slice]
        last = torch.zeros((2, n), dtype=torch.float32, device=dev)
        steps = 0
        for it in range(1, K + 1):
            prev = env.snapshot(states)
            action = OrderedDict((("T", stopped.to(torch.float32)), ("mu", mu_t[it - 1]), ("sigma_d", sg_t[it - 1])))
            states, _ = env.step(states, action)
            r = env.residuals(states, prev=prev)
            live = ~stopped
            # a stopped slice was not stepped (its delta against the snapshot is 0): its history repeats the last value
            last = torch.where(live.reshape(1, n), torch.stack((r[:, _DELTA], r[:, _PRIMAL])), last)
            hist[it - 1] = last
            steps = it
            if self.tol is not None:
                newly = live & (r[:, _DELTA] <= self.tol)
                iterations = torch.where(newly, torch.full_like(iterations, it), iterations)
                stopped = stopped | newly
                if it < K and it % self.sync_every == 0 and bool(stopped.all()):      # the loop's only host sync
                    break
        if steps < K:
            hist[steps:] = last
        dc = env.residuals(states, dc=True)[:, _DC].cpu() if self.dc else None
        return FixedResult(psnr=env.compute_reward(states["x"], states["gt"]), initial_psnr=initial, iterations=iterations.cpu(),
                           delta=hist[:, 0].t().contiguous().cpu(), primal=hist[:, 1].t().contiguous().cpu(), x=states["x"], z=states["z"], u=states["u"], dc=dc,
                           ssim=env.compute_ssim(states["x"], states["gt"]) if self.ssim else None, initial_ssim=initial_ssim,
                           steps=steps)
