"""`PnPEnv`: the reference's PnP-ADMM environment interface (/root/reference/evaluation/env.py:30-116)
served by the HIP engine.  Same method names, arity and return shapes, so a driver written against the
reference (`Evaluator.run_greedy` eval.py:189-220, `run_mcts` mcts.py:212-258) calls it unchanged:

    reset(data, device) -> OrderedDict          step(states, action_dict) -> (states, done)
    get_policy_ob(states)                       compute_reward(x, gt)       run_no_ref_reward(states)

plus `compute_ssim(x, gt)`, the reference's `calculate_ssim` on the image `compute_reward` judges.

Differences, all documented in DESIGN.md:
  * any batch N and H, W each one of 16..1024 of the form 2^a * 5^b: the powers of two and 80, 160, 320, 400, 640, 800
    (fastMRI's 320 x 320, 640 x 320; the reference is hard-wired to 1 x 128 x 128, env.py:44,64,115)
  * per-slice mu / sigma_d / T (1-element tensors broadcast, as the reference's drivers pass)
  * states['x'|'z'|'u'] are persistent device tensors updated IN PLACE by `step` (the reference rebinds
    freshly allocated tensors, env.py:95-97); use `snapshot`/`restore` to keep an old state (MCTS)
  * states['x'] is float32 from reset on (the reference holds complex x0 until the first step;
    every caller reads `.real`, which is a no-op on a real tensor)
  * the ARNIQA scorer (a torch.hub network fetch, env.py:36-40) is replaced by an injectable callable
  * `step` stays a function of the `states` it is handed (as in the reference, env.py:75,88-90): the engine holds ONE set
    of pre-shifted k-space constants, and states carry the id of their episode in the private key `_episode`; when
    states of another episode (another env on the same denoiser, an older reset) are stepped, the shim re-installs that
    episode's y0 / mask from the dict first (pnp_set_kspace)
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Dict, Optional, Tuple

import torch

from .denoiser import UNetDenoiser2D
from .engine import PnPEngine, _next_episode


def _as_complex(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_complex() else torch.view_as_complex(t.contiguous().float())


class PnPEnv:
    def __init__(self, max_episode_step: int, denoiser: UNetDenoiser2D, device_type,
                 no_ref_scorer: Optional[Callable[[torch.Tensor], float]] = None, replica: int = 0, cg_iters: int = 8,
                 nufft_width: int = 6, nufft_grid=None, nc_normal: str = "nufft",
                 offres_normal: str = "nufft", offres_mc: bool = False) -> None:
        if nc_normal not in ("nufft", "toeplitz"):
            raise ValueError(f"nc_normal must be 'nufft' or 'toeplitz', got {nc_normal!r}")
        if offres_normal not in ("nufft", "toeplitz"):
            raise ValueError(f"offres_normal must be 'nufft' or 'toeplitz', got {offres_normal!r}")
        self.offres_normal = offres_normal      # off-resonance episodes: the form of A^H W A inside the CG (include/pnpadmm_offres_tz.h)
        self.offres_mc = bool(offres_mc)        # data["omega"] with data["sens"]: the coils x segments stage (include/pnpadmm_offres_mc.h)
        self.nc_normal = nc_normal              # non-Cartesian episodes: the form of A^H W A inside the CG (include/pnpadmm_toeplitz.h)
        self.max_episode_step = max_episode_step
        self.cg_iters = int(cg_iters)           # multi-coil and non-Cartesian episodes: conjugate-gradient iterations per step
        self.nufft_width = int(nufft_width)     # non-Cartesian episodes (data["traj"]): the kernel width and the grid (None: the default)
        self.nufft_grid = None if nufft_grid is None else (int(nufft_grid[0]), int(nufft_grid[1]))
        self.denoiser = denoiser.to(device_type)
        self.no_ref_model = no_ref_scorer
        self._engine: Optional[PnPEngine] = None
        self._device_type = device_type
        self._replica = int(replica)

    def fork(self, replica: int) -> "PnPEnv":
        """Another env on the same denoiser weights whose engines are replicas of their own (own workspace, own k-space
        constants): two sub-batches of one job can then be stepped concurrently on two streams."""
        return PnPEnv(self.max_episode_step, self.denoiser, self._device_type, self.no_ref_model, replica=replica, cg_iters=self.cg_iters,
                      nufft_width=self.nufft_width, nufft_grid=self.nufft_grid, nc_normal=self.nc_normal,
                      offres_mc=getattr(self, "offres_mc", False), offres_normal=getattr(self, "offres_normal", "nufft"))

    # ---- engine management ------------------------------------------------------------------
    def _engine_for(self, n: int, h: int, w: int, device: torch.device) -> PnPEngine:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self._engine = self.denoiser.engine_for(n, h, w, idx, self._replica)
        return self._engine

    # ---- reference interface ----------------------------------------------------------------
    def reset(self, data: Dict[str, torch.Tensor], device_type) -> "OrderedDict[str, torch.Tensor]":
        """env.py:57-71.  data: collated `.mat` dict - x0, y0, ATy0 float [..,H,W,2]; mask [..,H,W]; gt."""
        device = torch.device(device_type)
        if device.type != "cuda":
            raise RuntimeError("PnPEnv runs on the GPU only (device_type='cuda'); there is no CPU path")
        x0 = _as_complex(torch.as_tensor(data["x0"]))
        h, w = x0.shape[-2:]
        n = x0.numel() // (h * w)
        x0 = x0.reshape(n, 1, h, w).to(device).contiguous()
        if hasattr(data, "get") and data.get("traj") is not None:
            return self._reset_nc(data, x0, n, h, w, device)
        sens = data.get("sens") if hasattr(data, "get") else None
        if sens is not None:                    # a multi-coil problem: sens [C,H,W] or [N,C,H,W], y0 with a coil axis
            sens = torch.as_tensor(sens)
            sens = (sens if sens.is_complex() else _as_complex(sens)).to(torch.complex64)
            if sens.dim() not in (3, 4) or tuple(sens.shape[-2:]) != (h, w) or (sens.dim() == 4 and sens.shape[0] != n):
                raise ValueError(f"sens: expected [C,{h},{w}] or [{n},C,{h},{w}], got {tuple(sens.shape)}")
            sens = sens.to(device).contiguous()
            coils = sens.shape[-3]
        else:
            coils = 1
        y0 = _as_complex(torch.as_tensor(data["y0"])).reshape(n, coils, h, w).to(device).contiguous()
        mask = torch.as_tensor(data["mask"])
        mask = mask.reshape(-1, h, w) if mask.numel() != h * w else mask.reshape(h, w)
        if mask.dim() == 3 and mask.shape[0] not in (1, n):
            raise ValueError(f"mask batch {mask.shape[0]} does not match {n} slices")
        mask = mask.to(device).to(torch.bool).contiguous()
        gt = torch.as_tensor(data["gt"]).to(device).float()
        eng = self._engine_for(n, h, w, device)
        x, z, u = eng.reset(x0, y0, mask, sens=sens, cg_iters=self.cg_iters)
        aty0 = torch.as_tensor(data["ATy0"])[..., 0] if "ATy0" in data else None
        return OrderedDict({"x": x, "y0": y0, "z": z, "u": u, "mask": mask, "gt": gt, "ATy0": aty0,
                            "T": torch.zeros(n, dtype=torch.float32, device=device),
                            "complex_y0": data["y0"], "_episode": eng.live_episode, "sens": sens})

    def _plan_nc(self, eng: PnPEngine, traj) -> None:
        """The engine's NUFFT plan is the one of this trajectory: re-planned only when it differs from the live plan."""
        if not eng.nufft_planned(traj, self.nufft_grid, self.nufft_width):
            eng.nufft_plan(traj, grid=self.nufft_grid, width=self.nufft_width)

    def _reset_nc(self, data, x0: torch.Tensor, n: int, h: int, w: int, device) -> "OrderedDict[str, torch.Tensor]":
        """A non-Cartesian episode: data["traj"] float64 [M,2], y0 [N,1,M,2] (or complex [N,M]), optional data["dcf"] float32 [M].  With
        data["sens"] (complex [C,H,W] or [N,C,H,W]) it is a non-Cartesian SENSE episode: y0 [N,C,M,2] (or complex [N,C,M])."""
        traj = torch.as_tensor(data["traj"]).to(torch.float64).cpu().reshape(-1, 2).contiguous()      # (the caller's own tensor when it is one)
        m = traj.shape[0]
        sens = data.get("sens")
        if sens is not None and data.get("omega") is not None and not getattr(self, "offres_mc", False):
            raise ValueError("an off-resonance episode is single-coil (data['omega'] with data['sens'] is not supported)")
        if sens is not None:
            sens = torch.as_tensor(sens)
            sens = (sens if sens.is_complex() else _as_complex(sens)).to(torch.complex64)
            if sens.dim() not in (3, 4) or tuple(sens.shape[-2:]) != (h, w) or (sens.dim() == 4 and sens.shape[0] != n):
                raise ValueError(f"sens: expected [C,{h},{w}] or [{n},C,{h},{w}], got {tuple(sens.shape)}")
            sens = sens.to(device).contiguous()
        y0 = _as_complex(torch.as_tensor(data["y0"]))
        y0 = (y0.reshape(n, m) if sens is None else y0.reshape(n, sens.shape[-3], m)).to(device).contiguous()
        dcf = data.get("dcf")
        dcf = None if dcf is None else torch.as_tensor(dcf).to(device, torch.float32).reshape(m).contiguous()
        gt = torch.as_tensor(data["gt"]).to(device).float()
        eng = self._engine_for(n, h, w, device)
        self._plan_nc(eng, traj)
        if data.get("omega") is not None:                   # under a field map: the time-segmented stage (include/pnpadmm_offres.h)
            return self._reset_offres(data, eng, x0, y0, sens, dcf, gt, traj, n, device)
        if sens is None:
            x, z, u = (eng.reset_nc_tz if self.nc_normal == "toeplitz" else eng.reset_nc)(x0, y0, dcf, cg_iters=self.cg_iters)
        else:
            x, z, u = (eng.reset_ncsense_tz if self.nc_normal == "toeplitz" else eng.reset_ncsense)(x0, y0, sens, dcf, cg_iters=self.cg_iters)
        aty0 = torch.as_tensor(data["ATy0"])[..., 0] if "ATy0" in data else None
        return OrderedDict({"x": x, "y0": y0, "z": z, "u": u, "mask": None, "gt": gt, "ATy0": aty0,
                            "T": torch.zeros(n, dtype=torch.float32, device=device),
                            "complex_y0": data["y0"], "_episode": eng.live_episode, "sens": sens, "traj": traj, "dcf": dcf})

    @staticmethod
    def _offres_args(data, m: int):
        """(times float64 [M] on the host, segments) of an off-resonance episode: data["times"], and data["segments"] or the chooser's
        (`acquisition.offres_segments` of max |omega| and the span of the times, at most the library's 32)"""
        from . import acquisition
        if data.get("times") is None:
            raise ValueError('an off-resonance episode (data["omega"]) needs data["times"]: the time of every trajectory sample')
        times = torch.as_tensor(data["times"]).to(torch.float64).cpu().reshape(-1).contiguous()
        if times.numel() != m:
            raise ValueError(f"times: expected {m} samples, got {tuple(times.shape)}")
        seg = data.get("segments")
        if seg is None:
            om_max = float(torch.as_tensor(data["omega"]).abs().max())
            if PnPEnv._interp_of(data) == "ls":
                seg = min(acquisition.offres_ls_segments(om_max * (1.0 + 1e-6), float(times.max() - times.min())), acquisition.OFFRES_MAX_SEGMENTS)
            else:
                seg = min(acquisition.offres_segments(om_max, float(times.max() - times.min())), acquisition.OFFRES_MAX_SEGMENTS)
        return times, int(seg)

    @staticmethod
    def _interp_of(data) -> str:
        """data["b0_interp"]: "linear" | "ls", or pnp_offres_interpolator's code 1 | 2 (what `acquisition.simulate` writes); absent: linear"""
        v = data.get("b0_interp", "linear")
        if not isinstance(v, str):
            v = {1: "linear", 2: "ls"}.get(int(v), v)
        if v not in ("linear", "ls"):
            raise ValueError(f"data['b0_interp'] must be 'linear' or 'ls' (or 1 or 2), got {v!r}")
        return v

    @staticmethod
    def _offres_plan(eng: PnPEngine, times, seg: int, interp: str, omega_max) -> None:
        """make the engine's off-resonance plan the episode's, unless it is the live one"""
        if interp == "ls":
            band = float(omega_max) if seg > 1 else 0.0
            if not eng.offres_ls_planned(times, seg, band):
                eng.offres_plan_ls(times, seg, band)
        elif not eng.offres_planned(times, seg):
            eng.offres_plan(times, seg)

    def _reset_offres(self, data, eng: PnPEngine, x0, y0, sens, dcf, gt, traj, n: int, device) -> "OrderedDict[str, torch.Tensor]":
        """An off-resonance episode: data["omega"] float32 [H,W] or [N,H,W] in rad/s, data["times"] float64 [M] seconds, optional
        data["segments"], optional data["b0_interp"] "linear" | "ls" (the least-squares temporal interpolator over the map's own band,
        max |omega| (1 + 1e-6)); gridding form of the normal operator, or with offres_normal="toeplitz" its Toeplitz form.  Single-coil, unless the env was made with offres_mc=True: then
        data["sens"] beside data["omega"] installs the coils x segments stage (`PnPEngine.reset_offres_mc`), y0 [N,C,M]."""
        if sens is not None and not getattr(self, "offres_mc", False):
            raise ValueError("an off-resonance episode is single-coil (data['omega'] with data['sens'] is not supported)")
        if self.nc_normal == "toeplitz":
            raise ValueError("an off-resonance episode has no Toeplitz normal operator (nc_normal='toeplitz' with data['omega'])")
        times, seg = self._offres_args(data, traj.shape[0])
        omega = torch.as_tensor(data["omega"]).to(device, torch.float32).contiguous()
        interp = self._interp_of(data)
        extra = {} if interp == "linear" else {"b0_interp": interp, "omega_max": float(omega.abs().max()) * (1.0 + 1e-6)}
        self._offres_plan(eng, times, seg, interp, extra.get("omega_max"))
        tz = getattr(self, "offres_normal", "nufft") == "toeplitz"   # (the engine plans the spectra when the plans or the weights changed)
        if sens is not None:
            x, z, u = (eng.reset_offres_mc_tz if tz else eng.reset_offres_mc)(x0, y0, sens, omega, dcf, cg_iters=self.cg_iters)
        else:
            x, z, u = (eng.reset_offres_tz if tz else eng.reset_offres)(x0, y0, omega, dcf, cg_iters=self.cg_iters)
        aty0 = torch.as_tensor(data["ATy0"])[..., 0] if "ATy0" in data else None
        return OrderedDict({"x": x, "y0": y0, "z": z, "u": u, "mask": None, "gt": gt, "ATy0": aty0,
                            "T": torch.zeros(n, dtype=torch.float32, device=device),
                            "complex_y0": data["y0"], "_episode": eng.live_episode, "sens": sens, "traj": traj, "dcf": dcf,
                            "omega": omega, "times": times, "segments": seg, **extra})

    def _bind_episode(self, eng: PnPEngine, states) -> None:
        """Make the engine's k-space constants those of `states` (env.py:88-90 reads y0 / mask from the dict)."""
        ep = states.get("_episode", 0)
        if states.get("traj") is not None and not eng.nufft_planned(states["traj"], self.nufft_grid, self.nufft_width):
            eng.nufft_plan(states["traj"], grid=self.nufft_grid, width=self.nufft_width)      # (drops the live episode)
        if states.get("omega") is not None:                                                   # (a new plan drops a live off-resonance episode)
            self._offres_plan(eng, states["times"], int(states["segments"]), self._interp_of(states), states.get("omega_max"))
        if ep and ep == eng.live_episode:
            return
        if not ep:                              # a state dict built by hand the reference's way
            ep = states["_episode"] = _next_episode()
        n, h, w = eng.n, eng.h, eng.w
        if states.get("traj") is not None:
            tz = self.nc_normal == "toeplitz"   # (the engine re-plans the spectrum when the plan or the episode's weights changed)
            y = states["y0"]
            y = y if y.is_complex() else _as_complex(y)
            otz = getattr(self, "offres_normal", "nufft") == "toeplitz"
            if states.get("omega") is not None and states.get("sens") is not None:      # a multi-coil off-resonance episode
                sens = states["sens"]
                install = eng.set_kspace_offres_mc_tz if otz else eng.set_kspace_offres_mc
                install(y.reshape(n, sens.shape[-3], -1).to(eng.device).contiguous(), sens, states["omega"], states.get("dcf"), episode=ep,
                        cg_iters=self.cg_iters)
                return
            if states.get("omega") is not None:  # an off-resonance episode
                (eng.set_kspace_offres_tz if otz else eng.set_kspace_offres)(y.reshape(n, -1).to(eng.device).contiguous(), states["omega"],
                                                                             states.get("dcf"), episode=ep, cg_iters=self.cg_iters)
                return
            if states.get("sens") is not None:  # a non-Cartesian SENSE episode
                sens = states["sens"]
                y = y.reshape(n, sens.shape[-3], -1).to(eng.device).contiguous()
                (eng.set_kspace_ncsense_tz if tz else eng.set_kspace_ncsense)(y, sens, states.get("dcf"), episode=ep, cg_iters=self.cg_iters)
                return
            (eng.set_kspace_nc_tz if tz else eng.set_kspace_nc)(y.reshape(n, -1).to(eng.device).contiguous(), states.get("dcf"), episode=ep,
                                                                cg_iters=self.cg_iters)
            return
        sens = states.get("sens")
        coils = 1 if sens is None else sens.shape[-3]
        y0 = _as_complex(states["y0"]).reshape(n, coils, h, w).to(eng.device).contiguous()
        mask = torch.as_tensor(states["mask"]).to(eng.device)
        mask = mask.reshape(h, w) if mask.numel() == h * w else mask.reshape(n, h, w)
        eng.set_kspace(y0, mask, episode=ep, sens=sens, cg_iters=self.cg_iters)

    def _param(self, v, n: int, device) -> torch.Tensor:
        t = torch.as_tensor(v, dtype=torch.float32, device=device).reshape(-1)
        if t.numel() == 1 and n > 1:
            t = t.expand(n)
        if t.numel() != n:
            raise ValueError(f"action has {t.numel()} values for {n} slices")
        return t.contiguous()

    def step(self, states: "OrderedDict[str, torch.Tensor]", action_dict) -> Tuple["OrderedDict", object]:
        """env.py:74-100.  Slices with T > 0.5 are done and untouched.  Returns (same dict, done): a Python
        bool for N == 1 like the reference, else a bool tensor [N] (no host sync)."""
        x, z, u = states["x"], states["z"], states["u"]
        n, _, h, w = z.shape
        eng = self._engine if self._engine is not None and (self._engine.n, self._engine.h, self._engine.w) == (n, h, w) \
            else self._engine_for(n, h, w, z.device)
        dev = z.device
        T = self._param(action_dict["T"], n, dev)
        mu = self._param(action_dict["mu"], n, dev)
        sigma_d = self._param(action_dict["sigma_d"], n, dev)
        if x.is_complex():                      # a state built by hand the reference's way
            x = x.real.contiguous()
        done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._bind_episode(eng, states)
        eng.step(x, z, u, mu, sigma_d, t_action=T, t_state=states["T"], done=done)
        states["x"] = x
        if n == 1:
            return states, bool(done.item())
        return states, done.bool()

    @staticmethod
    def get_policy_ob(state) -> torch.Tensor:
        """env.py:102-109: Re(x) flattened, one row per slice."""
        x = state["x"].real
        return x.reshape(x.shape[0], -1)

    def compute_reward(self, x: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """env.py:112-125: PSNR of clamp(Re x, 0, 1) against gt, [N,1] on the CPU like the reference."""
        gt = gt.to(x.device).float()
        h, w = gt.shape[-2:]
        n = gt.numel() // (h * w)
        xr = (x.real if x.is_complex() else x).float().reshape(n, 1, h, w).contiguous()
        eng = self._engine if self._engine is not None and (self._engine.n, self._engine.h, self._engine.w) == (n, h, w) \
            else self._engine_for(n, h, w, x.device)
        return eng.psnr(xr, gt.reshape(n, 1, h, w).contiguous()).reshape(n, 1).cpu()

    def compute_ssim(self, x: torch.Tensor, gt: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
        """SSIM of clamp(Re x, 0, 1) against gt (the image `compute_reward` judges), [N,1] on the CPU: calculate_ssim
        (evaluation/utils/transformations.py:61-95) with the reference's window (win_size 11) and k1, k2, per slice."""
        gt = gt.to(x.device).float()
        h, w = gt.shape[-2:]
        n = gt.numel() // (h * w)
        xr = (x.real if x.is_complex() else x).float().reshape(n, 1, h, w).contiguous()
        eng = self._engine if self._engine is not None and (self._engine.n, self._engine.h, self._engine.w) == (n, h, w) \
            else self._engine_for(n, h, w, x.device)
        return eng.ssim(xr, gt.reshape(n, 1, h, w).contiguous(), data_range=data_range, clamp=True).reshape(n, 1).cpu()

    def run_no_ref_reward(self, state) -> float:
        """env.py:42-54 scored with ARNIQA fetched from the network; here an injected callable
        scorer(x[N,1,H,W]) -> float."""
        if self.no_ref_model is None:
            raise RuntimeError("no-reference scorer not configured: pass no_ref_scorer= to PnPEnv "
                               "(the reference fetches ARNIQA with torch.hub, unavailable offline)")
        return float(self.no_ref_model(state["x"]))

    def residuals(self, states, prev=None, dc: bool = False) -> torch.Tensor:
        """ADMM residuals of `states` on the device: float32 [N, 6], columns `engine.RESIDUAL_COLUMNS` (primal, dx, dz, du, delta,
        dc).  `prev` = what `snapshot` returned for the iterate before the step: the packed form goes straight to the kernel, the
        per-tensor form (row slices, states of another size) is packed first.  dc=True adds the k-space data misfit against the y0 /
        mask of the states' own episode (re-installed first when the engine holds another one's)."""
        x, z, u = states["x"], states["z"], states["u"]
        n, _, h, w = z.shape
        eng = self._engine if self._engine is not None and (self._engine.n, self._engine.h, self._engine.w) == (n, h, w) \
            else self._engine_for(n, h, w, z.device)
        if x.is_complex():
            x = x.real.contiguous()
        packed = None
        if prev is not None:
            if "packed" in prev:
                packed = prev["packed"]
            else:
                for k in ("x", "z", "u"):
                    if prev[k].numel() != states[k].numel():
                        raise ValueError(f"prev['{k}'] has {prev[k].numel()} elements, the states have {states[k].numel()}")
                px = prev["x"].real if prev["x"].is_complex() else prev["x"]
                packed = eng.snapshot(px.float().contiguous(), prev["z"].contiguous(), prev["u"].contiguous())
        if dc:
            self._bind_episode(eng, states)
        return eng.residuals(x.contiguous(), z.contiguous(), u.contiguous(), prev=packed, dc=dc)

    # ---- explicit state copies (the reference rebinds tensors; this engine updates in place) ----
    def snapshot(self, states) -> Dict[str, torch.Tensor]:
        """A node's copy of the iterate.  Whole-batch states of the live engine go through pnp_snapshot into one packed
        device buffer; anything else (row slices, states of another size) is cloned tensor by tensor."""
        e = self._engine
        if (e is not None and states["x"].numel() == e.n * e.h * e.w and states["T"].numel() == e.n
                and states["T"].dtype == torch.float32 and states["T"].is_contiguous()):
            return {"packed": e.snapshot(states["x"], states["z"], states["u"], states["T"])}
        return {k: states[k].clone() for k in ("x", "z", "u", "T")}

    def restore(self, states, snap) -> None:
        if "packed" in snap:
            self._engine.restore(snap["packed"], states["x"], states["z"], states["u"], states["T"])
            return
        for k in ("x", "z", "u", "T"):
            states[k].copy_(snap[k])
