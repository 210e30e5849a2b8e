"""PnPEngine: one handle of libpnpadmm.so bound to torch-ROCm tensors.

torch is used only for device memory and streams; every computation on the hot path is a
HIP kernel behind the C ABI (include/pnpadmm.h)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .weights import flatten_state_dict

RESIDUAL_COLUMNS = _lib.RESIDUAL_COLUMNS


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_episode_counter = 0


def _next_episode() -> int:
    """Process-wide id of one `reset` (one set of k-space constants): states carry it, engines remember the live one."""
    global _episode_counter
    _episode_counter += 1
    return _episode_counter


class PnPEngine:
    """Owns the workspace for N slices of H x W on one GPU.  Not thread-safe; one per process/GPU."""

    def __init__(self, n: int, h: int, w: int, device: Optional[int] = None, profile: bool = False,
                 denoiser: bool = True, keep_stages: bool = False, bf16_convs: bool = False, profile_layers: bool = False):
        if not torch.cuda.is_available():
            raise _lib.PnPError("PnPEngine needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.lib = _lib.load()
        self.n, self.h, self.w = int(n), int(h), int(w)
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        flags = ((_lib.PNP_FLAG_PROFILE if profile else 0) | (0 if denoiser else _lib.PNP_FLAG_NO_DENOISER)
                 | (_lib.PNP_FLAG_KEEP_STAGES if keep_stages else 0) | (_lib.PNP_FLAG_BF16_CONVS if bf16_convs else 0)
                 | (_lib.PNP_FLAG_PROFILE_LAYERS if profile_layers else 0))
        cfg = _lib.pnp_config(self.n, self.h, self.w, self.device_index, flags)
        hnd = C.c_void_p()
        _lib.check(self.lib.pnp_create(C.byref(cfg), C.byref(hnd)), "pnp_create")
        self._h = hnd
        self.profile = profile or profile_layers
        self.bf16_convs = bool(bf16_convs)
        self.live_episode = 0        # id of the reset whose y0 / mask the engine currently holds (0: none)

    def _stream(self) -> int:
        """The caller's current stream ON THE ENGINE'S DEVICE (not on torch's current device)."""
        return torch.cuda.current_stream(self.device).cuda_stream

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------
    def _chk(self, t: torch.Tensor, dtype, numel: int, name: str) -> torch.Tensor:
        if t.device != self.device:
            raise ValueError(f"{name}: expected a tensor on {self.device}, got {t.device}")
        if t.dtype != dtype:
            raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
        if t.numel() != numel:
            raise ValueError(f"{name}: expected {numel} elements, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        return t

    def _iterate(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """fresh (x f32, z c64, u c64) [N,1,H,W] for a reset to fill"""
        x = torch.empty((self.n, 1, self.h, self.w), dtype=torch.float32, device=self.device)
        z = torch.empty((self.n, 1, self.h, self.w), dtype=torch.complex64, device=self.device)
        return x, z, torch.empty_like(z)

    def _mask(self, mask: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """mask bool/uint8 [H,W] or [N,H,W] -> (uint8 tensor, mask_n)"""
        hw = self.h * self.w
        m = mask.to(torch.uint8).contiguous()
        if m.numel() not in (hw, self.n * hw):
            raise ValueError(f"mask: expected {hw} or {self.n * hw} elements, got {tuple(mask.shape)}")
        self._chk(m, torch.uint8, m.numel(), "mask")
        return m, (1 if m.numel() == hw else self.n)

    def _cg_residual(self, fn: str) -> torch.Tensor:
        """float32 [N] from the live stage's pnp_*_cg_residual"""
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _lib.check(getattr(self.lib, fn)(self._h, out.data_ptr(), self._stream()), fn)
        return out

    def _normal(self, fn: str, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = the live stage's pnp_*_normal of p complex64 [N,1,H,W] and mu float32 [N]"""
        self._chk(p, torch.complex64, self.n * self.h * self.w, "p"); self._chk(mu, torch.float32, self.n, "mu")
        q = torch.empty_like(p)
        _lib.check(getattr(self.lib, fn)(self._h, p.data_ptr(), mu.data_ptr(), q.data_ptr(), self._stream()), fn)
        return q

    @property
    def workspace_bytes(self) -> int:
        return int(self.lib.pnp_workspace_bytes(self._h))

    # -- weights ---------------------------------------------------------------------------
    def load_weights(self, state_dict: Mapping[str, object]) -> None:
        """state_dict with the reference's 56 keys (evaluation/noise.py:146-148); tensors or ndarrays."""
        blob = np.ascontiguousarray(flatten_state_dict(state_dict))
        _lib.check(self.lib.pnp_load_unet_weights(self._h, blob.ctypes.data, blob.size), "pnp_load_unet_weights")

    # -- multi-coil helpers ----------------------------------------------------------------
    def _sens(self, sens: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
        """Coil maps complex64 [C,H,W] (shared) or [N,C,H,W] -> (tensor, coils, sens_n)."""
        hw = self.h * self.w
        if sens.dim() not in (3, 4) or tuple(sens.shape[-2:]) != (self.h, self.w) or (sens.dim() == 4 and sens.shape[0] != self.n):
            raise ValueError(f"sens: expected [C,{self.h},{self.w}] or [{self.n},C,{self.h},{self.w}], got {tuple(sens.shape)}")
        coils = int(sens.shape[-3])
        sens = self._chk(sens, torch.complex64, sens.numel(), "sens")
        return sens, coils, (1 if sens.dim() == 3 else self.n)

    @property
    def coils(self) -> int:
        """Coils of the installed multi-coil constants; 0 in single-coil mode."""
        return int(self.lib.pnp_mc_coils(self._h))

    def cg_residual(self) -> torch.Tensor:
        """float32 [N]: the relative residual the CG solve of the last step ended with (pnp_mc_cg_residual; multi-coil mode only)."""
        return self._cg_residual("pnp_mc_cg_residual")

    def normal_op(self, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = A^H A p + mu p with the installed multi-coil constants (pnp_mc_normal); p complex64 [N,1,H,W], mu float32 [N]."""
        return self._normal("pnp_mc_normal", p, mu)

    # -- non-Cartesian sampling ------------------------------------------------------------
    def nufft_plan(self, traj, grid: Optional[Tuple[int, int]] = None, width: int = 6) -> None:
        """Plan the NUFFT pair for one trajectory shared by all slices (pnp_nufft_plan): traj [M,2] = (ky, kx) in cycles per pixel,
        each in [-0.5, 0.5] (array or tensor; taken as float64 on the host); grid = (gh, gw) or None for the smallest accepted
        1.25x grid; width = the kernel width J in {4, 6, 8}.  A new plan replaces the old one and drops non-Cartesian constants."""
        t = np.ascontiguousarray(traj.detach().cpu().numpy() if isinstance(traj, torch.Tensor) else traj, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != 2:
            raise ValueError(f"traj: expected [M,2], got {t.shape}")
        gh, gw = (0, 0) if grid is None else (int(grid[0]), int(grid[1]))
        self._nufft_key = None
        self._tz_weights = None      # the library drops the Toeplitz spectrum with the plan it was built for
        self._offres_key = None      # ... and the off-resonance plan
        _lib.check(self.lib.pnp_nufft_plan(self._h, t.ctypes.data, t.shape[0], gh, gw, int(width), 0), "pnp_nufft_plan")
        self._nufft_key = (t.copy(), gh, gw, int(width), traj)
        self.live_episode = 0        # non-Cartesian constants are dropped with their plan: whoever binds episodes re-installs

    _nufft_key = None            # (a copy of traj, gh, gw, width, the object traj was given as) of the live plan

    def nufft_planned(self, traj, grid: Optional[Tuple[int, int]] = None, width: int = 6) -> bool:
        """Whether the live plan was made from exactly these arguments (so that a caller binding episodes need not re-plan).  The very
        object the plan was made from (an episode's own trajectory tensor, step after step) is recognised without looking at its values."""
        k = self._nufft_key
        if k is not None and k[4] is traj:
            return k[1:4] == ((0, 0) if grid is None else (int(grid[0]), int(grid[1]))) + (int(width),)
        t = np.asarray(traj.detach().cpu().numpy() if isinstance(traj, torch.Tensor) else traj, dtype=np.float64)
        gh, gw = (0, 0) if grid is None else (int(grid[0]), int(grid[1]))
        return k is not None and k[1:4] == (gh, gw, int(width)) and k[0].shape == t.shape and bool(np.array_equal(k[0], t))

    @property
    def nufft_samples(self) -> int:
        """M of the handle's NUFFT plan; 0 without one."""
        return int(self.lib.pnp_nufft_samples(self._h))

    @property
    def nufft_grid(self) -> Tuple[int, int]:
        gh, gw = C.c_int(), C.c_int()
        _lib.check(self.lib.pnp_nufft_grid(self._h, C.byref(gh), C.byref(gw)), "pnp_nufft_grid")
        return gh.value, gw.value

    def _batch_of(self, t: torch.Tensor, per: int, name: str) -> int:
        if per < 1 or t.numel() % per or not 1 <= t.numel() // per <= self.n:
            raise ValueError(f"{name}: expected 1..{self.n} slices of {per} elements, got {tuple(t.shape)}")
        return t.numel() // per

    def nufft_forward(self, img: torch.Tensor) -> torch.Tensor:
        """samples complex64 [B,M] = A img (pnp_nufft_forward); img complex64 [B,H,W] (or [B,1,H,W]), B <= N."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        out = torch.empty((b, self.nufft_samples), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_nufft_forward(self._h, img.data_ptr(), b, out.data_ptr(), self._stream()), "pnp_nufft_forward")
        return out

    def nufft_adjoint(self, samples: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img complex64 [B,H,W] = A^H (weights . samples) (pnp_nufft_adjoint); samples complex64 [B,M], weights float32 [M] or None."""
        m = self.nufft_samples
        b = self._batch_of(samples, m, "samples")
        self._chk(samples, torch.complex64, samples.numel(), "samples")
        if weights is not None:
            self._chk(weights, torch.float32, m, "weights")
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_nufft_adjoint(self._h, samples.data_ptr(), weights.data_ptr() if weights is not None else None, b,
                                              out.data_ptr(), self._stream()), "pnp_nufft_adjoint")
        return out

    def _nc_args(self, y: torch.Tensor, w: Optional[torch.Tensor]):
        m = self.nufft_samples
        self._chk(y, torch.complex64, self.n * m if m else y.numel(), "y")     # without a plan the library reports the state error
        if w is not None:
            self._chk(w, torch.float32, m, "w")
        return y.data_ptr(), (w.data_ptr() if w is not None else None)

    def reset_nc(self, x0: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor] = None,
                 cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Install the non-Cartesian constants (y complex64 [N,M] or [N,1,M], w float32 [M] or None) and start an episode from x0
        complex64 [N,1,H,W] (pnp_reset_nc).  Returns fresh (x f32, z c64, u c64); steps then solve the k-space subproblem by `cg_iters`
        CG iterations on the NUFFT normal operator."""
        return self._install_nc("nc", True, False, x0, y, None, None, w, cg_iters)

    def reset_nc_tz(self, x0: torch.Tensor, y: torch.Tensor, w: Optional[torch.Tensor] = None,
                    cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`reset_nc` with the CG on the Toeplitz form of A^H W A (pnp_reset_nc_tz): the spectrum is planned here when none exists for these
        weights, which are then the weights of aty and of the DC column too."""
        return self._install_nc("nc", True, True, x0, y, None, None, w, cg_iters)

    def _install_nc(self, stem, reset, toeplitz, x0, y, sens, omega, w, cg_iters, episode=0):
        """The twelve installers of the non-Cartesian stages: `reset`: pnp_reset_<stem>[_tz] from x0 (returns the fresh iterate), else
        pnp_set_kspace_<stem>[_tz] for `episode`.  stem "nc", "ncsense" (takes sens), "offres" (takes omega) or "offres_mc" (both); a _tz form
        plans the spectrum of its family for w first and passes no weights."""
        coils, segmented = stem in ("ncsense", "offres_mc"), stem.startswith("offres")
        name = f"pnp_{'reset' if reset else 'set_kspace'}_{stem}{'_tz' if toeplitz else ''}"
        if reset:
            x0 = self._chk(x0, torch.complex64, self.n * self.h * self.w, "x0")
        if coils:
            yp, *mid, wp = self._ncsense_args(y, sens, w)
        else:
            yp, wp = self._nc_args(y, w)
            mid = []
        if segmented:
            omega, map_n = self._omega(omega)
            mid += [omega.data_ptr(), map_n]
        it = self._iterate() if reset else ()
        if toeplitz:
            (self._offres_tz_for if segmented else self._toeplitz_for)(w)
        else:
            mid.append(wp)
        args = ([x0.data_ptr()] if reset else []) + [yp] + mid + [int(cg_iters)] + [t.data_ptr() for t in it]
        _lib.check(getattr(self.lib, name)(self._h, *args, self._stream()), name)
        self.live_episode = _next_episode() if reset else (episode or _next_episode())
        return it

    def _acquire_nc(self, stem, gt, sens, omega, sigma_n, seed, dcf):
        """The four simulated acquisitions of the non-Cartesian stages (pnp_acquire_<stem>, stems as in `_install_nc`): returns (y, aty0, x0)."""
        coils, segmented = stem in ("ncsense", "offres_mc"), stem.startswith("offres")
        name = f"pnp_acquire_{stem}"
        gt = self._chk(gt, torch.float32, self.n * self.h * self.w, "gt")
        mid, lines = [], (self.n,)
        if coils:
            sens, c, sens_n = self._sens(sens)
            mid, lines = [sens.data_ptr(), c, sens_n], (self.n, c)
        if segmented:
            omega, map_n = self._omega(omega)
            mid += [omega.data_ptr(), map_n]
        m = self.nufft_samples
        if dcf is not None:
            self._chk(dcf, torch.float32, m, "dcf")
        y = torch.empty(lines + (max(m, 1),), dtype=torch.complex64, device=self.device)
        aty0 = torch.empty((self.n, 1, self.h, self.w), dtype=torch.complex64, device=self.device)
        x0 = torch.empty_like(aty0)
        _lib.check(getattr(self.lib, name)(self._h, gt.data_ptr(), *mid, _ptr(dcf), float(sigma_n), int(seed) & (2 ** 64 - 1), 0, y.data_ptr(),
                                           aty0.data_ptr(), x0.data_ptr(), self._stream()), name)
        return y, aty0, x0

    def set_kspace_nc(self, y: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0, cg_iters: int = 8) -> None:
        """Re-install the non-Cartesian constants of another episode without touching any iterate (pnp_set_kspace_nc)."""
        self._install_nc("nc", False, False, None, y, None, None, w, cg_iters, episode)

    def set_kspace_nc_tz(self, y: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0, cg_iters: int = 8) -> None:
        """`set_kspace_nc` for an episode whose CG runs the Toeplitz operator (pnp_set_kspace_nc_tz; the spectrum as in `reset_nc_tz`)."""
        self._install_nc("nc", False, True, None, y, None, None, w, cg_iters, episode)

    # -- Toeplitz normal operator (include/pnpadmm_toeplitz.h) ----------------------------------
    _tz_weights = None           # (the weights tensor the live spectrum was planned from, or None for unit weights,)

    def toeplitz_plan(self, weights: Optional[torch.Tensor] = None) -> None:
        """Build the Toeplitz spectrum of A^H W A for the planned trajectory and these weights (pnp_toeplitz_plan): weights float32 [M]
        or None (1).  Replaces an earlier spectrum; a live Toeplitz stage's constants are dropped."""
        if weights is not None:
            self._chk(weights, torch.float32, self.nufft_samples or weights.numel(), "weights")
        was_live = self.toeplitz_live
        self._tz_weights = None
        _lib.check(self.lib.pnp_toeplitz_plan(self._h, weights.data_ptr() if weights is not None else None, 0, self._stream()),
                   "pnp_toeplitz_plan")
        self._tz_weights = (weights.clone() if weights is not None else None,)
        if was_live:
            self.live_episode = 0    # dropped with the spectrum: whoever binds episodes re-installs

    def _toeplitz_for(self, w: Optional[torch.Tensor]) -> None:
        """plan the spectrum unless the live one was planned from these very weights"""
        k = self._tz_weights
        if k is not None and self.toeplitz_planned:
            if (k[0] is None and w is None) or (k[0] is not None and w is not None and k[0].shape == w.shape and torch.equal(k[0], w)):
                return
        self.toeplitz_plan(w)

    @property
    def toeplitz_planned(self) -> bool:
        """Whether a Toeplitz spectrum exists for the handle's NUFFT plan."""
        return bool(self.lib.pnp_toeplitz_planned(self._h))

    @property
    def toeplitz_live(self) -> bool:
        """Whether the live stage's CG runs the Toeplitz operator."""
        return bool(self.lib.pnp_toeplitz_live(self._h))

    def toeplitz_spectrum(self) -> torch.Tensor:
        """float32 [2H,2W]: the spectrum K, centred like `fft2c`'s output (pnp_toeplitz_spectrum)."""
        out = torch.empty((2 * self.h, 2 * self.w), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnp_toeplitz_spectrum(self._h, out.data_ptr(), self._stream()), "pnp_toeplitz_spectrum")
        return out

    def toeplitz_apply(self, img: torch.Tensor) -> torch.Tensor:
        """complex64 [B,H,W] = A^H W A img by the Toeplitz form, without mu (pnp_toeplitz_apply); img complex64 [B,H,W] (or [B,1,H,W])."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_toeplitz_apply(self._h, img.data_ptr(), b, out.data_ptr(), self._stream()), "pnp_toeplitz_apply")
        return out

    def toeplitz_apply_mc(self, img: torch.Tensor, sens: torch.Tensor) -> torch.Tensor:
        """complex64 [B,H,W] = sum_c conj(S_c) . Toep(S_c . img) (pnp_toeplitz_apply_mc); sens complex64 [C,H,W] or [N,C,H,W]."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        sens, coils, sens_n = self._sens(sens)
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_toeplitz_apply_mc(self._h, img.data_ptr(), sens.data_ptr(), coils, sens_n, b, out.data_ptr(), self._stream()),
                   "pnp_toeplitz_apply_mc")
        return out

    # -- density compensation (include/pnpadmm_dcf.h) ------------------------------------------
    def _positive(self, w: torch.Tensor, name: str) -> torch.Tensor:
        """float32 [M] weights that are positive and finite (one read-back: a setup-time check; the library reads any other entry as 1)"""
        self._chk(w, torch.float32, self.nufft_samples or w.numel(), name)
        if not bool(((w > 0) & torch.isfinite(w)).all()):
            raise ValueError(f"{name}: every weight must be positive and finite")
        return w

    def nufft_psi(self, w: torch.Tensor) -> torch.Tensor:
        """float32 [M] = Psi w, Psi = G G^T with G the planned gridding kernel, evaluated in float64 (pnp_nufft_psi); w float32 [M],
        positive and finite (ValueError otherwise)."""
        self._positive(w, "w")
        out = torch.empty(w.numel(), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnp_nufft_psi(self._h, w.data_ptr(), out.data_ptr(), self._stream()), "pnp_nufft_psi")
        return out

    def nufft_dcf(self, iters: int = 30, w0: Optional[torch.Tensor] = None, return_info: bool = False):
        """float32 [M]: density weights of the planned trajectory by `iters` (1..256) Pipe-Menon iterations w <- w / (Psi w) from w0 (float32
        [M], positive and finite - ValueError otherwise - or None: ones), scaled to sum h w (pnp_nufft_dcf).  return_info: (w, info) with
        info float32 [iters + 1] = max |Psi w - 1| before each iteration and after the last."""
        iters = int(iters)
        if w0 is not None:
            self._positive(w0, "w0")
        w = torch.empty(max(self.nufft_samples, 1), dtype=torch.float32, device=self.device)
        info = torch.empty(max(iters, 0) + 1, dtype=torch.float32, device=self.device) if return_info else None
        _lib.check(self.lib.pnp_nufft_dcf(self._h, _ptr(w0), iters, 0, w.data_ptr(), _ptr(info), self._stream()), "pnp_nufft_dcf")
        return (w, info) if return_info else w

    def nc_normal(self, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = A^H W A p + mu p with the installed non-Cartesian constants (pnp_nc_normal); p complex64 [N,1,H,W], mu float32 [N]."""
        return self._normal("pnp_nc_normal", p, mu)

    def nc_cg_residual(self) -> torch.Tensor:
        """float32 [N]: the relative residual the CG solve of the last step ended with (pnp_nc_cg_residual; non-Cartesian mode only)."""
        return self._cg_residual("pnp_nc_cg_residual")

    def acquire_nc(self, gt: torch.Tensor, sigma_n: float, seed: int,
                   dcf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Simulated non-Cartesian acquisition on the planned trajectory (pnp_acquire_nc): gt float32 [N,1,H,W]; returns
        (y complex64 [N,M], aty0 = A^H (dcf . y) complex64 [N,1,H,W], x0 = max(aty0, 0))."""
        return self._acquire_nc("nc", gt, None, None, sigma_n, seed, dcf)

    # -- non-Cartesian SENSE (include/pnpadmm_ncsense.h) --------------------------------------
    @property
    def ncsense_coils(self) -> int:
        """Coils of the installed non-Cartesian SENSE constants; 0 unless that mode is live."""
        return int(self.lib.pnp_ncsense_coils(self._h))

    def nufft_forward_mc(self, img: torch.Tensor, sens: torch.Tensor) -> torch.Tensor:
        """samples complex64 [B,C,M] = [F_nu(S_c . img)]_c (pnp_nufft_forward_mc); img complex64 [B,H,W] (or [B,1,H,W]), B <= N; sens
        complex64 [C,H,W] or [N,C,H,W]."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        sens, coils, sens_n = self._sens(sens)
        out = torch.empty((b, coils, max(self.nufft_samples, 1)), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_nufft_forward_mc(self._h, img.data_ptr(), sens.data_ptr(), coils, sens_n, b, out.data_ptr(), self._stream()),
                   "pnp_nufft_forward_mc")
        return out

    def nufft_adjoint_mc(self, samples: torch.Tensor, sens: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img complex64 [B,H,W] = sum_c conj(S_c) . F_nu^H(weights . samples_c) (pnp_nufft_adjoint_mc); samples complex64 [B,C,M], weights
        float32 [M] or None."""
        m = self.nufft_samples
        sens, coils, sens_n = self._sens(sens)
        b = self._batch_of(samples, coils * m, "samples")
        self._chk(samples, torch.complex64, samples.numel(), "samples")
        if weights is not None:
            self._chk(weights, torch.float32, m, "weights")
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_nufft_adjoint_mc(self._h, samples.data_ptr(), weights.data_ptr() if weights is not None else None,
                                                 sens.data_ptr(), coils, sens_n, b, out.data_ptr(), self._stream()), "pnp_nufft_adjoint_mc")
        return out

    def _ncsense_args(self, y: torch.Tensor, sens: torch.Tensor, w: Optional[torch.Tensor]):
        m = self.nufft_samples
        sens, coils, sens_n = self._sens(sens)
        self._chk(y, torch.complex64, self.n * coils * m if m else y.numel(), "y")     # without a plan the library reports the state error
        if w is not None:
            self._chk(w, torch.float32, m, "w")
        return y.data_ptr(), sens.data_ptr(), coils, sens_n, (w.data_ptr() if w is not None else None)

    def reset_ncsense(self, x0: torch.Tensor, y: torch.Tensor, sens: torch.Tensor, w: Optional[torch.Tensor] = None,
                      cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Install the non-Cartesian SENSE constants (y complex64 [N,C,M], sens complex64 [C,H,W] or [N,C,H,W], w float32 [M] or None) and
        start an episode from x0 complex64 [N,1,H,W] (pnp_reset_ncsense).  Returns fresh (x f32, z c64, u c64); steps then solve the
        k-space subproblem by `cg_iters` CG iterations on A^H W A + mu I, A p = [F_nu(S_c . p)]_c."""
        return self._install_nc("ncsense", True, False, x0, y, sens, None, w, cg_iters)

    def reset_ncsense_tz(self, x0: torch.Tensor, y: torch.Tensor, sens: torch.Tensor, w: Optional[torch.Tensor] = None,
                         cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`reset_ncsense` with the CG on the Toeplitz form of each coil's A^H W A (pnp_reset_ncsense_tz; the spectrum as in `reset_nc_tz`)."""
        return self._install_nc("ncsense", True, True, x0, y, sens, None, w, cg_iters)


    def set_kspace_ncsense(self, y: torch.Tensor, sens: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0,
                           cg_iters: int = 8) -> None:
        """Re-install the non-Cartesian SENSE constants of another episode without touching any iterate (pnp_set_kspace_ncsense)."""
        self._install_nc("ncsense", False, False, None, y, sens, None, w, cg_iters, episode)

    def set_kspace_ncsense_tz(self, y: torch.Tensor, sens: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0,
                              cg_iters: int = 8) -> None:
        """`set_kspace_ncsense` for an episode whose CG runs the Toeplitz operator (pnp_set_kspace_ncsense_tz)."""
        self._install_nc("ncsense", False, True, None, y, sens, None, w, cg_iters, episode)


    def ncsense_normal(self, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = A^H W A p + mu p with the installed non-Cartesian SENSE constants (pnp_ncsense_normal); p complex64 [N,1,H,W], mu float32 [N]."""
        return self._normal("pnp_ncsense_normal", p, mu)

    def ncsense_cg_residual(self) -> torch.Tensor:
        """float32 [N]: the relative residual the CG solve of the last step ended with (pnp_ncsense_cg_residual; that mode only)."""
        return self._cg_residual("pnp_ncsense_cg_residual")

    def acquire_ncsense(self, gt: torch.Tensor, sens: torch.Tensor, sigma_n: float, seed: int,
                        dcf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Simulated multi-coil acquisition on the planned trajectory (pnp_acquire_ncsense): gt float32 [N,1,H,W]; returns
        (y complex64 [N,C,M], aty0 = A^H (dcf . y) complex64 [N,1,H,W], x0 = max(aty0, 0))."""
        return self._acquire_nc("ncsense", gt, sens, None, sigma_n, seed, dcf)

    # -- off-resonance correction (include/pnpadmm_offres.h) ------------------------------------
    def offres_plan(self, times, segments: int) -> None:
        """Plan the time-segmented off-resonance operator on the live NUFFT plan (pnp_offres_plan): times [M] seconds, one per trajectory
        sample (array or tensor; taken as float64 on the host), segments = L in 1..32.  Replaces an earlier off-resonance plan and drops a
        live off-resonance stage; `nufft_plan` drops this plan."""
        t = np.ascontiguousarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        m = self.nufft_samples
        if m and t.size != m:
            raise ValueError(f"times: expected {m} samples, got {t.shape}")
        if self.offres_live or self.offres_mc_coils:
            self.live_episode = 0
        self._offres_key = None
        _lib.check(self.lib.pnp_offres_plan(self._h, t.ctypes.data, int(segments), 0), "pnp_offres_plan")
        self._offres_key = (t.copy(), int(segments))

    _offres_key = None           # (a copy of times, segments[, omega_max: a least-squares plan]) of the live off-resonance plan

    def offres_plan_ls(self, times, segments: int, omega_max: float) -> None:
        """Plan the off-resonance operator with the least-squares temporal interpolator (pnp_offres_plan_ls, include/pnpadmm_offres_ls.h):
        as `offres_plan`, with one coefficient per (segment, sample) fitted over the band |omega| <= omega_max (rad/s).  Replaces an earlier
        off-resonance plan of either kind; `offres_plan` and `nufft_plan` replace / drop this one."""
        t = np.ascontiguousarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        m = self.nufft_samples
        if m and t.size != m:
            raise ValueError(f"times: expected {m} samples, got {t.shape}")
        if self.offres_live or self.offres_mc_coils:
            self.live_episode = 0
        self._offres_key = None
        _lib.check(self.lib.pnp_offres_plan_ls(self._h, t.ctypes.data, int(segments), float(omega_max), 0), "pnp_offres_plan_ls")
        self._offres_key = (t.copy(), int(segments), float(omega_max))

    def offres_ls_planned(self, times, segments: int, omega_max: float) -> bool:
        """Whether the live off-resonance plan is the least-squares plan of exactly these times, segments and omega_max."""
        k = self._offres_key
        if k is None or len(k) != 3 or self.offres_interpolator() != "ls" or self.offres_segments != int(segments) or k[1] != int(segments):
            return False
        t = np.asarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        return k[2] == float(omega_max) and k[0].shape == t.shape and bool(np.array_equal(k[0], t))

    def offres_interpolator(self) -> Optional[str]:
        """"linear" or "ls": the temporal interpolator of the live off-resonance plan (pnp_offres_interpolator); None without a plan."""
        return {1: "linear", 2: "ls"}.get(int(self.lib.pnp_offres_interpolator(self._h)))

    def offres_ls_coeffs(self) -> np.ndarray:
        """float32 [L, M]: the coefficient table of the live least-squares plan, copied back from the device (pnp_offres_ls_coeffs)."""
        out = np.empty((max(self.offres_segments, 1), max(self.nufft_samples, 1)), dtype=np.float32)
        _lib.check(self.lib.pnp_offres_ls_coeffs(self._h, out.ctypes.data), "pnp_offres_ls_coeffs")
        return out

    def offres_planned(self, times, segments: int) -> bool:
        """Whether the live off-resonance plan was made from exactly these times and segments on the live NUFFT plan."""
        k = self._offres_key
        if k is None or len(k) != 2 or self.offres_segments != int(segments) or k[1] != int(segments):   # (pnp_nufft_plan drops the plan: 0 segments)
            return False
        t = np.asarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64).reshape(-1)
        return k[0].shape == t.shape and bool(np.array_equal(k[0], t))

    @property
    def offres_segments(self) -> int:
        """L of the handle's off-resonance plan; 0 without one."""
        return int(self.lib.pnp_offres_segments(self._h))

    @property
    def offres_live(self) -> bool:
        """Whether the live data-fidelity stage is the off-resonance one."""
        return bool(self.lib.pnp_offres_live(self._h))

    def _omega(self, omega: torch.Tensor, name: str = "omega") -> Tuple[torch.Tensor, int]:
        """Field map float32 [H,W] (shared) or [N,H,W] in rad/s -> (tensor, map_n)."""
        hw = self.h * self.w
        if omega.numel() not in (hw, self.n * hw):
            raise ValueError(f"{name}: expected {hw} or {self.n * hw} elements, got {tuple(omega.shape)}")
        self._chk(omega, torch.float32, omega.numel(), name)
        return omega, (1 if omega.numel() == hw and (self.n > 1 or omega.dim() < 3) else self.n)

    def _offres_maps_arg(self, maps: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """Segment maps complex64 [L,H,W] (shared) or [N,L,H,W] -> (tensor, map_n)."""
        per = max(self.offres_segments, 1) * self.h * self.w
        if maps.numel() not in (per, self.n * per):
            raise ValueError(f"maps: expected {per} or {self.n * per} elements, got {tuple(maps.shape)}")
        self._chk(maps, torch.complex64, maps.numel(), "maps")
        return maps, (1 if maps.numel() == per and (self.n > 1 or maps.dim() < 4) else self.n)

    def offres_maps(self, omega: torch.Tensor) -> torch.Tensor:
        """E_l = exp(-i omega tau_l), complex64 [L,H,W] for a shared map omega float32 [H,W], [N,L,H,W] for [N,H,W] (pnp_offres_maps)."""
        omega, map_n = self._omega(omega)
        shape = (self.offres_segments, self.h, self.w)
        maps = torch.empty(shape if map_n == 1 and omega.dim() < 3 else (map_n,) + shape, dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_maps(self._h, omega.data_ptr(), map_n, maps.data_ptr(), self._stream()), "pnp_offres_maps")
        return maps

    def offres_forward(self, img: torch.Tensor, maps: torch.Tensor) -> torch.Tensor:
        """samples complex64 [B,M] = the segmented A img (pnp_offres_forward); img complex64 [B,H,W] (or [B,1,H,W]), B <= N; maps from
        `offres_maps`."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        maps, map_n = self._offres_maps_arg(maps)
        out = torch.empty((b, max(self.nufft_samples, 1)), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_forward(self._h, img.data_ptr(), maps.data_ptr(), map_n, b, out.data_ptr(), self._stream()),
                   "pnp_offres_forward")
        return out

    def offres_adjoint(self, samples: torch.Tensor, maps: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img complex64 [B,H,W] = sum_l conj(E_l) . F_nu^H(weights . b_l . samples) (pnp_offres_adjoint); samples complex64 [B,M], weights
        float32 [M] or None."""
        m = self.nufft_samples
        b = self._batch_of(samples, m, "samples")
        self._chk(samples, torch.complex64, samples.numel(), "samples")
        maps, map_n = self._offres_maps_arg(maps)
        if weights is not None:
            self._chk(weights, torch.float32, m, "weights")
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_adjoint(self._h, samples.data_ptr(), weights.data_ptr() if weights is not None else None, maps.data_ptr(),
                                               map_n, b, out.data_ptr(), self._stream()), "pnp_offres_adjoint")
        return out

    def reset_offres(self, x0: torch.Tensor, y: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                     cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Install the off-resonance constants (y complex64 [N,M], omega float32 [H,W] or [N,H,W] in rad/s, w float32 [M] or None) and start an
        episode from x0 complex64 [N,1,H,W] (pnp_reset_offres).  Returns fresh (x f32, z c64, u c64); steps then solve the k-space subproblem
        by `cg_iters` CG iterations on A^H W A + mu I with the time-segmented A."""
        return self._install_nc("offres", True, False, x0, y, None, omega, w, cg_iters)

    def set_kspace_offres(self, y: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0,
                          cg_iters: int = 8) -> None:
        """Re-install the off-resonance constants of another episode without touching any iterate (pnp_set_kspace_offres)."""
        self._install_nc("offres", False, False, None, y, None, omega, w, cg_iters, episode)

    def offres_normal(self, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = A^H W A p + mu p with the installed off-resonance constants (pnp_offres_normal); p complex64 [N,1,H,W], mu float32 [N]."""
        return self._normal("pnp_offres_normal", p, mu)

    def offres_cg_residual(self) -> torch.Tensor:
        """float32 [N]: the relative residual the CG solve of the last step ended with (pnp_offres_cg_residual; that mode only)."""
        return self._cg_residual("pnp_offres_cg_residual")

    def acquire_offres(self, gt: torch.Tensor, omega: torch.Tensor, sigma_n: float, seed: int,
                       dcf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Simulated acquisition under the field map on the planned trajectory and times (pnp_acquire_offres): gt float32 [N,1,H,W]; returns
        (y complex64 [N,M], aty0 = A^H (dcf . y) complex64 [N,1,H,W], x0 = max(aty0, 0))."""
        return self._acquire_nc("offres", gt, None, omega, sigma_n, seed, dcf)

    # -- off-resonance correction for multi-coil data (include/pnpadmm_offres_mc.h) -----------
    @property
    def offres_mc_coils(self) -> int:
        """Coils of the live multi-coil off-resonance stage (pnp_offres_mc_coils); 0 while another stage is live."""
        return int(self.lib.pnp_offres_mc_coils(self._h))

    def offres_forward_mc(self, img: torch.Tensor, maps: torch.Tensor, sens: torch.Tensor) -> torch.Tensor:
        """samples complex64 [B,C,M] = [sum_l b_l F_nu(E_l . S_c . img)]_c (pnp_offres_forward_mc) on the live off-resonance plan, linear or
        least squares; img complex64 [B,H,W] (or [B,1,H,W]), B <= N; maps from `offres_maps`; sens complex64 [C,H,W] or [N,C,H,W]."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        maps, map_n = self._offres_maps_arg(maps)
        sens, coils, sens_n = self._sens(sens)
        out = torch.empty((b, coils, max(self.nufft_samples, 1)), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_forward_mc(self._h, img.data_ptr(), maps.data_ptr(), map_n, sens.data_ptr(), sens_n, coils, b,
                                                  out.data_ptr(), self._stream()), "pnp_offres_forward_mc")
        return out

    def offres_adjoint_mc(self, samples: torch.Tensor, maps: torch.Tensor, sens: torch.Tensor,
                          weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img complex64 [B,H,W] = sum_c conj(S_c) . sum_l conj(E_l) . F_nu^H(weights . b_l . samples_c) (pnp_offres_adjoint_mc); samples
        complex64 [B,C,M], weights float32 [M] or None."""
        m = self.nufft_samples
        maps, map_n = self._offres_maps_arg(maps)
        sens, coils, sens_n = self._sens(sens)
        b = self._batch_of(samples, coils * m, "samples")
        self._chk(samples, torch.complex64, samples.numel(), "samples")
        if weights is not None:
            self._chk(weights, torch.float32, m, "weights")
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_adjoint_mc(self._h, samples.data_ptr(), weights.data_ptr() if weights is not None else None,
                                                  maps.data_ptr(), map_n, sens.data_ptr(), sens_n, coils, b, out.data_ptr(), self._stream()),
                   "pnp_offres_adjoint_mc")
        return out

    def reset_offres_mc(self, x0: torch.Tensor, y: torch.Tensor, sens: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                        cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Install the multi-coil off-resonance constants (y complex64 [N,C,M], sens complex64 [C,H,W] or [N,C,H,W], omega float32 [H,W] or
        [N,H,W] in rad/s, w float32 [M] or None) and start an episode from x0 complex64 [N,1,H,W] (pnp_reset_offres_mc).  Returns fresh
        (x f32, z c64, u c64); steps then solve the k-space subproblem by `cg_iters` CG iterations on A^H W A + mu I with the coils times
        segments operator A."""
        return self._install_nc("offres_mc", True, False, x0, y, sens, omega, w, cg_iters)

    def set_kspace_offres_mc(self, y: torch.Tensor, sens: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                             episode: int = 0, cg_iters: int = 8) -> None:
        """Re-install the multi-coil off-resonance constants of another episode without touching any iterate (pnp_set_kspace_offres_mc)."""
        self._install_nc("offres_mc", False, False, None, y, sens, omega, w, cg_iters, episode)

    def offres_mc_normal(self, p: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """q = A^H W A p + mu p with the installed multi-coil off-resonance constants (pnp_offres_mc_normal); p complex64 [N,1,H,W], mu
        float32 [N]."""
        return self._normal("pnp_offres_mc_normal", p, mu)

    def offres_mc_cg_residual(self) -> torch.Tensor:
        """float32 [N]: the relative residual the CG solve of the last step ended with (pnp_offres_mc_cg_residual; that mode only)."""
        return self._cg_residual("pnp_offres_mc_cg_residual")

    def acquire_offres_mc(self, gt: torch.Tensor, sens: torch.Tensor, omega: torch.Tensor, sigma_n: float, seed: int,
                          dcf: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Simulated multi-coil acquisition under the field map on the planned trajectory and times (pnp_acquire_offres_mc): gt float32
        [N,1,H,W]; returns (y complex64 [N,C,M], aty0 = A^H (dcf . y) complex64 [N,1,H,W], x0 = max(aty0, 0))."""
        return self._acquire_nc("offres_mc", gt, sens, omega, sigma_n, seed, dcf)

    # -- Toeplitz form of the off-resonance operator (include/pnpadmm_offres_tz.h) -------------
    _otz_weights = None          # (the weights tensor the live spectra were planned from, or None for unit weights,)

    def offres_tz_plan(self, weights: Optional[torch.Tensor] = None) -> None:
        """Build the Toeplitz spectra of A^H W A for the planned trajectory, the live off-resonance plan (linear or least squares) and these
        weights (pnp_offres_tz_plan): weights float32 [M] or None (1).  Replaces earlier spectra; a live Toeplitz off-resonance stage's
        constants are dropped.  `nufft_plan`, `offres_plan` and `offres_plan_ls` drop the spectra."""
        if weights is not None:
            self._chk(weights, torch.float32, self.nufft_samples or weights.numel(), "weights")
        was_live = self.offres_tz_live
        self._otz_weights = None
        _lib.check(self.lib.pnp_offres_tz_plan(self._h, weights.data_ptr() if weights is not None else None, 0, self._stream()),
                   "pnp_offres_tz_plan")
        self._otz_weights = (weights.clone() if weights is not None else None,)
        if was_live:
            self.live_episode = 0    # dropped with the spectra: whoever binds episodes re-installs

    def _offres_tz_for(self, w: Optional[torch.Tensor]) -> None:
        """plan the spectra unless the live ones were planned from these very weights on the live plans (the library forgets them when
        either plan is replaced)"""
        k = self._otz_weights
        if k is not None and self.offres_tz_planned:
            if (k[0] is None and w is None) or (k[0] is not None and w is not None and k[0].shape == w.shape and torch.equal(k[0], w)):
                return
        self.offres_tz_plan(w)

    @property
    def offres_tz_planned(self) -> bool:
        """Whether Toeplitz spectra exist for the handle's NUFFT plan and off-resonance plan."""
        return bool(self.lib.pnp_offres_tz_planned(self._h))

    @property
    def offres_tz_live(self) -> bool:
        """Whether the live stage's CG runs the Toeplitz form of the off-resonance operator."""
        return bool(self.lib.pnp_offres_tz_live(self._h))

    @property
    def offres_tz_spectra(self) -> int:
        """P, the number of stored spectra (2L - 1 under a linear plan, L (L + 1) / 2 under least squares); 0 without them."""
        return int(self.lib.pnp_offres_tz_spectra(self._h))

    def offres_tz_spectrum(self) -> torch.Tensor:
        """float32 [P,2H,2W]: the spectra K_ll', each centred like `fft2c`'s output (pnp_offres_tz_spectrum); the pair order is the upper
        triangle row by row under least squares and (l, l), (l, l+1) interleaved under a linear plan."""
        out = torch.empty((max(self.offres_tz_spectra, 1), 2 * self.h, 2 * self.w), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnp_offres_tz_spectrum(self._h, out.data_ptr(), self._stream()), "pnp_offres_tz_spectrum")
        return out

    def offres_tz_apply(self, img: torch.Tensor, maps: torch.Tensor) -> torch.Tensor:
        """complex64 [B,H,W] = A^H W A img of the segmented model by its Toeplitz form, without mu (pnp_offres_tz_apply); img complex64
        [B,H,W] (or [B,1,H,W]); maps from `offres_maps`."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        maps, map_n = self._offres_maps_arg(maps)
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_tz_apply(self._h, img.data_ptr(), maps.data_ptr(), map_n, b, out.data_ptr(), self._stream()),
                   "pnp_offres_tz_apply")
        return out

    def offres_tz_apply_mc(self, img: torch.Tensor, maps: torch.Tensor, sens: torch.Tensor) -> torch.Tensor:
        """complex64 [B,H,W] = sum_c conj(S_c) . [offres_tz_apply](S_c . img) (pnp_offres_tz_apply_mc); sens complex64 [C,H,W] or [N,C,H,W]."""
        b = self._batch_of(img, self.h * self.w, "img")
        self._chk(img, torch.complex64, img.numel(), "img")
        maps, map_n = self._offres_maps_arg(maps)
        sens, coils, sens_n = self._sens(sens)
        out = torch.empty((b, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_offres_tz_apply_mc(self._h, img.data_ptr(), maps.data_ptr(), map_n, sens.data_ptr(), sens_n, coils, b,
                                                   out.data_ptr(), self._stream()), "pnp_offres_tz_apply_mc")
        return out

    def reset_offres_tz(self, x0: torch.Tensor, y: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                        cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`reset_offres` with the CG on the Toeplitz form of A^H W A (pnp_reset_offres_tz): the spectra are planned here when none exist
        for these weights and the live plans; the weights are then those of aty and of the DC column too."""
        return self._install_nc("offres", True, True, x0, y, None, omega, w, cg_iters)

    def set_kspace_offres_tz(self, y: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None, episode: int = 0,
                             cg_iters: int = 8) -> None:
        """`set_kspace_offres` for an episode whose CG runs the Toeplitz form (pnp_set_kspace_offres_tz; the spectra as in `reset_offres_tz`)."""
        self._install_nc("offres", False, True, None, y, None, omega, w, cg_iters, episode)

    def reset_offres_mc_tz(self, x0: torch.Tensor, y: torch.Tensor, sens: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                           cg_iters: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """`reset_offres_mc` with the CG on the Toeplitz form of A^H W A (pnp_reset_offres_mc_tz; the spectra as in `reset_offres_tz`)."""
        return self._install_nc("offres_mc", True, True, x0, y, sens, omega, w, cg_iters)

    def set_kspace_offres_mc_tz(self, y: torch.Tensor, sens: torch.Tensor, omega: torch.Tensor, w: Optional[torch.Tensor] = None,
                                episode: int = 0, cg_iters: int = 8) -> None:
        """`set_kspace_offres_mc` for an episode whose CG runs the Toeplitz form (pnp_set_kspace_offres_mc_tz)."""
        self._install_nc("offres_mc", False, True, None, y, sens, omega, w, cg_iters, episode)

    # -- field map estimation (include/pnpadmm_fieldmap.h) ----------------------------------
    def _echoes(self, x1: torch.Tensor, x2: torch.Tensor) -> int:
        """the coil count of two echo images complex64 [N,C,H,W] (or [N,H,W]: one coil)"""
        per = self.n * self.h * self.w
        if x1.numel() == 0 or x1.numel() % per or x1.numel() // per > _lib.PNP_MC_MAX_COILS:
            raise ValueError(f"x1: expected [{self.n},C,{self.h},{self.w}] with C = 1..{_lib.PNP_MC_MAX_COILS}, got {tuple(x1.shape)}")
        self._chk(x1, torch.complex64, x1.numel(), "x1")
        self._chk(x2, torch.complex64, x1.numel(), "x2")
        return x1.numel() // per

    def fieldmap_estimate(self, x1: torch.Tensor, x2: torch.Tensor, dte: float, beta: float = 0.05, iters: int = 200,
                          return_weight: bool = False):
        """float32 [N,H,W] rad/s: the field map of two echo images x1, x2 (complex64 [N,C,H,W], taken `dte` seconds apart) by the regularised
        fit of pnp_fieldmap_estimate - `iters` (0..4096) Jacobi sweeps of the separable quadratic surrogate at roughness weight `beta`;
        iters = 0 is the raw phase difference.  No phase unwrapping: valid for |omega| dte < pi.  The result is what `reset_offres` takes as
        its per-slice omega.  return_weight: (omega, weight) with the normalised magnitude weights float32 [N,H,W]."""
        coils = self._echoes(x1, x2)
        omega = torch.empty((self.n, self.h, self.w), dtype=torch.float32, device=self.device)
        weight = torch.empty_like(omega) if return_weight else None
        _lib.check(self.lib.pnp_fieldmap_estimate(self._h, x1.data_ptr(), x2.data_ptr(), coils, float(dte), float(beta), int(iters), 0,
                                                  omega.data_ptr(), _ptr(weight), self._stream()), "pnp_fieldmap_estimate")
        return (omega, weight) if return_weight else omega

    def fieldmap_cost(self, x1: torch.Tensor, x2: torch.Tensor, dte: float, beta: float, omega: torch.Tensor) -> torch.Tensor:
        """float64 [N]: the cost Psi of pnpadmm_fieldmap.h at omega (float32 [N,H,W] rad/s) for the echo images x1, x2: the reference-free
        convergence figure of `fieldmap_estimate` (pnp_fieldmap_cost)."""
        coils = self._echoes(x1, x2)
        self._chk(omega, torch.float32, self.n * self.h * self.w, "omega")
        cost = torch.empty(self.n, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.pnp_fieldmap_cost(self._h, x1.data_ptr(), x2.data_ptr(), coils, float(dte), float(beta), omega.data_ptr(),
                                              cost.data_ptr(), self._stream()), "pnp_fieldmap_cost")
        return cost

    # -- hot path --------------------------------------------------------------------------
    def _offres_for(self, times, segments, interpolator: str = "linear", omega_max: Optional[float] = None,
                    omega: Optional[torch.Tensor] = None) -> None:
        """the off-resonance plan of `reset` / `set_kspace` with omega: planned here when times are given and differ from the live plan's.
        interpolator "ls": the least-squares plan over |omega| <= omega_max, by default max |omega| (1 + 1e-6) of the map in hand; a map
        that exceeds a given omega_max is refused (the library does not detect it)."""
        if interpolator not in _lib.OFFRES_INTERPOLATORS:
            raise ValueError(f"interpolator must be one of {sorted(_lib.OFFRES_INTERPOLATORS)} (got {interpolator!r})")
        if interpolator == "linear":
            if omega_max is not None:
                raise ValueError("omega_max goes with interpolator='ls'")
        elif omega is not None:
            top = float(omega.abs().max())
            if omega_max is None:
                omega_max = top * (1.0 + 1e-6)
            elif top > float(omega_max):
                raise ValueError(f"the field map reaches {top:g} rad/s, outside the band omega_max = {float(omega_max):g} of the least-squares plan")
        if times is None:
            if interpolator == "ls" and self.offres_interpolator() != "ls":
                raise ValueError("interpolator='ls' without times needs a live least-squares plan (offres_plan_ls)")
            return
        if segments is None:
            raise ValueError("times needs segments (acquisition.offres_segments chooses them)")
        if interpolator == "ls":
            if omega_max is None:
                raise ValueError("interpolator='ls' needs omega_max or a field map")
            if int(segments) == 1:
                omega_max = 0.0                                  # one centre: the band is not read
            if not self.offres_ls_planned(times, segments, omega_max):
                self.offres_plan_ls(times, segments, omega_max)
        elif not self.offres_planned(times, segments):
            self.offres_plan(times, segments)

    def reset(self, x0: torch.Tensor, y0: torch.Tensor, mask: Optional[torch.Tensor] = None, sens: Optional[torch.Tensor] = None,
              cg_iters: int = 8, omega: Optional[torch.Tensor] = None, times=None, segments: Optional[int] = None,
              w: Optional[torch.Tensor] = None, interpolator: str = "linear",
              omega_max: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """x0, y0 complex64 [N,1,H,W]; mask bool/uint8 [H,W] (or [N,H,W]).  Returns fresh (x f32, z c64, u c64).
        With sens (complex64 [C,H,W] or [N,C,H,W]) y0 is [N,C,H,W] and the handle enters multi-coil mode (pnp_reset_mc): the k-space
        subproblem is then solved by `cg_iters` conjugate-gradient iterations per step.
        With omega (field map, float32 [H,W] or [N,H,W] in rad/s) the episode is the off-resonance one on the planned trajectory
        (`reset_offres`): y0 is the samples [N,M], mask is not read, w float32 [M] or None are the sample weights; times with segments plan
        the time segments first (`offres_plan`) unless the live plan is that one; interpolator "ls" plans the least-squares interpolator
        instead (`offres_plan_ls`), over omega_max or, by default, the map's own max |omega| (1 + 1e-6)."""
        if omega is not None:
            if sens is not None:
                raise ValueError("reset: the off-resonance stage is single-coil (omega with sens is not supported)")
            self._offres_for(times, segments, interpolator, omega_max, omega)
            return self.reset_offres(x0, y0, omega, w, cg_iters=cg_iters)
        if times is not None or segments is not None or w is not None or interpolator != "linear" or omega_max is not None:
            raise ValueError("reset: times, segments, w, interpolator and omega_max go with omega")
        nhw = self.n * self.h * self.w
        x0 = self._chk(x0, torch.complex64, nhw, "x0")
        if sens is not None:
            sens, coils, sens_n = self._sens(sens)
            y0 = self._chk(y0, torch.complex64, nhw * coils, "y0")
            m, mask_n = self._mask(mask)
            x, z, u = self._iterate()
            _lib.check(self.lib.pnp_reset_mc(self._h, x0.data_ptr(), y0.data_ptr(), sens.data_ptr(), coils, sens_n, m.data_ptr(), mask_n,
                                             int(cg_iters), x.data_ptr(), z.data_ptr(), u.data_ptr(), self._stream()), "pnp_reset_mc")
        else:
            y0 = self._chk(y0, torch.complex64, nhw, "y0")
            m, mask_n = self._mask(mask)
            x, z, u = self._iterate()
            _lib.check(self.lib.pnp_reset(self._h, x0.data_ptr(), y0.data_ptr(), m.data_ptr(), mask_n, x.data_ptr(),
                                          z.data_ptr(), u.data_ptr(), self._stream()), "pnp_reset")
        self.live_episode = _next_episode()
        return x, z, u

    def set_kspace(self, y0: torch.Tensor, mask: Optional[torch.Tensor] = None, episode: int = 0, sens: Optional[torch.Tensor] = None,
                   cg_iters: int = 8, omega: Optional[torch.Tensor] = None, times=None, segments: Optional[int] = None,
                   w: Optional[torch.Tensor] = None, interpolator: str = "linear", omega_max: Optional[float] = None) -> None:
        """Re-install the k-space constants (y0, mask) of another episode without touching any iterate
        (pnp_set_kspace); `episode` = the id that episode's reset returned (0: a fresh id).  With sens: a multi-coil episode's
        constants (pnp_set_kspace_mc), as in `reset`.  With omega: an off-resonance episode's (`set_kspace_offres`), as in `reset`."""
        if omega is not None:
            if sens is not None:
                raise ValueError("set_kspace: the off-resonance stage is single-coil (omega with sens is not supported)")
            self._offres_for(times, segments, interpolator, omega_max, omega)
            return self.set_kspace_offres(y0, omega, w, episode=episode, cg_iters=cg_iters)
        if times is not None or segments is not None or w is not None or interpolator != "linear" or omega_max is not None:
            raise ValueError("set_kspace: times, segments, w, interpolator and omega_max go with omega")
        nhw = self.n * self.h * self.w
        m, mask_n = self._mask(mask)
        if sens is not None:
            sens, coils, sens_n = self._sens(sens)
            y0 = self._chk(y0, torch.complex64, nhw * coils, "y0")
            _lib.check(self.lib.pnp_set_kspace_mc(self._h, y0.data_ptr(), sens.data_ptr(), coils, sens_n, m.data_ptr(), mask_n,
                                                  int(cg_iters), self._stream()), "pnp_set_kspace_mc")
        else:
            y0 = self._chk(y0, torch.complex64, nhw, "y0")
            _lib.check(self.lib.pnp_set_kspace(self._h, y0.data_ptr(), m.data_ptr(), mask_n, self._stream()), "pnp_set_kspace")
        self.live_episode = episode or _next_episode()

    def step(self, x: torch.Tensor, z: torch.Tensor, u: torch.Tensor, mu: torch.Tensor, sigma_d: torch.Tensor,
             t_action: Optional[torch.Tensor] = None, t_state: Optional[torch.Tensor] = None,
             done: Optional[torch.Tensor] = None) -> None:
        """One ADMM iteration in place on (x, z, u).  mu, sigma_d, t_action, t_state: float32 [N]; done: uint8 [N]."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(z, torch.complex64, nhw, "z"); self._chk(u, torch.complex64, nhw, "u")
        self._chk(mu, torch.float32, self.n, "mu"); self._chk(sigma_d, torch.float32, self.n, "sigma_d")
        if t_action is not None: self._chk(t_action, torch.float32, self.n, "t_action")
        if t_state is not None: self._chk(t_state, torch.float32, self.n, "t_state")
        if done is not None: self._chk(done, torch.uint8, self.n, "done")
        _lib.check(self.lib.pnp_step(self._h, mu.data_ptr(), sigma_d.data_ptr(), _ptr(t_action), x.data_ptr(),
                                     z.data_ptr(), u.data_ptr(), _ptr(t_state), _ptr(done), self._stream()), "pnp_step")

    def denoise(self, x: torch.Tensor, sigma: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(sigma, torch.float32, self.n, "sigma")
        if out is None:
            out = torch.empty_like(x)
        self._chk(out, torch.float32, nhw, "out")
        _lib.check(self.lib.pnp_denoise(self._h, x.data_ptr(), sigma.data_ptr(), out.data_ptr(), self._stream()), "pnp_denoise")
        return out

    def tv_denoise(self, x: torch.Tensor, lam: torch.Tensor, iters: int = 20, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Isotropic total-variation denoiser (pnp_tv_denoise): `iters` steps of Chambolle's dual projection, then clamp(x - lam div p, 0, 1).
        x float32 [N,1,H,W], lam float32 [N] (0 gives the clamp alone); out may be x.  Any engine kind, any size the engine takes."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(lam, torch.float32, self.n, "lam")
        iters = int(iters)
        if not 1 <= iters <= _lib.PNP_TV_MAX_ITERS:
            raise ValueError(f"iters must be 1..{_lib.PNP_TV_MAX_ITERS}, got {iters}")
        if out is None:
            out = torch.empty_like(x)
        self._chk(out, torch.float32, nhw, "out")
        _lib.check(self.lib.pnp_tv_denoise(self._h, x.data_ptr(), lam.data_ptr(), iters, out.data_ptr(), self._stream()), "pnp_tv_denoise")
        return out

    def set_prior(self, prior: str, tv_scale: float = 1.0, tv_iters: int = 20) -> None:
        """The x-update of `step` (pnp_set_prior): "unet" (the default) or "tv" - total variation with weight tv_scale * sigma_d and
        tv_iters dual steps, which needs no weights and also runs on an engine built with denoiser=False."""
        if prior not in _lib.PRIORS:
            raise ValueError(f"prior must be one of {tuple(_lib.PRIORS)}, got {prior!r}")
        _lib.check(self.lib.pnp_set_prior(self._h, _lib.PRIORS[prior], float(tv_scale), int(tv_iters)), "pnp_set_prior")

    def haar_denoise(self, x: torch.Tensor, lam: torch.Tensor, levels: int = 3, mode: str = "ti", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Haar wavelet shrinkage (pnp_haar_denoise): `levels` levels, threshold lam, periodic boundaries, clamped to [0, 1]; mode "ti" is the
        translation-invariant (fully cycle-spun) form, "ortho" the decimated orthonormal transform.  x float32 [N,1,H,W], lam float32 [N]
        (0 gives the clamp alone); out may be x.  Any engine kind, any size the engine takes."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(lam, torch.float32, self.n, "lam")
        levels = int(levels)
        if not 1 <= levels <= _lib.PNP_HAAR_MAX_LEVELS:
            raise ValueError(f"levels must be 1..{_lib.PNP_HAAR_MAX_LEVELS}, got {levels}")
        if mode not in _lib.HAAR_MODES:
            raise ValueError(f"mode must be one of {tuple(_lib.HAAR_MODES)}, got {mode!r}")
        if out is None:
            out = torch.empty_like(x)
        self._chk(out, torch.float32, nhw, "out")
        _lib.check(self.lib.pnp_haar_denoise(self._h, x.data_ptr(), lam.data_ptr(), levels, _lib.HAAR_MODES[mode], out.data_ptr(), self._stream()),
                   "pnp_haar_denoise")
        return out

    def set_haar_prior(self, scale: float = 1.0, levels: int = 3, mode: str = "ti") -> None:
        """Makes Haar shrinkage the x-update of `step` (pnp_set_prior_haar): threshold scale * sigma_d; like "tv" it needs no weights and
        also runs on an engine built with denoiser=False.  `set_prior("unet" | "tv")` switches away from it."""
        if mode not in _lib.HAAR_MODES:
            raise ValueError(f"mode must be one of {tuple(_lib.HAAR_MODES)}, got {mode!r}")
        _lib.check(self.lib.pnp_set_prior_haar(self._h, float(scale), int(levels), _lib.HAAR_MODES[mode]), "pnp_set_prior_haar")

    def haar_settings(self) -> Tuple[float, int, str]:
        """(haar_scale, levels, mode) as the handle holds them (pnp_get_prior_haar), whatever the current prior."""
        sc, lv, md = C.c_double(), C.c_int(), C.c_int()
        _lib.check(self.lib.pnp_get_prior_haar(self._h, C.byref(sc), C.byref(lv), C.byref(md)), "pnp_get_prior_haar")
        return float(sc.value), int(lv.value), {v: k for k, v in _lib.HAAR_MODES.items()}[md.value]

    @property
    def prior(self) -> str:
        """"unet", "tv" or "haar" (pnp_get_prior)."""
        return self.prior_settings()[0]

    def prior_settings(self) -> Tuple[str, float, int]:
        """(prior, tv_scale, tv_iters) as the handle holds them; under "haar" the pair is the stored TV pair (`haar_settings` has Haar's)."""
        pr, sc, it = C.c_int(), C.c_double(), C.c_int()
        _lib.check(self.lib.pnp_get_prior(self._h, C.byref(pr), C.byref(sc), C.byref(it)), "pnp_get_prior")
        return _lib.PRIOR_NAMES[pr.value], float(sc.value), int(it.value)

    def fft2c(self, img: torch.Tensor, inverse: bool = False) -> torch.Tensor:
        if img.dtype != torch.complex64 or img.shape[-2:] != (self.h, self.w):
            raise ValueError(f"fft2c: expected complex64 [...,{self.h},{self.w}], got {img.dtype} {tuple(img.shape)}")
        batch = img.numel() // (self.h * self.w)
        img = self._chk(img, torch.complex64, batch * self.h * self.w, "img")
        out = torch.empty_like(img)
        _lib.check(self.lib.pnp_fft2c(self._h, img.data_ptr(), out.data_ptr(), batch, self.h, self.w, int(inverse),
                                      self._stream()), "pnp_fft2c")
        return out

    def prox_dual(self, x, z, u, mu, t_action=None) -> None:
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(z, torch.complex64, nhw, "z"); self._chk(u, torch.complex64, nhw, "u")
        self._chk(mu, torch.float32, self.n, "mu")
        _lib.check(self.lib.pnp_prox_dual(self._h, mu.data_ptr(), _ptr(t_action), x.data_ptr(), z.data_ptr(),
                                          u.data_ptr(), self._stream()), "pnp_prox_dual")

    def psnr(self, x: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(gt, torch.float32, nhw, "gt")
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnp_psnr(self._h, x.data_ptr(), gt.data_ptr(), out.data_ptr(), self._stream()), "pnp_psnr")
        return out

    def ssim(self, x: torch.Tensor, gt: torch.Tensor, data_range: float = 1.0, k1: float = 0.01, k2: float = 0.03,
             radius: int = 8, clamp: bool = True, return_map: bool = False):
        """Per-slice SSIM (pnp_ssim): Gaussian window sigma 1.5 with `radius` taps each side (8 = the reference's win_size 11),
        'reflect' border, mean over all H x W pixels.  clamp: x clamped to [0, 1] first, like `psnr`.  Returns [N] on the device,
        and with return_map also the SSIM map [N,1,H,W]."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(gt, torch.float32, nhw, "gt")
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        smap = torch.empty((self.n, 1, self.h, self.w), dtype=torch.float32, device=self.device) if return_map else None
        _lib.check(self.lib.pnp_ssim(self._h, x.data_ptr(), gt.data_ptr(), float(data_range), float(k1), float(k2), int(radius),
                                     _lib.PNP_SSIM_CLAMP_X if clamp else 0, out.data_ptr(), _ptr(smap), self._stream()), "pnp_ssim")
        return (out, smap) if return_map else out

    def residuals(self, x: torch.Tensor, z: torch.Tensor, u: torch.Tensor, prev: Optional[torch.Tensor] = None, dc: bool = False,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ADMM residuals of the iterate (pnp_residuals): float32 [N, 6] on the device, columns `RESIDUAL_COLUMNS` = primal ||x - z||,
        dx, dz, du (change against `prev`, a buffer `snapshot` returned), delta = (dx + dz + du) / sqrt(H W), dc = the k-space data
        misfit ||where(mask, fft_c(x) - y0, 0)|| of the live episode.  Without `prev` columns 1-4 are 0, without `dc` column 5 is."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(z, torch.complex64, nhw, "z"); self._chk(u, torch.complex64, nhw, "u")
        flags = (_lib.PNP_RES_DC if dc else 0)
        if prev is not None:
            if prev.device != self.device or not prev.is_contiguous() or \
                    prev.numel() * prev.element_size() != self.lib.pnp_snapshot_bytes(self._h):
                raise ValueError("prev: not a snapshot of this engine")
            flags |= _lib.PNP_RES_DELTA
        if out is None:
            out = torch.empty((self.n, _lib.PNP_RES_COLS), dtype=torch.float32, device=self.device)
        self._chk(out, torch.float32, self.n * _lib.PNP_RES_COLS, "out")
        _lib.check(self.lib.pnp_residuals(self._h, x.data_ptr(), z.data_ptr(), u.data_ptr(), _ptr(prev), flags, out.data_ptr(),
                                          self._stream()), "pnp_residuals")
        return out

    def acquire(self, gt: torch.Tensor, mask: torch.Tensor, sigma_n: float, seed: int,
                sens: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """With sens (complex64 [C,H,W] or [N,C,H,W]): the multi-coil acquisition (pnp_acquire_mc), y0 complex64 [N,C,H,W] with
        y_c = mask * (fft_c(S_c gt) + sigma_n * noise_c), ATy0 = sum_c conj(S_c) ifft_c(y_c).  Without:

        Simulated CS-MRI acquisition of the engine's N slices on the device (pnp_acquire): gt float32 [N,1,H,W] in [0, 1], mask
        bool/uint8 [H,W] (or [N,H,W]) in the centred layout.  Returns complex64 [N,1,H,W] tensors (y0, ATy0, x0) with
        y0 = mask * (fft_c(gt) + sigma_n * noise), ATy0 = ifft_c(y0), x0 = max(ATy0, 0) on both planes; slice n draws the noise
        `synthetic.make_problem` draws for seed + n."""
        nhw = self.n * self.h * self.w
        gt = self._chk(gt, torch.float32, nhw, "gt")
        m, mask_n = self._mask(mask)
        seed = int(seed)
        if not 0 <= seed < 2 ** 64 - self.n:
            raise ValueError(f"seed: expected 0 <= seed < 2**64 - n, got {seed}")
        if sens is not None:
            sens, coils, sens_n = self._sens(sens)
            y0 = torch.empty((self.n, coils, self.h, self.w), dtype=torch.complex64, device=self.device)
            aty0 = torch.empty((self.n, 1, self.h, self.w), dtype=torch.complex64, device=self.device)
            x0 = torch.empty_like(aty0)
            _lib.check(self.lib.pnp_acquire_mc(self._h, gt.data_ptr(), sens.data_ptr(), coils, sens_n, m.data_ptr(), mask_n, float(sigma_n),
                                               seed, 0, y0.data_ptr(), aty0.data_ptr(), x0.data_ptr(), self._stream()), "pnp_acquire_mc")
            return y0, aty0, x0
        y0 = torch.empty((self.n, 1, self.h, self.w), dtype=torch.complex64, device=self.device)
        aty0, x0 = torch.empty_like(y0), torch.empty_like(y0)
        _lib.check(self.lib.pnp_acquire(self._h, gt.data_ptr(), m.data_ptr(), mask_n, float(sigma_n), seed, 0, y0.data_ptr(), aty0.data_ptr(),
                                        x0.data_ptr(), self._stream()), "pnp_acquire")
        return y0, aty0, x0

    def estimate_sens(self, y0: torch.Tensor, acs: Tuple[int, int], window: str = "hann", thresh: float = 0.0, return_rss: bool = False):
        """Coil sensitivity maps from the fully sampled calibration block of multi-coil k-space (pnp_estimate_sens): y0 complex64
        [N,C,H,W] in the centred layout, acs = (acs_h, acs_w) the even sides of the centred block, window "hann" or "box".  Each
        coil's windowed block is transformed back and divided by the root-sum-of-squares over the coils; pixels whose rss is not
        above thresh * (the slice's largest rss) get zero maps.  Returns complex64 [N,C,H,W] per-slice maps for `reset(..., sens=)`,
        and with return_rss also rss float32 [N,H,W].  Does not change the engine's mode or its installed constants."""
        if y0.dim() != 4 or y0.shape[0] != self.n or tuple(y0.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"y0: expected [{self.n},C,{self.h},{self.w}], got {tuple(y0.shape)}")
        coils = int(y0.shape[1])
        y0 = self._chk(y0, torch.complex64, self.n * coils * self.h * self.w, "y0")
        if window not in _lib.SENS_WINDOWS:
            raise ValueError(f"window must be one of {tuple(_lib.SENS_WINDOWS)}, got {window!r}")
        acs_h, acs_w = (int(v) for v in acs)
        sens = torch.empty_like(y0)
        rss = torch.empty((self.n, self.h, self.w), dtype=torch.float32, device=self.device) if return_rss else None
        _lib.check(self.lib.pnp_estimate_sens(self._h, y0.data_ptr(), coils, acs_h, acs_w, _lib.SENS_WINDOWS[window], float(thresh), 0,
                                              sens.data_ptr(), _ptr(rss), self._stream()), "pnp_estimate_sens")
        return (sens, rss) if return_rss else sens

    def espirit_sens(self, y0: torch.Tensor, acs: Tuple[int, int], ksize: int = 6, sv_thresh: float = 0.02, crop: float = 0.9, iters: int = 16,
                     window: str = "hann", thresh: float = 0.0, return_eval: bool = False, return_kernels: bool = False):
        """ESPIRiT coil sensitivity maps from the fully sampled calibration block of multi-coil k-space (pnp_espirit_sens): y0 complex64
        [N,C,H,W] in the centred layout, C <= 16 (compress more channels first), acs = (acs_h, acs_w) the even sides of the centred block,
        ksize the side of the calibration kernels (C ksize^2 <= 512; a block with fewer (acs_h - ksize + 1)(acs_w - ksize + 1) windows than
        C ksize^2 calibrates badly).  The signal space of the calibration matrix keeps the singular values above sv_thresh times the
        largest; per pixel the dominant eigenvector comes from `iters` power steps started at the low-resolution estimate of
        `estimate_sens` (same window), its phase is set so that the image stays real, and pixels whose eigenvalue is not above crop - or
        whose low-resolution rss is not above thresh * (the slice's largest) - get zero maps.  Returns complex64 [N,C,H,W] per-slice maps
        for `reset(..., sens=)`; with return_eval also the eigenvalue map float32 [N,H,W]; with return_kernels also (kern complex64
        [N,C,C,2 ksize - 1,2 ksize - 1], nkept int32 [N]).  Does not change the engine's mode or its installed constants."""
        if y0.dim() != 4 or y0.shape[0] != self.n or tuple(y0.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"y0: expected [{self.n},C,{self.h},{self.w}], got {tuple(y0.shape)}")
        coils = int(y0.shape[1])
        y0 = self._chk(y0, torch.complex64, self.n * coils * self.h * self.w, "y0")
        if window not in _lib.SENS_WINDOWS:
            raise ValueError(f"window must be one of {tuple(_lib.SENS_WINDOWS)}, got {window!r}")
        if not 1 <= coils <= _lib.PNP_ESPIRIT_MAX_COILS:
            raise ValueError(f"espirit_sens takes 1..{_lib.PNP_ESPIRIT_MAX_COILS} coils, got {coils}: compress the channels first")
        ksize, iters = int(ksize), int(iters)
        if not 2 <= ksize <= _lib.PNP_ESPIRIT_MAX_KSIZE or coils * ksize * ksize > _lib.PNP_ESPIRIT_MAX_N:
            raise ValueError(f"ksize must be 2..{_lib.PNP_ESPIRIT_MAX_KSIZE} with coils * ksize^2 <= {_lib.PNP_ESPIRIT_MAX_N}, got {ksize} at "
                             f"{coils} coils")
        acs_h, acs_w = (int(v) for v in acs)
        sens = torch.empty_like(y0)
        ev = torch.empty((self.n, self.h, self.w), dtype=torch.float32, device=self.device) if return_eval else None
        d = 2 * ksize - 1
        kern = torch.empty((self.n, coils, coils, d, d), dtype=torch.complex64, device=self.device) if return_kernels else None
        nkept = torch.empty((self.n,), dtype=torch.int32, device=self.device) if return_kernels else None
        _lib.check(self.lib.pnp_espirit_sens(self._h, y0.data_ptr(), coils, acs_h, acs_w, ksize, float(sv_thresh), float(crop), iters,
                                             _lib.SENS_WINDOWS[window], float(thresh), 0, sens.data_ptr(), _ptr(ev), _ptr(kern), _ptr(nkept),
                                             self._stream()), "pnp_espirit_sens")
        out = (sens,) + ((ev,) if return_eval else ()) + ((kern, nkept) if return_kernels else ())
        return out if len(out) > 1 else sens

    def coil_compress_matrix(self, y0: torch.Tensor, acs: Tuple[int, int], return_gram: bool = False):
        """Coil compression matrices from the calibration block of multi-coil k-space (pnp_coil_compress_matrix): y0 complex64
        [N,C,H,W] in the centred layout, C <= 64, acs = (acs_h, acs_w) the even sides of the centred block.  Per slice the C x C channel
        covariance of the block is diagonalised on the device; row v of cmat is virtual coil v, in order of descending eigenvalue.
        Returns (cmat complex64 [N,C,C], eig float32 [N,C]) and with return_gram also the covariance, complex128 [N,C,C].  Does not
        change the engine's mode or its installed constants."""
        if y0.dim() != 4 or y0.shape[0] != self.n or tuple(y0.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"y0: expected [{self.n},C,{self.h},{self.w}], got {tuple(y0.shape)}")
        coils = int(y0.shape[1])
        y0 = self._chk(y0, torch.complex64, self.n * coils * self.h * self.w, "y0")
        acs_h, acs_w = (int(v) for v in acs)
        cmat = torch.empty((self.n, coils, coils), dtype=torch.complex64, device=self.device)
        eig = torch.empty((self.n, coils), dtype=torch.float32, device=self.device)
        gram = torch.empty((self.n, coils, coils), dtype=torch.complex128, device=self.device) if return_gram else None
        _lib.check(self.lib.pnp_coil_compress_matrix(self._h, y0.data_ptr(), coils, acs_h, acs_w, 0, cmat.data_ptr(), eig.data_ptr(),
                                                     _ptr(gram), self._stream()), "pnp_coil_compress_matrix")
        return (cmat, eig, gram) if return_gram else (cmat, eig)

    def coil_compress_apply(self, planes: torch.Tensor, cmat: torch.Tensor, out_coils: int) -> torch.Tensor:
        """The leading `out_coils` virtual coils of `planes` (pnp_coil_compress_apply): planes complex64 [N,C,H,W] - k-space or coil
        maps, the mix is pointwise -, cmat complex64 [C,C] (one matrix for all slices) or [N,C,C].  Returns complex64 [N,out_coils,H,W],
        out[n,v] = sum_c cmat[n,v,c] planes[n,c]."""
        if planes.dim() != 4 or planes.shape[0] != self.n or tuple(planes.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"planes: expected [{self.n},C,{self.h},{self.w}], got {tuple(planes.shape)}")
        coils = int(planes.shape[1])
        planes = self._chk(planes, torch.complex64, self.n * coils * self.h * self.w, "planes")
        if tuple(cmat.shape) not in ((coils, coils), (1, coils, coils), (self.n, coils, coils)):
            raise ValueError(f"cmat: expected [{coils},{coils}] or [{self.n},{coils},{coils}], got {tuple(cmat.shape)}")
        cmat_n = 1 if cmat.numel() == coils * coils else self.n
        cmat = self._chk(cmat, torch.complex64, cmat_n * coils * coils, "cmat")
        out_coils = int(out_coils)
        if not 1 <= out_coils <= min(coils, _lib.PNP_MC_MAX_COILS):
            raise ValueError(f"out_coils must be 1..{min(coils, _lib.PNP_MC_MAX_COILS)}, got {out_coils}")
        out = torch.empty((self.n, out_coils, self.h, self.w), dtype=torch.complex64, device=self.device)
        _lib.check(self.lib.pnp_coil_compress_apply(self._h, planes.data_ptr(), coils, cmat.data_ptr(), cmat_n, out_coils, out.data_ptr(),
                                                    self._stream()), "pnp_coil_compress_apply")
        return out

    def noise_cov(self, noise: torch.Tensor) -> torch.Tensor:
        """Channel noise covariance of noise-only scans (pnp_noise_cov): noise complex64 [C,S] or [M,C,S], C <= 64, any M (not tied to the
        engine's N).  Returns Psi complex128 [M,C,C] ([C,C] for a 2-d input), Psi[a][b] = mean_s n_a[s] conj(n_b[s]), summed in float64 in
        a fixed order, exactly Hermitian.  Does not change the engine's mode or its installed constants."""
        if noise.dim() not in (2, 3):
            raise ValueError(f"noise: expected [C,S] or [M,C,S], got {tuple(noise.shape)}")
        m = 1 if noise.dim() == 2 else int(noise.shape[0])
        coils, samples = int(noise.shape[-2]), int(noise.shape[-1])
        noise = self._chk(noise, torch.complex64, m * coils * samples, "noise")
        psi = torch.empty((m, coils, coils), dtype=torch.complex128, device=self.device)
        _lib.check(self.lib.pnp_noise_cov(self._h, noise.data_ptr(), m, coils, samples, 0, psi.data_ptr(), self._stream()), "pnp_noise_cov")
        return psi[0] if noise.dim() == 2 else psi

    def whiten_matrix(self, psi: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Whitening matrices of Hermitian positive-definite covariances (pnp_whiten_matrix): psi complex128 [C,C] or [M,C,C].  Returns
        (wmat, lmat, info): Psi = L L^H, W = L^-1, both complex64 lower-triangular in psi's shape, and info int32 [M] - 0, or j + 1 when
        column j's pivot fails (that matrix's wmat and lmat are then the identity).  Nothing is read back: check info where it matters."""
        if psi.dim() not in (2, 3) or psi.shape[-1] != psi.shape[-2]:
            raise ValueError(f"psi: expected [C,C] or [M,C,C], got {tuple(psi.shape)}")
        m = 1 if psi.dim() == 2 else int(psi.shape[0])
        coils = int(psi.shape[-1])
        psi = self._chk(psi, torch.complex128, m * coils * coils, "psi")
        wmat = torch.empty(tuple(psi.shape), dtype=torch.complex64, device=self.device)
        lmat = torch.empty_like(wmat)
        info = torch.empty((m,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pnp_whiten_matrix(self._h, psi.data_ptr(), m, coils, 0, wmat.data_ptr(), lmat.data_ptr(), info.data_ptr(),
                                              self._stream()), "pnp_whiten_matrix")
        return wmat, lmat, info

    def whiten_apply(self, planes: torch.Tensor, wmat: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The lower-triangular channel mix out[n,v] = sum_{c <= v} wmat[n,v,c] planes[n,c] (pnp_whiten_apply): planes complex64 [N,C,H,W]
        - k-space or coil maps -, wmat complex64 [C,C] (one matrix for all slices) or [N,C,C], only its lower triangle is read.
        out=planes runs in place (no second buffer); out=None allocates the result."""
        if planes.dim() != 4 or planes.shape[0] != self.n or tuple(planes.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"planes: expected [{self.n},C,{self.h},{self.w}], got {tuple(planes.shape)}")
        coils = int(planes.shape[1])
        planes = self._chk(planes, torch.complex64, self.n * coils * self.h * self.w, "planes")
        if tuple(wmat.shape) not in ((coils, coils), (1, coils, coils), (self.n, coils, coils)):
            raise ValueError(f"wmat: expected [{coils},{coils}] or [{self.n},{coils},{coils}], got {tuple(wmat.shape)}")
        wmat_n = 1 if wmat.numel() == coils * coils else self.n
        wmat = self._chk(wmat, torch.complex64, wmat_n * coils * coils, "wmat")
        if out is None:
            out = torch.empty_like(planes)
        elif tuple(out.shape) != tuple(planes.shape):
            raise ValueError(f"out: expected {tuple(planes.shape)}, got {tuple(out.shape)}")
        out = self._chk(out, torch.complex64, planes.numel(), "out")
        _lib.check(self.lib.pnp_whiten_apply(self._h, planes.data_ptr(), coils, wmat.data_ptr(), wmat_n, out.data_ptr(), self._stream()),
                   "pnp_whiten_apply")
        return out

    @staticmethod
    def _grappa_kernel(coils: int, accel: int, kernel) -> Tuple[int, int, int, int]:
        """(by, bx, ns, nt) of a GRAPPA kernel, or ValueError for what pnp_grappa_* would refuse"""
        by, bx = (int(v) for v in kernel)
        if not 1 <= coils <= _lib.PNP_GRAPPA_MAX_COILS:
            raise ValueError(f"grappa takes 1..{_lib.PNP_GRAPPA_MAX_COILS} coils, got {coils}: compress the channels first")
        if not 2 <= accel <= _lib.PNP_GRAPPA_MAX_ACCEL:
            raise ValueError(f"accel must be 2..{_lib.PNP_GRAPPA_MAX_ACCEL}, got {accel}")
        if by not in (1, 3, 5, 7) or bx not in (2, 4) or coils * by * bx > _lib.PNP_GRAPPA_MAX_SRC:
            raise ValueError(f"kernel must be (1|3|5|7, 2|4) with coils * by * bx <= {_lib.PNP_GRAPPA_MAX_SRC}, got {(by, bx)} at {coils} coils")
        return by, bx, coils * by * bx, coils * (accel - 1)

    def grappa_weights(self, y0: torch.Tensor, acs: Tuple[int, int], accel: int, kernel: Tuple[int, int] = (5, 4), lam: float = 1e-2,
                       return_gram: bool = False):
        """GRAPPA interpolation weights from the fully sampled calibration block of multi-coil k-space (pnp_grappa_weights): y0 complex64
        [N,C,H,W] in the centred layout, C <= 32, acs = (acs_h, acs_w) the even sides of the centred block, accel = R the spacing of the
        comb of acquired columns (it divides W), kernel = (by, bx): by rows (1, 3, 5 or 7) by bx acquired columns (2 or 4).  Per slice the
        normal equations of all windows of the block, regularised by lam * trace / ns, are solved in float64 on the device.  Returns
        (wts complex64 [N,nt,ns], info int32 [N]) with ns = C by bx sources and nt = C (R - 1) targets - info is 0, or j + 1 when pivot j
        fails (that slice's weights are then zero; nothing is read back: check info where it matters) - and with return_gram also the
        normal matrix A^H [A | T], complex128 [N,ns,ns+nt].  lam = 1e-2 is a default from a scan on the analytic coils, not a tuned value.
        Does not change the engine's mode or its installed constants."""
        if y0.dim() != 4 or y0.shape[0] != self.n or tuple(y0.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"y0: expected [{self.n},C,{self.h},{self.w}], got {tuple(y0.shape)}")
        coils, accel = int(y0.shape[1]), int(accel)
        y0 = self._chk(y0, torch.complex64, self.n * coils * self.h * self.w, "y0")
        by, bx, ns, nt = self._grappa_kernel(coils, accel, kernel)
        acs_h, acs_w = (int(v) for v in acs)
        wts = torch.empty((self.n, nt, ns), dtype=torch.complex64, device=self.device)
        info = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        gram = torch.empty((self.n, ns, ns + nt), dtype=torch.complex128, device=self.device) if return_gram else None
        _lib.check(self.lib.pnp_grappa_weights(self._h, y0.data_ptr(), coils, acs_h, acs_w, accel, by, bx, float(lam), 0, wts.data_ptr(),
                                               info.data_ptr(), _ptr(gram), self._stream()), "pnp_grappa_weights")
        return (wts, info, gram) if return_gram else (wts, info)

    def grappa_apply(self, y0: torch.Tensor, wts: torch.Tensor, mask: torch.Tensor, accel: int, offset: int, kernel: Tuple[int, int] = (5, 4),
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K-space with its missing columns synthesised from their acquired neighbours (pnp_grappa_apply): y0 complex64 [N,C,H,W], wts
        complex64 [nt,ns] (one set for all slices) or [N,nt,ns] from `grappa_weights`, mask bool/uint8 [H,W] or [N,H,W] in the centred
        layout, the acquired comb x = offset (mod accel).  Bins of the mask and of the comb are copies of y0; every other bin is the
        weighted sum of its by x bx x C neighbours on the comb, indices periodic.  out must not overlap y0; None allocates it."""
        if y0.dim() != 4 or y0.shape[0] != self.n or tuple(y0.shape[-2:]) != (self.h, self.w):
            raise ValueError(f"y0: expected [{self.n},C,{self.h},{self.w}], got {tuple(y0.shape)}")
        coils, accel, offset = int(y0.shape[1]), int(accel), int(offset)
        y0 = self._chk(y0, torch.complex64, self.n * coils * self.h * self.w, "y0")
        by, bx, ns, nt = self._grappa_kernel(coils, accel, kernel)
        if tuple(wts.shape) not in ((nt, ns), (1, nt, ns), (self.n, nt, ns)):
            raise ValueError(f"wts: expected [{nt},{ns}] or [{self.n},{nt},{ns}], got {tuple(wts.shape)}")
        wts_n = 1 if wts.numel() == nt * ns else self.n
        wts = self._chk(wts, torch.complex64, wts_n * nt * ns, "wts")
        m, mask_n = self._mask(mask)
        if out is None:
            out = torch.empty_like(y0)
        elif tuple(out.shape) != tuple(y0.shape):
            raise ValueError(f"out: expected {tuple(y0.shape)}, got {tuple(out.shape)}")
        out = self._chk(out, torch.complex64, y0.numel(), "out")
        _lib.check(self.lib.pnp_grappa_apply(self._h, y0.data_ptr(), coils, m.data_ptr(), mask_n, accel, offset, by, bx, wts.data_ptr(), wts_n,
                                             out.data_ptr(), self._stream()), "pnp_grappa_apply")
        return out

    def snapshot(self, x: torch.Tensor, z: torch.Tensor, u: torch.Tensor, t_state: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One packed device buffer [x | z | u | T] (pnp_snapshot): a tree-search node's copy of the iterate."""
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(z, torch.complex64, nhw, "z"); self._chk(u, torch.complex64, nhw, "u")
        if t_state is not None:
            self._chk(t_state, torch.float32, self.n, "t_state")
        nbytes = self.lib.pnp_snapshot_bytes(self._h)
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        elif out.numel() * out.element_size() != nbytes or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"snapshot buffer must be {nbytes} contiguous bytes on {self.device}")
        _lib.check(self.lib.pnp_snapshot(self._h, x.data_ptr(), z.data_ptr(), u.data_ptr(), _ptr(t_state), out.data_ptr(),
                                         self._stream()), "pnp_snapshot")
        return out

    def restore(self, snap: torch.Tensor, x: torch.Tensor, z: torch.Tensor, u: torch.Tensor,
                t_state: Optional[torch.Tensor] = None) -> None:
        nhw = self.n * self.h * self.w
        self._chk(x, torch.float32, nhw, "x"); self._chk(z, torch.complex64, nhw, "z"); self._chk(u, torch.complex64, nhw, "u")
        if t_state is not None:
            self._chk(t_state, torch.float32, self.n, "t_state")
        if snap.numel() * snap.element_size() != self.lib.pnp_snapshot_bytes(self._h) or not snap.is_contiguous():
            raise ValueError("not a snapshot of this engine")
        _lib.check(self.lib.pnp_restore(self._h, snap.data_ptr(), x.data_ptr(), z.data_ptr(), u.data_ptr(), _ptr(t_state),
                                        self._stream()), "pnp_restore")

    def read_stage(self, which: int) -> torch.Tensor:
        c, hh, ww = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.lib.pnp_unet_read_stage(self._h, which, None, C.byref(c), C.byref(hh), C.byref(ww), self._stream()),
                   "pnp_unet_read_stage")
        out = torch.empty((self.n, c.value, hh.value, ww.value), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pnp_unet_read_stage(self._h, which, out.data_ptr(), None, None, None, self._stream()),
                   "pnp_unet_read_stage")
        return out

    def conv_algorithms(self):
        """Per conv layer: 0 direct MFMA, 1 Winograd F(2x2), 4 Winograd F(4x4), 2 first layer (VALU), 3 last layer,
        5 bf16 producer/consumer kernel (bf16 mode, chip-filling problems)."""
        out = (C.c_int32 * _lib.N_LAYERS)()
        _lib.check(self.lib.pnp_conv_algorithms(self._h, out), "pnp_conv_algorithms")
        return list(out)

    def conv_schedules(self):
        """Per conv layer, the schedule of the F(4x4) arithmetic it runs: 0 not on F(4x4), 1 all waves in step, 2 the tile halves half
        a chunk apart, 3 16-tile M-blocks in independent workgroups, 4 cout-split (16 tiles x 128 channels per workgroup)."""
        out = (C.c_int32 * _lib.N_LAYERS)()
        _lib.check(self.lib.pnp_conv_schedules(self._h, out), "pnp_conv_schedules")
        return list(out)

    def bf16_weight_terms(self) -> int:
        """bf16 terms per conv weight: 0 on an f32 handle, 2 in bf16 mode (hi + lo), 1 with PNP_BF16_W1 (ablation)."""
        return int(self.lib.pnp_bf16_weight_terms(self._h))

    # -- kernel timing ---------------------------------------------------------------------
    def profile_reset(self) -> None:
        _lib.check(self.lib.pnp_profile_reset(self._h), "pnp_profile_reset")

    def profile_collect(self) -> Dict[str, Dict[str, float]]:
        """Call after synchronising the stream.  {class: {ms, launches}} plus per-layer lists."""
        ms = (C.c_double * _lib.PROFILE_CLASSES)()
        cnt = (C.c_int64 * _lib.PROFILE_CLASSES)()
        _lib.check(self.lib.pnp_profile_collect(self._h, ms, cnt), "pnp_profile_collect")
        lms = (C.c_double * _lib.N_LAYERS)()
        lcnt = (C.c_int64 * _lib.N_LAYERS)()
        _lib.check(self.lib.pnp_profile_layers(self._h, lms, lcnt), "pnp_profile_layers")
        out = {name: {"ms": ms[i], "launches": int(cnt[i])} for i, name in enumerate(_lib.PROFILE_CLASS_NAMES)}
        out["layers"] = {"ms": list(lms), "launches": [int(v) for v in lcnt]}
        return out
