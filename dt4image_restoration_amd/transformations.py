"""`fft` / `ifft`: drop-ins for the reference's centred orthonormal FFT pair
(/root/reference/evaluation/utils/transformations.py:6-19), running the LDS Stockham kernels of
libpnpadmm.so.  Sides of 16..1024 of the form 2^a * 5^b: the powers of two and 80, 160, 320, 400, 640, 800 (the
reference only ever passes 128 x 128).

`calculate_ssim`: drop-in for the reference's Gaussian-window SSIM (transformations.py:61-95, scipy on the host),
running pnp_ssim on the GPU.  Sides that are multiples of 16 (16..1024)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from .engine import PnPEngine

_engines: Dict[Tuple[int, int, int, int], PnPEngine] = {}


def _engine(batch: int, h: int, w: int, dev: int) -> PnPEngine:
    key = (batch, h, w, dev)
    e = _engines.get(key)
    if e is None:
        e = _engines[key] = PnPEngine(batch, h, w, device=dev, denoiser=False)
    return e


def _run(img: torch.Tensor, inverse: bool) -> torch.Tensor:
    if not img.is_cuda:
        raise RuntimeError("fft/ifft: the HIP path needs a GPU tensor; there is no CPU path")
    if not img.is_complex():
        img = img.to(torch.complex64)
    h, w = img.shape[-2:]
    c = img.to(torch.complex64).contiguous()
    batch = c.numel() // (h * w)
    return _engine(batch, h, w, c.device.index).fft2c(c, inverse=inverse).reshape(img.shape)


def fft(img: torch.Tensor) -> torch.Tensor:
    return _run(img, False)


def ifft(img: torch.Tensor) -> torch.Tensor:
    return _run(img, True)


def calculate_ssim(img1, img2, k1=0.01, k2=0.03, win_size=11, L=255):
    """SSIM of img1 against img2 exactly as the reference defines it: scipy's gaussian_filter(sigma=1.5,
    truncate=win_size//2) - radius int(1.5 * (win_size // 2) + 0.5), 'reflect' border - c1 = (k1 L)^2, c2 = (k2 L)^2,
    score = mean of the map, no clamp.  Returns (ssim_map, score) like the reference.

    img1, img2: [H, W] or batched [..., H, W], numpy arrays or GPU tensors (converted to float32).  A batch is scored per
    image: score has the batch shape ([] for one image).  numpy in -> numpy out (map float32, score float64); tensors in ->
    tensors on the device.  H, W must be multiples of 16; there is no CPU path."""
    as_numpy = not (isinstance(img1, torch.Tensor) or isinstance(img2, torch.Tensor))
    t1, t2 = torch.as_tensor(img1), torch.as_tensor(img2)
    if t1.shape != t2.shape or t1.dim() < 2:
        raise ValueError(f"calculate_ssim: img1 {tuple(t1.shape)} and img2 {tuple(t2.shape)} must be images of one shape")
    h, w = t1.shape[-2:]
    if h % 16 or w % 16 or h < 16 or w < 16:
        raise ValueError(f"calculate_ssim: the HIP kernel takes sides that are multiples of 16 (>= 16); got {h} x {w}")
    if t1.is_cuda:
        dev = t1.device
    elif t2.is_cuda:
        dev = t2.device
    elif as_numpy and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        raise RuntimeError("calculate_ssim: the HIP path needs a GPU (numpy input or GPU tensors); there is no CPU path")
    lead = tuple(t1.shape[:-2])
    batch = int(np.prod(lead)) if lead else 1
    x = t1.to(dev, torch.float32).reshape(batch, 1, h, w).contiguous()
    g = t2.to(dev, torch.float32).reshape(batch, 1, h, w).contiguous()
    radius = int(1.5 * (win_size // 2) + 0.5)                     # scipy: int(truncate * sigma + 0.5)
    score, smap = _engine(batch, h, w, dev.index).ssim(x, g, data_range=float(L), k1=float(k1), k2=float(k2), radius=radius,
                                                        clamp=False, return_map=True)
    smap, score = smap.reshape(t1.shape), score.reshape(lead)
    if as_numpy:
        return smap.cpu().numpy(), score.double().cpu().numpy()[()]
    return smap, score
