#!/usr/bin/env python3
"""Generate tests/golden/g9_ssim.npz by RUNNING THE REFERENCE'S OWN `calculate_ssim`
(evaluation/utils/transformations.py:61-95, scipy's gaussian_filter) on float64 inputs.

Run in the build container only (needs the reference checkout and scipy; neither exists on the GPU
box and nothing at test time imports them):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_ssim.py

Pairs: the synthetic ground truth against its zero-filled reconstruction x0 (real part, clipped at 0 like
datasets.py:160) and against a blurred copy of itself, at 128 x 128 (both pairs), 96 x 80, 256 x 256 and 16 x 16.
Inputs are stored as float16 - values every precision represents exactly, so the float32 kernel and the float64
reference see the same numbers - which keeps the file small.  Parameter sets (win_size, L): (11, 1), (11, 255), (7, 1).
Scores are float64; the maps (float32) are kept for the 128 x 128 and 16 x 16 pairs only.

Everything written is DATA (inputs + the reference's outputs); no reference source text is copied.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DT4IR_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from dt4image_restoration_amd import synthetic  # noqa: E402

PARAMS = ((11, 1.0), (11, 255.0), (7, 1.0))
# (name, h, w, kind, map kept)
PAIRS = (("p128_x0", 128, 128, "x0", True), ("p128_blur", 128, 128, "blur", True), ("p96x80_x0", 96, 80, "x0", False),
         ("p256_blur", 256, 256, "blur", False), ("p16_x0", 16, 16, "x0", True))


def blur(img):
    """3 x 3 box blur with edge replication (any smoothing will do: it only has to differ from the input)."""
    p = np.pad(img, 1, mode="edge")
    h, w = img.shape
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0


def main():
    sys.path.insert(0, REF)
    from evaluation.utils.transformations import calculate_ssim
    out = {"params": np.array(PARAMS, dtype=np.float64), "pairs": np.array([p[0] for p in PAIRS])}
    for i, (name, h, w, kind, keep_map) in enumerate(PAIRS):
        prob = synthetic.make_problem(1, h, w, accel=4.0, sigma_n=10.0 / 255.0, seed=900 + i)
        gt = prob["gt"].reshape(h, w).astype(np.float16)
        x = (prob["x0"][..., 0].reshape(h, w) if kind == "x0" else blur(gt.astype(np.float64))).astype(np.float16)
        out[f"{name}_x"], out[f"{name}_gt"] = x, gt
        for j, (win, L) in enumerate(PARAMS):
            smap, score = calculate_ssim(x.astype(np.float64), gt.astype(np.float64), win_size=win, L=L)
            out[f"{name}_score{j}"] = np.float64(score)
            if keep_map:
                out[f"{name}_map{j}"] = smap.astype(np.float32)
    path = os.path.join(HERE, "g9_ssim.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
