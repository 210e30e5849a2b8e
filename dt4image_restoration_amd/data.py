"""On-disk evaluation format of the reference: one `.mat` per image with keys
`x0, y0, ATy0` (float [..,H,W,2], real/imag last), `mask` [H,W], `gt` [1,H,W]
(/root/reference/dataset/datasets.py:135-207).  Filenames carry the task, e.g. `..._4_10...mat` -> "4x_10"
(acceleration x noise level; `extract_task` datasets.py:13-16).  scipy.io reads/writes it; no sample file ships with the
reference, so the writer here is what the tests round-trip."""
from __future__ import annotations

import os
import re
from typing import Dict, List, Sequence, Tuple

import numpy as np

OPTIMAL_TASKS = ["2x_5", "2x_10", "2x_15", "4x_5", "4x_10", "4x_15", "8x_5", "8x_10", "8x_15"]   # datasets.py:175
FLEX_TASKS = ["rtg_1.5", "rtg_3", "rtg_3.5", "rtg_4", "rtg_4.5", "rtg_5"]                          # datasets.py:136
OPTIMAL_RTG_RANGE = (-1.08, 16.6)       # datasets.py:178-179
FLEX_RTG_RANGE = (-1.8, 5.0)            # datasets.py:139-140
_MAT_KEYS = ("x0", "y0", "mask", "ATy0", "gt")


def task_from_filename(fn: str) -> str:
    """`\\d+_\\d+` in the file name -> '<accel>x_<sigma>' (datasets.py:13-16, :188-189)."""
    m = re.search(r"\d+_\d+", os.path.basename(fn))
    if m is None:
        raise ValueError(f"no '<accel>_<sigma>' task tag in file name {fn!r}")
    t = m.group()
    return t[0] + "x" + t[1:]           # exactly the reference's string surgery (single-digit acceleration)


def normalised_rtg(target: float, flex: bool = False) -> float:
    lo, hi = FLEX_RTG_RANGE if flex else OPTIMAL_RTG_RANGE
    return (float(target) - lo) / (hi - lo)


def save_mat(path: str, problem: Dict[str, np.ndarray], index: int = 0) -> None:
    """Write slice `index` of a `synthetic.make_problem` dict in the reference's `.mat` layout.  `x0` is stored as the
    raw zero-filled reconstruction (= ATy0, negative pixels included), as a TFPnP-style file holds it; the loader clips."""
    from scipy.io import savemat
    if "traj" in problem:                                    # a non-Cartesian acquisition: samples [1,M,2], the trajectory and weights, no mask
        nc = {"x0": problem["ATy0"][index], "y0": problem["y0"][index], "ATy0": problem["ATy0"][index], "gt": problem["gt"][index],
              "traj": problem["traj"]}
        if problem.get("dcf") is not None:
            nc["dcf"] = problem["dcf"]
        if problem.get("sens") is not None:                  # non-Cartesian SENSE: samples [C,M,2] and the maps [C,H,W] of this slice
            s = np.asarray(problem["sens"])
            nc["sens"] = s if s.ndim == 3 else s[index]
        savemat(path, nc)
        return
    savemat(path, {"x0": problem["ATy0"][index], "y0": problem["y0"][index], "ATy0": problem["ATy0"][index],
                   "mask": problem["mask"].astype(np.uint8), "gt": problem["gt"][index]})


def load_mat(path: str) -> Dict[str, np.ndarray]:
    """One image as the reference's datasets return it (datasets.py:153-160,191-199): `x0` clipped at 0 is what the
    environment gets (`action_dict['x0']`, :160,199), while the policy's first state token is the UNclipped real part
    of the stored x0 (:162,201 read `mat['x0'][..., 0]` after the clip only rebound the dict entry) - kept here as
    `x0_raw` [..,H,W] so a reference checkpoint sees the same first observation."""
    from scipy.io import loadmat
    mat = loadmat(path)
    missing = [k for k in _MAT_KEYS if k not in mat]
    if missing:
        raise KeyError(f"{path}: missing keys {missing}")
    out = {k: np.asarray(mat[k]) for k in _MAT_KEYS}
    out["x0_raw"] = np.array(out["x0"][..., 0], dtype=np.float32)
    out["x0"] = np.clip(out["x0"], a_min=0, a_max=None)
    return out


def list_dir(data_dir: str, limit: int = 0) -> List[str]:
    """The `.mat` files of a directory in the reference's order (sorted, datasets.py:146-147), first `limit` if given."""
    fns = sorted(f for f in os.listdir(data_dir) if f.endswith(".mat"))
    if limit:
        fns = fns[:limit]
    if not fns:
        raise FileNotFoundError(f"no .mat files in {data_dir}")
    return fns


def load_dir(data_dir: str, limit: int = 0, start: int = 0, stop: int = None) -> Tuple[Dict[str, np.ndarray], List[str]]:
    """The `.mat` files [start, stop) of a directory (of its first `limit` files, sorted) stacked into one batch dict
    {x0,y0,ATy0: [N,1,H,W,2], mask [H,W], gt [N,1,H,W], x0_raw [N,1,H,W]} + their task names.  A rank of a sharded run
    reads only its own files."""
    fns = list_dir(data_dir, limit)[start:stop]
    if not fns:
        raise FileNotFoundError(f"no .mat files in {data_dir} [{start}:{stop}]")
    items = [load_mat(os.path.join(data_dir, f)) for f in fns]
    h, w = items[0]["mask"].shape[-2:]
    for f, it in zip(fns, items):
        if it["mask"].shape[-2:] != (h, w) or not np.array_equal(it["mask"] != 0, items[0]["mask"] != 0):
            raise ValueError(f"{f}: all files of one batch must share size and sampling mask")
    batch = {k: np.stack([it[k].reshape(1, h, w, 2) for it in items]).astype(np.float32) for k in ("x0", "y0", "ATy0")}
    batch["gt"] = np.stack([it["gt"].reshape(1, h, w) for it in items]).astype(np.float32)
    batch["x0_raw"] = np.stack([it["x0_raw"].reshape(1, h, w) for it in items]).astype(np.float32)
    batch["mask"] = items[0]["mask"].reshape(h, w) != 0
    return batch, [task_from_filename(f) for f in fns]


def _gt_index(gt_dir: str, limit: int = 0) -> List[Tuple[str, int, Tuple[int, int]]]:
    """(file, images in it, (H, W)) for the `.npy` / `.mat` files of a directory, sorted by name, cut after the first `limit`
    images; only headers are read."""
    out, total = [], 0
    for f in sorted(os.listdir(gt_dir)):
        path = os.path.join(gt_dir, f)
        if f.endswith(".npy"):
            shape = np.load(path, mmap_mode="r").shape
        elif f.endswith(".mat"):
            from scipy.io import whosmat
            found = [sh for name, sh, _ in whosmat(path) if name == "gt"]
            if not found:
                raise KeyError(f"{path}: no 'gt' key")
            shape = tuple(found[0])
        else:
            continue
        if len(shape) == 2:
            shape = (1,) + tuple(shape)
        if len(shape) != 3:
            raise ValueError(f"{path}: expected [H,W] or [n,H,W], got {tuple(shape)}")
        n = int(shape[0])
        if limit and total + n > limit:
            n = limit - total
        if n > 0:
            out.append((f, n, (int(shape[1]), int(shape[2]))))
            total += n
        if limit and total >= limit:
            break
    if not out:
        raise FileNotFoundError(f"no .npy / .mat ground-truth files in {gt_dir}")
    sizes = {hw for _, _, hw in out}
    if len(sizes) != 1:
        raise ValueError(f"{gt_dir}: all images of one folder must share one size, found {sorted(sizes)}")
    return out


gt_index = _gt_index


def count_gt_dir(gt_dir: str, limit: int = 0) -> int:
    """Number of ground-truth images `load_gt_dir(gt_dir, limit)` would return."""
    return sum(n for _, n, _ in _gt_index(gt_dir, limit))


def load_gt_dir(gt_dir: str, limit: int = 0, start: int = 0, stop: int = None, index=None) -> Tuple[np.ndarray, List[str]]:
    """Ground-truth images [start, stop) of a folder (of its first `limit` images; files sorted by name): float32 [N,1,H,W] and
    one name per image.  Reads `.npy` files ([H,W] or [n,H,W], any float type) and `.mat` files with a `gt` key ([H,W], [1,H,W] or
    [n,H,W]); a rank of a sharded run opens only the files its range touches.  Mixed sizes and values outside [0, 1] are refused
    (the acquisition and the PSNR both assume the reference's unit range).  index: what `gt_index(gt_dir, limit)` returned, for a
    caller that reads one folder in several ranges (the headers are then read once)."""
    if index is None:
        index = _gt_index(gt_dir, limit)
    total = sum(n for _, n, _ in index)
    stop = total if stop is None else min(stop, total)
    if not 0 <= start < stop:
        raise FileNotFoundError(f"no ground-truth images in {gt_dir} [{start}:{stop}]")
    imgs, names, first = [], [], 0
    for f, n, (h, w) in index:
        a, b = max(start, first), min(stop, first + n)
        if a < b:
            path = os.path.join(gt_dir, f)
            if f.endswith(".npy"):
                arr = np.load(path, mmap_mode="r")
            else:
                from scipy.io import loadmat
                arr = loadmat(path)["gt"]
            if not np.issubdtype(arr.dtype, np.floating):
                raise ValueError(f"{path}: expected a float array, got {arr.dtype}")
            arr = np.asarray(arr.reshape(-1, h, w)[a - first:b - first], dtype=np.float32)
            if not np.isfinite(arr).all() or arr.min() < 0.0 or arr.max() > 1.0:
                raise ValueError(f"{path}: ground-truth values must lie in [0, 1] (found {arr.min():g} .. {arr.max():g})")
            imgs.append(arr)
            stem = os.path.splitext(f)[0]
            names += [stem if n == 1 else f"{stem}-{i:04d}" for i in range(a - first, b - first)]
        first += n
    return np.concatenate(imgs).reshape(-1, 1, h, w), names


def task_tokens(tasks: Sequence[str], flex_target: float = None) -> np.ndarray:
    if flex_target is not None:
        key = "rtg_" + (str(int(flex_target)) if float(flex_target).is_integer() else str(flex_target))
        return np.full(len(tasks), FLEX_TASKS.index(key), dtype=np.int64)
    return np.array([OPTIMAL_TASKS.index(t) for t in tasks], dtype=np.int64)
