"""Statistical outlier removal for input clouds (`--outlier_k`): drop the points whose mean distance to their k nearest neighbours
exceeds the cloud's mean of that figure by more than `std_ratio` standard deviations.

One stray point shrinks the object inside the encoder's unit box (`data.normalize_pc` scales by the bounding box), and farthest-point
sampling picks strays first, by construction; scans and fused depth maps carry them.  The filter needs the k neighbours of EVERY point.
`grid_knn` is the one call into the HIP library for that (csrc/pc_grid.hpp; C ABI ma_op_pc_knn_grid, whose header comment states the
contract): a uniform cell grid built on the GPU and a search over it whose lists equal the brute force's (`pc_normals.knn`) bit for bit,
whatever the grid.  `choose_grid` fits the grid to the object on the host.  It needs CUDA tensors; there is no CPU fallback.  There is
no reference counterpart.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_common import (MAX_DIM, MAX_POINTS, MAX_QUERIES, as_host_cloud, check_device_cloud, check_finite, check_grid, check_want, cuda_device, is_int,
                        is_real, need_cuda, upload_xyz)
from .pc_normals import check_k, knn

GRID_SAMPLE = 1 << 16                                            # rows choose_grid looks at, at the most
FORM_AUTO, FORM_BRUTE, FORM_GRID = 0, 1, 2
GRID_FROM_N = 1 << 18                                            # form 0: the grid from this many points on
POINTS_PER_ALONG_SQUARED = 256                                   # choose_grid: sqrt(N / 256) cells along the longest axis (the sweep of section 14)
WANT = ("idx", "d2", "mean")


def choose_grid(xyz, k: int = 16, along=None):
    """xyz (N, >= 3) host array, finite -> (origin (3) float32, cell float32, dims (3) int32) for `grid_knn`: the box is the per-axis
    1st to 99th percentile of a strided subsample of at most 65 536 rows, so that it follows the object and not its strays (points
    outside it fall into the border cells), widened by one cell on every side; the cells are cubes, about sqrt(N / 256) of them along
    the longest axis, 1 .. 128: a few hundred points in each occupied cell of a surface, which is what the sweep of DESIGN.md section
    14 supports once a cloud has strays, whose searches walk many empty cells.  A function of the array alone: no random numbers.  The grid only decides the time of the search, never its result.  along: that number of cells instead (the sweep
    of scripts/time_pc_outliers.py)."""
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] < 3 or xyz.shape[0] < 1:
        raise ValueError(f"a point cloud must be a (N, >= 3) array, got {xyz.shape}")
    check_k(k)
    N = xyz.shape[0]
    sub = np.asarray(xyz[::max(1, -(-N // GRID_SAMPLE)), :3], dtype=np.float64)
    lo, hi = np.percentile(sub, 1.0, axis=0), np.percentile(sub, 99.0, axis=0)
    extent = hi - lo
    longest = float(extent.max())
    along = int(min(max(round(math.sqrt(N / POINTS_PER_ALONG_SQUARED)) if along is None else int(along), 1), MAX_DIM))
    cell = np.float32(longest / max(along - 2, 1))
    if not (np.isfinite(cell) and cell > np.finfo(np.float32).tiny and np.isfinite(lo).all()):      # one position, or nothing to fit to
        return np.asarray(lo if np.isfinite(lo).all() else np.zeros(3), np.float32), np.float32(1.0), np.ones(3, np.int32)
    dims = np.clip(np.ceil(extent / float(cell)).astype(np.int64) + 2, 1, MAX_DIM).astype(np.int32)
    origin = (lo - float(cell)).astype(np.float32)
    return origin, cell, dims


def grid_knn(points: torch.Tensor, k: int = 16, grid=None, want=("idx", "d2")):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns; every row is a query -> a dict with the entries named in
    `want`: "idx" (N, k) int32 and "d2" (N, k) float32, the lists `pc_normals.knn(points, None, k)` returns, bit for bit, and "mean"
    (N) float64, the mean of sqrt(d2) over each list (ma_op_pc_knn_grid).  With want = ("mean",) the lists are never written to
    memory.  grid: (origin, cell, dims), None = `choose_grid` of the points (copied to the host for it); the result does not depend on
    it.  Unlike `knn`, N may reach 2^22."""
    k = check_k(k)
    check_device_cloud(points, k, "k")
    want = check_want(want, WANT)
    if grid is not None:
        grid = check_grid(grid)
    need_cuda(points, "grid_knn")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        N = ref.shape[0]
        origin, cell, dims = grid if grid is not None else choose_grid(ref[:, :3].cpu().numpy(), k)
        nbytes = lib.ma_pc_knn_grid_workspace_bytes(N, k, int(dims[0]), int(dims[1]), int(dims[2]))
        if nbytes == 0:
            raise ValueError(f"outside the limits of ma_op_pc_knn_grid: N = {N}, k = {k}, dims = {dims.tolist()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = {}
        if "idx" in want:
            out["idx"] = torch.empty((N, k), dtype=torch.int32, device=dev)
        if "d2" in want:
            out["d2"] = torch.empty((N, k), dtype=torch.float32, device=dev)
        if "mean" in want:
            out["mean"] = torch.empty(N, dtype=torch.float64, device=dev)
        ptr = {w: (out[w].data_ptr() if w in out else None) for w in WANT}
        _lib.check(lib.ma_op_pc_knn_grid(ref.data_ptr(), N, ref.shape[1], k, (C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist()),
                                         ptr["idx"], ptr["d2"], ptr["mean"], ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _check_form(form) -> int:
    if not is_int(form) or int(form) not in (FORM_AUTO, FORM_BRUTE, FORM_GRID):
        raise ValueError(f"form must be 0 (automatic), 1 (brute force) or 2 (cell grid), got {form!r}")
    return int(form)


def resolve_form(N: int, form: int) -> int:
    """form 0 is a function of N alone: the grid where DESIGN.md section 14 measured it ahead of the brute force with and without
    strays, from 2^18 points on"""
    if form != FORM_AUTO:
        return form
    return FORM_GRID if N >= GRID_FROM_N else FORM_BRUTE


def knn_mean_distance(points: torch.Tensor, k: int = 16, form: int = 0) -> torch.Tensor:
    """points (N, 3 | 6) float32 on the GPU -> (N) float64 on the GPU: per point the mean distance to its k nearest neighbours, itself
    included at distance 0: (sum_j sqrt((double) d2_j)) / k in list order.  form: 1 = the brute force (`pc_normals.knn` and the same
    sum, N <= 2^20), 2 = the cell grid (`grid_knn`, N <= 2^22), 0 = a function of N alone.  The values do not depend on it, bit for
    bit."""
    k = check_k(k)
    check_device_cloud(points, k, "k")
    form = resolve_form(points.shape[0], _check_form(form))
    if form == FORM_BRUTE and points.shape[0] > MAX_QUERIES:
        raise ValueError(f"form 1 (brute force) takes at most 2^20 points, got N = {points.shape[0]}")
    need_cuda(points, "knn_mean_distance")
    if form == FORM_GRID:
        return grid_knn(points, k, None, want=("mean",))["mean"]
    _, d2 = knn(points, None, k)
    total = torch.zeros(points.shape[0], dtype=torch.float64, device=points.device)
    for j in range(k):                                           # in list order, one rounded addition each, as the kernel sums
        total = total + torch.sqrt(d2[:, j].to(torch.float64))
    return total / torch.full_like(total, float(k))              # a tensor divisor: a true division, as the kernel's (a scalar one becomes a multiplication by 1 / k)


def check_filter_args(k, std_ratio, form=0) -> tuple:
    """The checks on (k, std_ratio, form); returns them as (int, float, int)."""
    k = check_k(k)
    if not is_real(std_ratio) or not (0.0 <= float(std_ratio) < float("inf")):
        raise ValueError(f"std_ratio must be finite and >= 0, got {std_ratio!r}")
    return k, float(std_ratio), _check_form(form)


def check_outlier_args(xyz, k, std_ratio, form=0) -> np.ndarray:
    """The checks of remove_statistical_outliers that need no device; returns xyz as an array."""
    xyz = as_host_cloud(xyz)
    k, _, form = check_filter_args(k, std_ratio, form)
    if not k <= xyz.shape[0] <= MAX_POINTS:
        raise ValueError(f"outlier removal needs k <= N <= 2^22 points, got N = {xyz.shape[0]} with k = {k}")
    if form == FORM_BRUTE and xyz.shape[0] > MAX_QUERIES:
        raise ValueError(f"form 1 (brute force) takes at most 2^20 points, got N = {xyz.shape[0]}")
    check_finite(xyz)
    return xyz


def remove_statistical_outliers(xyz, k: int = 16, std_ratio: float = 2.0, device="cuda", form: int = 0):
    """xyz (N, >= 3) host array, only the first three columns are read (uploaded as float32) -> (keep (N) bool, mean_dist (N) float64,
    threshold): mean_dist from `knn_mean_distance` on the GPU, then on the host threshold = mean_dist.mean() + std_ratio *
    mean_dist.std() (numpy float64, population sigma) and keep = mean_dist <= threshold."""
    xyz = check_outlier_args(xyz, k, std_ratio, form)
    dev = cuda_device(device, "remove_statistical_outliers")
    with torch.cuda.device(dev):
        m = knn_mean_distance(upload_xyz(xyz, dev), int(k), int(form)).cpu().numpy()
    threshold = float(m.mean() + float(std_ratio) * m.std())
    return m <= threshold, m, threshold


def filter_rows(xyz, k: int, std_ratio: float, n_points: int, uid: str, device="cuda") -> np.ndarray:
    """The rows of xyz that survive the filter, in their order; prints the removal line of the command line.  Fewer than n_points
    survivors is a ValueError."""
    keep, _, threshold = remove_statistical_outliers(xyz, k, std_ratio, device=device)
    kept = int(keep.sum())
    print(f"{uid}: outlier filter removed {keep.shape[0] - kept} of {keep.shape[0]} points (k = {k}, threshold {threshold:.6g})")
    if kept < n_points:
        raise ValueError(f"{uid}: only {kept} of {keep.shape[0]} points survive the outlier filter, fewer than the {n_points} the encoder takes")
    return xyz[keep]
