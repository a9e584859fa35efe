"""Euclidean clustering of input clouds (`--cluster_radius`): split a cloud into the connected components of the graph that links two
points when they are at most `radius` apart; PCL's EuclideanClusterExtraction is the same operation.

The statistical outlier filter cannot see a floating clump of a few hundred points: it is locally as dense as the object.  Such a clump
sets the scale of `data.normalize_pc` and farthest-point sampling picks it first; and a file that holds two objects is useless as one
cloud to a model that meshes one object.  `euclidean_clusters` is the one call into the HIP library (csrc/pc_cluster.hpp; C ABI
ma_op_pc_cluster, whose header comment states the contract): the cell grid of the outlier filter, a ring walk with an exact stop rule and
a lock-free union-find; labels[i] is the smallest row of i's component, whatever the grid.  `choose_cluster_grid` fits the grid on the
host, `components` and `split_rows` turn the labels into the parts `data.Dataset` makes items of.  It needs CUDA tensors; there is no CPU
fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_common import MAX_DIM, check_device_cloud, check_grid, check_host_cloud, check_want, cuda_device, is_int, is_real, need_cuda
from .pc_outliers import choose_grid

MAX_PAIRS = 1 << 36                                              # MA_PC_CLUSTER_MAX_PAIRS
MAX_RADIUS_IN_CELLS = 8                                          # ma_op_pc_cluster: radius / cell <= 8
WANT = ("labels", "sizes")
MODES = ("largest", "split")


def check_radius(radius) -> float:
    if not is_real(radius) or not (0.0 < float(radius) < float("inf")):
        raise ValueError(f"radius must be finite and > 0, got {radius!r}")
    if not np.isfinite(np.float32(radius)) or not np.float32(radius) > 0:
        raise ValueError(f"radius must be a positive finite float32, got {radius!r}")
    return float(radius)


def choose_cluster_grid(xyz, radius):
    """xyz (N, >= 3) host array, finite -> (origin (3) float32, cell float32, dims (3) int32) for `euclidean_clusters`: the box of
    `pc_outliers.choose_grid` (the 1st to 99th percentile of a subsample, widened by one cell) with the number of cells along the longest
    axis the largest that keeps cell >= radius, 128 at the most: a search then ends after two rings, and the cells hold as few points as
    that allows.  choose_grid's cell is longest / (along - 2), so along = floor(longest / radius) + 2; capped at 128 the cell only grows,
    and at most 128 cells an axis are at most 2^21 cells, so the limits always allow it.  A radius beyond the box's longest side: that
    box at three cells an axis with cell = radius.  A box without extent: one cell.  A function of the array and the radius alone: no
    random numbers.  The grid only decides the time."""
    radius = check_radius(radius)
    r32 = np.float32(radius)
    if float(r32) < radius:
        r32 = np.nextafter(r32, np.float32(np.inf))
    origin, longest, dims = choose_grid(xyz, 16, along=3)        # along = 3: the cell is the box's longest side
    if int(dims.max()) == 1:                                     # one position, or nothing to fit to
        return origin, np.float32(max(float(longest), float(r32))), dims
    if float(longest) < radius:
        return origin, r32, dims                                 # the same origin and dims with a larger cell: a larger box
    along = int(min(math.floor(float(longest) / radius) + 2, MAX_DIM))
    while True:
        origin, cell, dims = choose_grid(xyz, 16, along=along)
        if float(cell) >= radius or along <= 3:                  # (the float32 rounding of the cell can cost one step)
            return origin, cell, dims
        along -= 1


# ---- what every radius search over the grid shares (euclidean_clusters, pc_smooth.smooth_points, pc_upsample.upsample_points) ----------
def check_max_pairs(max_pairs) -> int:
    """The check on max_pairs; returns the cap the library takes, 0 = its own."""
    if max_pairs is not None and (not is_int(max_pairs) or not 1 <= int(max_pairs) < 1 << 64):
        raise ValueError(f"max_pairs must be None or an integer in 1..2^64 - 1, got {max_pairs!r}")
    return 0 if max_pairs is None else int(max_pairs)


def check_radius_grid(grid, radius):
    """An explicit grid, checked as `pc_common.check_grid` does and against the ratio rule; None stays None."""
    if grid is None:
        return None
    grid = check_grid(grid)
    if not radius / float(grid[1]) <= MAX_RADIUS_IN_CELLS:
        raise ValueError(f"the grid's cell must be at least radius / {MAX_RADIUS_IN_CELLS}, got cell {float(grid[1])} for radius {radius}")
    return grid


def grid_workspace(lib, op: str, ref: torch.Tensor, radius: float, grid):
    """For ma_op_pc_<op> on the contiguous device cloud `ref`: the grid (None = `choose_cluster_grid` of a host copy, which must be
    finite) as the three ctypes arguments (origin, cell, dims), and the workspace -> (grid arguments, workspace tensor, its bytes)."""
    N = ref.shape[0]
    if grid is None:
        host = ref[:, :3].cpu().numpy()
        if not np.isfinite(host).all():
            raise ValueError("the point cloud has non-finite coordinates")
        grid = choose_cluster_grid(host, radius)
    origin, cell, dims = grid
    nbytes = getattr(lib, f"ma_pc_{op}_workspace_bytes")(N, int(dims[0]), int(dims[1]), int(dims[2]))
    if nbytes == 0:
        raise ValueError(f"outside the limits of ma_op_pc_{op}: N = {N}, dims = {dims.tolist()}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ref.device)
    return ((C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist())), ws, nbytes


def check_pair_bound(fn: str, rc: int, bound: int, cap: int, N: int, radius: float):
    """The library refused the call because its pair bound exceeds the cap: a ValueError that names both."""
    if rc != _lib.MA_OK and bound > (cap or MAX_PAIRS):
        raise ValueError(f"{fn}: the pair bound {bound} exceeds max_pairs {cap or MAX_PAIRS} (N = {N}, radius {radius}): "
                         "use a smaller radius or fewer points")


def euclidean_clusters(points: torch.Tensor, radius, grid=None, want=("labels",), max_pairs=None):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns, finite -> a dict with the entries named in `want`: "labels"
    (N) int32, labels[i] = the smallest row index in the connected component of i, rows i and j being linked iff
    fl32(fl32(dx*dx + dy*dy) + dz*dz) <= fl32(radius * radius) (ma_op_pc_cluster), and "sizes" (N) int32, the number of rows of the
    component at its root and 0 elsewhere.  grid: (origin, cell, dims) with radius / cell <= 8, None = `choose_cluster_grid` of the
    points (copied to the host for it); the result does not depend on it.  max_pairs: the cap on the pair bound the library computes
    before it searches (None = its own, 2^36); a bound above it is a ValueError that names both."""
    radius = check_radius(radius)
    check_device_cloud(points, 1)
    want = check_want(want, WANT)
    cap = check_max_pairs(max_pairs)
    grid = check_radius_grid(grid, radius)
    need_cuda(points, "euclidean_clusters")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        N = ref.shape[0]
        grid_args, ws, nbytes = grid_workspace(lib, "cluster", ref, radius, grid)
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        sizes = torch.empty(N, dtype=torch.int32, device=dev) if "sizes" in want else None
        bound = C.c_uint64(0)
        rc = lib.ma_op_pc_cluster(ref.data_ptr(), N, ref.shape[1], radius, *grid_args, cap, labels.data_ptr(), None if sizes is None else sizes.data_ptr(),
                                  C.byref(bound), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        check_pair_bound("euclidean_clusters", rc, bound.value, cap, N, radius)
        _lib.check(rc)
    out = {"labels": labels, "sizes": sizes}
    return {w: out[w] for w in WANT if w in want}


def components(labels):
    """labels (N) host integers -> (roots (C), counts (C)) int64, ordered by count descending, then root ascending."""
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"labels must be a (N) integer array, got {labels.shape} {labels.dtype}")
    roots, counts = np.unique(labels.astype(np.int64), return_counts=True)
    order = np.lexsort((roots, -counts))
    return roots[order], counts[order].astype(np.int64)


def check_split_args(radius, min_points, mode) -> tuple:
    """The checks on (radius, min_points, mode); returns them as (float, int, str)."""
    radius = check_radius(radius)
    if not is_int(min_points) or int(min_points) < 1:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points!r}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    return radius, int(min_points), mode


def split_rows(xyz, radius, min_points, mode, uid: str, device="cuda"):
    """xyz (N, >= 3) host array, only the first three columns are read (uploaded as float32) -> a list of row-index arrays (int64), one
    per kept component: the components of `euclidean_clusters` with at least min_points rows, in the order of `components`, each in the
    file's row order; mode "largest" keeps the first only.  Prints the clustering line of the command line.  No component of
    min_points rows is a ValueError that names the largest size."""
    radius, min_points, mode = check_split_args(radius, min_points, mode)
    xyz = check_host_cloud(xyz, "clustering")
    dev = cuda_device(device, "split_rows")
    host = np.ascontiguousarray(xyz[:, :3], dtype=np.float32)
    grid = choose_cluster_grid(host, radius)
    with torch.cuda.device(dev):
        labels = euclidean_clusters(torch.from_numpy(host).to(dev), radius, grid)["labels"].cpu().numpy()
    roots, counts = components(labels)
    if int(counts[0]) < min_points:
        raise ValueError(f"{uid}: clustering (radius {radius:g}) found no component of {min_points} points: the largest of {roots.shape[0]} has {int(counts[0])}")
    keep = int((counts >= min_points).sum()) if mode == "split" else 1
    parts = [np.flatnonzero(labels == roots[c]) for c in range(keep)]
    kept = int(counts[:keep].sum())
    print(f"{uid}: clustering (radius {radius:g}) found {roots.shape[0]} components, kept {keep} (sizes {' '.join(str(int(c)) for c in counts[:keep])}), "
          f"dropped {xyz.shape[0] - kept} of {xyz.shape[0]} points")
    return parts
