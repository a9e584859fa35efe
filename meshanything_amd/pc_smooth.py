"""Smoothing of noisy input clouds (`--smooth_radius`): project every point onto the plane fitted to its radius neighbourhood (DESIGN.md
section 17); PCL's MovingLeastSquares without the polynomial is the same operation.

The other cleaning steps (outlier filter, plane removal, clustering) remove rows; none moves one.  A scan's measurement noise on the
surface itself therefore reaches the encoder, and the normals `pc_xyz` fits to 16 jittered neighbours inherit it.  `smooth_points` is the
one call into the HIP library (csrc/pc_smooth.hpp; C ABI ma_op_pc_smooth, whose header comment states the rule): the cell grid and ring
walk of the clustering, per point the weighted moments of its neighbourhood in float64 registers, the Jacobi solve of the normal
estimate, and the projection, all in one kernel; no neighbour list is stored.  `smooth_rows` is what `data.Dataset` calls.  A plane
projection shrinks a curved surface by roughly radius^2 / (8 * its radius of curvature) and rounds an edge over a width of the radius;
no polynomial fit is made.  It needs CUDA tensors; there is no CPU fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .pc_cluster import check_max_pairs, check_pair_bound, check_radius, check_radius_grid, choose_cluster_grid, grid_workspace
from .pc_common import check_device_cloud, check_host_cloud, check_int, check_want, cuda_device, is_int, need_cuda

MIN_COUNT = 3                                                    # MA_PC_SMOOTH_MIN_COUNT: the points a plane takes
DEFAULT_MIN_COUNT = 6
MAX_ITERS = 8
WANT = ("moved", "normals", "eigvals", "count")


def smooth_points(points: torch.Tensor, radius, min_count=DEFAULT_MIN_COUNT, grid=None, want=("moved",), max_pairs=None):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns, finite -> a dict with the entries named in `want`: "moved"
    (N, 3) float64, every row projected onto the plane fitted to the rows within `radius` of it (weights (1 - d^2 / r^2)^3, the plane
    through their weighted centroid, ma_op_pc_smooth); "normals" (N, 3) float64, that plane's unit normal, its component of largest
    magnitude positive; "eigvals" (N, 3) float64, the weighted covariance's eigenvalues ascending; "count" (N) int32, the rows within
    the radius, the row itself included.  A row with count < min_count (>= 3), or whose neighbours all coincide, stays where it is
    with normal (0, 0, 1) and eigenvalues 0.  grid: (origin, cell, dims) with radius / cell <= 8, None = `choose_cluster_grid` of the
    points (copied to the host for it); count does not depend on it, the float outputs only in the order of their sums.  max_pairs:
    the cap on the pair bound the library computes before it searches (None = its own, 2^36); a bound above it is a ValueError that
    names both."""
    radius = check_radius(radius)
    check_device_cloud(points, 1)
    if not is_int(min_count) or not MIN_COUNT <= int(min_count) < 1 << 31:
        raise ValueError(f"min_count must be an integer >= {MIN_COUNT}, got {min_count!r}")
    want = check_want(want, WANT)
    cap = check_max_pairs(max_pairs)
    grid = check_radius_grid(grid, radius)
    need_cuda(points, "smooth_points")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        N = ref.shape[0]
        grid_args, ws, nbytes = grid_workspace(lib, "smooth", ref, radius, grid)
        out = {w: torch.empty(N, dtype=torch.int32, device=dev) if w == "count" else torch.empty((N, 3), dtype=torch.float64, device=dev) for w in want}
        ptr = [out[w].data_ptr() if w in out else None for w in WANT]
        bound = C.c_uint64(0)
        rc = lib.ma_op_pc_smooth(ref.data_ptr(), N, ref.shape[1], radius, *grid_args, int(min_count), cap, *ptr, C.byref(bound), ws.data_ptr(), nbytes,
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        check_pair_bound("smooth_points", rc, bound.value, cap, N, radius)
        _lib.check(rc)
    return {w: out[w] for w in WANT if w in want}


def check_smooth_args(radius, iters) -> tuple:
    """The checks on (radius, iters); returns them as (float, int)."""
    radius = check_radius(radius)
    return radius, check_int("iters", iters, 1, MAX_ITERS)


def stayed(count, eigvals, min_count=DEFAULT_MIN_COUNT):
    """The rows a pass left where they were, from its count (N) and eigvals (N, 3): too few neighbours, or no plane (all eigenvalues 0)."""
    return (np.asarray(count) < min_count) | (np.asarray(eigvals) == 0).all(axis=1)


def smooth_rows(rows, radius, iters, uid: str, device="cuda") -> np.ndarray:
    """rows (N, >= 3) host array -> an array of the same shape and dtype with xyz replaced by `smooth_points`' "moved" after `iters`
    passes (min_count 6): the first pass runs on the float32 cast of xyz, every later one on the float32 cast of the pass before, over
    the first pass's grid, without leaving the device.  With 6 columns or more, columns 3:6 (the file's normals) are replaced by the
    last pass's normal, negated where its dot product with the file's normal is negative; where the last pass left the row in place
    they are kept.  Every other column is kept.  Prints the smoothing line of the command line."""
    radius, iters = check_smooth_args(radius, iters)
    rows = check_host_cloud(rows, "smoothing")
    dev = cuda_device(device, "smooth_rows")
    host = np.ascontiguousarray(rows[:, :3], dtype=np.float32)
    grid = choose_cluster_grid(host, radius)
    with torch.cuda.device(dev):
        cur = torch.from_numpy(host).to(dev)
        for it in range(iters):
            got = smooth_points(cur, radius, DEFAULT_MIN_COUNT, grid, want=WANT if it == iters - 1 else ("moved",))
            cur = got["moved"].to(torch.float32)
        moved, normals, eigvals, count = (got[w].cpu().numpy() for w in WANT)
    out = rows.copy()
    out[:, :3] = moved.astype(rows.dtype)
    if rows.shape[1] >= 6:
        fit = ~stayed(count, eigvals)
        side = np.einsum("ij,ij->i", normals, rows[:, 3:6].astype(np.float64)) < 0
        normals[side] *= -1.0
        out[fit, 3:6] = normals[fit].astype(rows.dtype)
    step = np.linalg.norm(moved - host.astype(np.float64), axis=1)
    print(f"{uid}: smoothing (radius {radius:g}, {iters} pass{'es' if iters > 1 else ''}) left {int((count < DEFAULT_MIN_COUNT).sum())} of {rows.shape[0]} "
          f"rows in place for lack of neighbours, mean displacement {float(step.mean()):.6g}, largest {float(step.max()):.6g}")
    return out
