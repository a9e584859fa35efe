"""Upsampling of sparse input clouds (`--upsample_radius`): every point with a fitted plane seeds a disc of lattice points in that plane,
and a lattice point is kept where its seed is the nearest input point; PCL's MovingLeastSquares with
SAMPLE_LOCAL_PLANE upsampling is the same operation, plus that Voronoi restriction.

The encoder takes 4096 points, and every other step of the input side refuses a cloud with fewer: a ModelNet cloud of 1024 points, or
the part that plane removal and clustering leave of a scan.  `upsample_points` is the one call into the HIP library
(csrc/pc_upsample.hpp; C ABI ma_op_pc_upsample, whose header comment states the rule): one workgroup per seed over the cell grid of the
clustering, a count pass, a 64-bit scan and an emit pass, no atomics; its outputs are a function of its inputs alone and EQUAL a numpy
restatement.  `upsample_rows` is what `data.Dataset` calls: one plane fit (`pc_smooth.smooth_points`), then the smallest lattice of the
ladder m = 2, 4, ..., 64 that reaches the target.  Consequences of the rule: the patches are flat; an open border grows outward by up to
the radius; at a sharp edge the fitted plane is diagonal and the patch sticks out; choose the radius at about one to two point spacings.
The patches differ in size, so follow it with farthest-point sampling (`--point_sampling fps`), which thins evenly.  It needs CUDA
tensors; there is no CPU fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .pc_cluster import check_max_pairs, check_pair_bound, check_radius, check_radius_grid, choose_cluster_grid, grid_workspace
from .pc_common import MAX_POINTS, check_device_cloud, check_host_cloud, check_int, cuda_device, is_int, need_cuda
from .pc_smooth import DEFAULT_MIN_COUNT, smooth_points, stayed

MAX_M = 64                                                       # MA_PC_UPSAMPLE_MAX_M
MAX_SLOTS = 1 << 31                                              # ma_op_pc_upsample: N * (2m+1)^2
LADDER = (2, 4, 8, 16, 32, 64)
MIN_ROWS = 64                                                    # the floor of the input side when upsampling is on
N_POINTS = 4096                                                  # the rows the encoder takes
DEFAULT_TARGET = 4 * N_POINTS


def lattice_size(m: int) -> int:
    """The candidates of one seed: the (a, b) != (0, 0) in -m..m with a^2 + b^2 <= m^2."""
    a = np.arange(-m, m + 1, dtype=np.int64)
    return int((a[:, None] ** 2 + a[None, :] ** 2 <= m * m).sum()) - 1


def upsample_points(points: torch.Tensor, normals: torch.Tensor, radius, m, active=None, grid=None, count_only=False, capacity=None, max_pairs=None):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns; normals (N, 3) float64 on the same GPU, a unit normal per
    row; active (N) bool or uint8 on the same GPU, or None = every row -> a dict: "xyz" (T, 3) float32, the lattice points at spacing
    radius / m within `radius` of an active row, in its plane, to which that row is the nearest of all rows (ties to the lower index;
    ma_op_pc_upsample states the rule); "seed" (T) int32, the row each came from; "counts" (N) int32, how many each row gave; "total" = T
    (int).  Seed-major, in lattice order inside a seed.  count_only: "xyz" and "seed" are None and nothing but the counts is computed.
    grid: (origin, cell, dims) with radius / cell <= 8, None = `choose_cluster_grid` of the points (copied to the host for it); no
    output depends on it.  capacity: the rows to allocate for the output, None = min(N * lattice_size(m), 2^22 - N); a total above it,
    or above 2^22 - N, is a ValueError.  max_pairs: as in `smooth_points`."""
    radius = check_radius(radius)
    m = check_int("m", m, 1, MAX_M)
    check_device_cloud(points, 1)
    N = points.shape[0]
    if not torch.is_tensor(normals) or normals.dtype != torch.float64 or tuple(normals.shape) != (N, 3):
        raise ValueError(f"normals must be a float64 ({N}, 3) tensor, got "
                         f"{(tuple(normals.shape), normals.dtype) if torch.is_tensor(normals) else type(normals).__name__}")
    if active is not None and (not torch.is_tensor(active) or active.dtype not in (torch.bool, torch.uint8) or tuple(active.shape) != (N,)):
        raise ValueError(f"active must be None or a bool / uint8 ({N},) tensor, got "
                         f"{(tuple(active.shape), active.dtype) if torch.is_tensor(active) else type(active).__name__}")
    if N * (2 * m + 1) ** 2 > MAX_SLOTS:
        raise ValueError(f"N * (2m+1)^2 must be at most 2^31, got N = {N}, m = {m}")
    if capacity is not None and (not is_int(capacity) or not 0 <= int(capacity) <= MAX_POINTS):
        raise ValueError(f"capacity must be None or an integer in 0..2^22, got {capacity!r}")
    cap = check_max_pairs(max_pairs)
    grid = check_radius_grid(grid, radius)
    need_cuda(points, "upsample_points")
    if normals.device != points.device or (active is not None and active.device != points.device):
        raise ValueError("points, normals and active must be on the same device")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        nrm = normals.contiguous()
        act = None if active is None else active.to(torch.uint8).contiguous()
        grid_args, ws, nbytes = grid_workspace(lib, "upsample", ref, radius, grid)
        counts = torch.empty(N, dtype=torch.int32, device=dev)
        rows = 0 if count_only else (min(N * lattice_size(m), MAX_POINTS - N) if capacity is None else int(capacity))
        xyz = None if count_only else torch.empty((rows, 3), dtype=torch.float32, device=dev)
        seed = None if count_only else torch.empty(rows, dtype=torch.int32, device=dev)
        total, bound = C.c_uint64(0), C.c_uint64(0)
        rc = lib.ma_op_pc_upsample(ref.data_ptr(), N, ref.shape[1], nrm.data_ptr(), None if act is None else act.data_ptr(), m, radius / m, *grid_args, cap,
                                   counts.data_ptr(), None if count_only else xyz.data_ptr(), None if count_only else seed.data_ptr(), rows,
                                   C.byref(total), C.byref(bound), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        check_pair_bound("upsample_points", rc, bound.value, cap, N, radius)
        if rc != _lib.MA_OK and not count_only and total.value > min(rows, MAX_POINTS - N):
            raise ValueError(f"upsample_points: the total {total.value} exceeds {'2^22 - N' if total.value > MAX_POINTS - N else 'the capacity'} = "
                             f"{min(rows, MAX_POINTS - N)} (N = {N}, radius {radius}, m = {m}): use a smaller m or radius")
        _lib.check(rc)
    T = int(total.value)
    return {"xyz": None if count_only else xyz[:T], "seed": None if count_only else seed[:T], "counts": counts, "total": T}


def check_upsample_args(radius, target, n_points: int = N_POINTS) -> tuple:
    """The checks on (radius, target); returns them as (float, int)."""
    radius = check_radius(radius)
    if not is_int(target) or not n_points <= int(target) <= MAX_POINTS:
        raise ValueError(f"the upsampling target must be an integer in {n_points}..2^22, got {target!r}")
    return radius, int(target)


def choose_m(count, N: int, target: int, radius: float) -> tuple:
    """The ladder: the first m of 2, 4, ..., 64 with N + count(m) >= target -> (m, count(m)).  `count(m)` is a count-only call.  A
    lattice that would pass N * (2m+1)^2 = 2^31 ends the ladder like m = 64 does: a ValueError that names N, the total reached and
    the radius."""
    total, reached = 0, None
    for m in LADDER:
        if N * (2 * m + 1) ** 2 > MAX_SLOTS:
            break
        total, reached = int(count(m)), m
        if N + total >= target:
            return m, total
    raise ValueError(f"upsampling {N} rows at radius {radius:g} reaches {N + total} rows" + (f" at m = {reached}" if reached else "") +
                     f", fewer than the {target} asked for: use a larger radius (about one to two point spacings)")


def upsample_rows(rows, radius, target, uid: str, device="cuda", return_fit=False):
    """rows (N, >= 3) host array -> an array of the same dtype and columns with at least `target` rows: the N input rows first, bit for
    bit, then one row per kept candidate of `upsample_points`, a copy of its seed's row (a pc_normal file's normals and any further
    column are the seed's) with xyz replaced by the candidate, cast to the file's dtype.  The planes come from one
    `smooth_points(..., want=("normals", "eigvals", "count"))` call on the float32 cast of xyz at the same radius; a row that call
    left without a plane seeds nothing.  m is the first of 2, 4, ..., 64 that reaches the target (`choose_m`).  N >= target: the rows
    come back unchanged.  Prints the upsampling line of the command line.  return_fit: also return the dict of the fit ("normals"
    (N, 3) float64, "active" (N) bool, "m", "seed" (T) int32)."""
    radius, target = check_upsample_args(radius, target)
    rows = check_host_cloud(rows, "smoothing")
    dev = cuda_device(device, "upsample_rows")
    N = rows.shape[0]
    if N >= target:
        print(f"{uid}: upsampling (radius {radius:g}) not needed: {N} rows, at least the {target} asked for")
        return (rows, None) if return_fit else rows
    host = np.ascontiguousarray(rows[:, :3], dtype=np.float32)
    grid = choose_cluster_grid(host, radius)
    with torch.cuda.device(dev):
        cur = torch.from_numpy(host).to(dev)
        fit = smooth_points(cur, radius, DEFAULT_MIN_COUNT, grid, want=("normals", "eigvals", "count"))
        plane = ~stayed(fit["count"].cpu().numpy(), fit["eigvals"].cpu().numpy())
        active = torch.from_numpy(plane).to(dev)
        m, total = choose_m(lambda m: upsample_points(cur, fit["normals"], radius, m, active, grid, count_only=True)["total"], N, target, radius)
        if N + total > MAX_POINTS:
            raise ValueError(f"{uid}: upsampling {N} rows at radius {radius:g}, m = {m} gives {N + total} rows, more than 2^22: use a smaller radius")
        got = upsample_points(cur, fit["normals"], radius, m, active, grid, capacity=total)
        xyz, seed = got["xyz"].cpu().numpy(), got["seed"].cpu().numpy()
    out = np.concatenate([rows, rows[seed]], axis=0)
    out[N:, :3] = xyz.astype(rows.dtype)
    print(f"{uid}: upsampling (radius {radius:g}, m {m}) {N} -> {out.shape[0]} rows, {int((~plane).sum())} seeds had no plane")
    if return_fit:
        return out, {"normals": fit["normals"].cpu().numpy(), "active": plane, "m": m, "seed": seed}
    return out
