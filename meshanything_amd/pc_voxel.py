"""Voxel thinning of dense input clouds (`--voxel_size`): keep one ROW per occupied voxel of a uniform grid.

A scanner, fused depth maps or photogrammetry leave 10 to 100 million points, far more than the 2^22 rows any other step of the input
side takes, and at a density that follows the sensor; every PCL or Open3D pipeline opens by thinning them.  The rule is
pcl::UniformSampling's, not VoxelGrid's centroid: per voxel of edge `leaf`, counted from the cloud's per-axis minimum, the row nearest
the voxel's centre survives, the lowest row index among equals, so rows stay rows and their normals travel with them.  The survivors are
found on the GPU with a hash table over the voxel keys and no sort (csrc/pc_voxel.hpp; C ABI ma_op_pc_voxel_reset / _insert / _mark, whose
header comment states the rule): the cloud passes through in chunks of at most 2^22 rows, so it never has to be on the device at once,
and the mask equals a numpy float32 restatement byte for byte, whatever the chunking and the table's capacity.  It needs a CUDA device;
there is no CPU fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_common import as_host_cloud, check_finite, check_int, cuda_device, is_real, need_cuda, upload_xyz

MAX_POINTS, MAX_CHUNK, MAX_VOXELS = 1 << 28, 1 << 22, 1 << 22     # MA_PC_VOXEL_MAX_POINTS, _MAX_CHUNK, _MAX_VOXELS
MAX_INDEX = 1 << 21                                               # voxels along an axis: three indices share a 63-bit key


def check_voxel_args(voxel_size) -> float:
    """The check on voxel_size that needs no file: a finite real > 0 that is one as float32 too; returns it as a float."""
    with np.errstate(over="ignore", under="ignore"):
        ok = is_real(voxel_size) and 0.0 < float(voxel_size) < float("inf") and 0.0 < float(np.float32(voxel_size)) < float("inf")
    if not ok:
        raise ValueError(f"voxel_size must be finite and > 0 (as float32 too), got {voxel_size!r}")
    return float(voxel_size)


def _check_capacity(capacity) -> int:
    if not isinstance(capacity, (int, np.integer)) or isinstance(capacity, bool) or not 2 <= int(capacity) <= 2 * MAX_VOXELS or int(capacity) & (int(capacity) - 1):
        raise ValueError(f"capacity must be a power of two in 2..2^23, got {capacity!r}")
    return int(capacity)


def default_capacity(N: int, max_voxels: int = MAX_VOXELS) -> int:
    """The power of two >= 2 * min(N, max_voxels): the table may be half full, and there are no more voxels than rows."""
    return 1 << max(1, (2 * min(int(N), int(max_voxels)) - 1).bit_length())


def check_keep_args(xyz, leaf, chunk_rows=MAX_CHUNK, max_voxels=MAX_VOXELS, capacity=None):
    """The checks of voxel_keep that need no device -> (xyz as an array, origin (3) float32, leaf, capacity)."""
    xyz = as_host_cloud(xyz)
    leaf = check_voxel_args(leaf)
    chunk_rows = check_int("chunk_rows", chunk_rows, 1, MAX_CHUNK)
    max_voxels = check_int("max_voxels", max_voxels, 1, MAX_VOXELS)
    N = xyz.shape[0]
    if not 1 <= N <= MAX_POINTS:
        raise ValueError(f"voxel thinning needs 1 <= N <= 2^28 points, got N = {N}")
    capacity = default_capacity(N, max_voxels) if capacity is None else _check_capacity(capacity)
    check_finite(xyz)
    origin = np.ascontiguousarray(xyz[:, :3].min(axis=0), dtype=np.float32)    # rounding is monotone: the minimum of the float32 values, whatever the file's dtype
    extent = (xyz[:, :3].max(axis=0).astype(np.float32).astype(np.float64) - origin.astype(np.float64)) / float(np.float32(leaf))
    if not (extent < MAX_INDEX - 1).all():
        raise ValueError(f"voxel_size = {leaf:g} is too small for this cloud: {extent.max():.6g} voxels along its longest axis, at most 2^21 - 1 fit: choose a larger one")
    return xyz, origin, leaf, chunk_rows, max_voxels, capacity


def new_table(capacity: int, dev) -> torch.Tensor:
    """An empty table of `capacity` slots on dev (ma_op_pc_voxel_reset)."""
    capacity = _check_capacity(capacity)
    dev = cuda_device(dev, "voxel thinning")
    lib = _lib.load()
    with torch.cuda.device(dev):
        table = torch.empty(lib.ma_pc_voxel_table_bytes(capacity), dtype=torch.uint8, device=dev)
        _lib.check(lib.ma_op_pc_voxel_reset(table.data_ptr(), capacity, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return table


def insert(table: torch.Tensor, capacity: int, points: torch.Tensor, row0: int, origin, leaf: float):
    """points (n, 3 | 6) float32 on the GPU, the rows row0 .. row0 + n - 1 of the cloud, into the table (ma_op_pc_voxel_insert)."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] not in (3, 6) or points.dtype != torch.float32:
        raise ValueError("points must be a (n, 3) or (n, 6) float32 tensor")
    if not 1 <= points.shape[0] <= MAX_CHUNK or not 0 <= int(row0) <= MAX_POINTS - points.shape[0]:
        raise ValueError(f"an insert takes 1..2^22 rows and row0 + n <= 2^28, got n = {points.shape[0]}, row0 = {row0}")
    need_cuda(points, "voxel thinning")
    lib = _lib.load()
    with torch.cuda.device(points.device):
        ref = points.contiguous()
        _lib.check(lib.ma_op_pc_voxel_insert(ref.data_ptr(), ref.shape[0], ref.shape[1], int(row0), (C.c_float * 3)(*np.asarray(origin, np.float32).tolist()),
                                             float(leaf), table.data_ptr(), int(capacity), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def mark(table: torch.Tensor, capacity: int, N: int):
    """-> (keep (N) uint8 on the GPU, {"used", "overflow", "out_of_range", "voxels"}) (ma_op_pc_voxel_mark; waits for the stream)."""
    lib = _lib.load()
    with torch.cuda.device(table.device):
        keep = torch.empty(int(N), dtype=torch.uint8, device=table.device)
        state = (C.c_uint32 * 4)()
        _lib.check(lib.ma_op_pc_voxel_mark(table.data_ptr(), int(capacity), keep.data_ptr(), int(N), state, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return keep, dict(zip(("used", "overflow", "out_of_range", "voxels"), (int(v) for v in state)))


def voxel_keep(xyz, leaf, device="cuda", chunk_rows: int = MAX_CHUNK, max_voxels: int = MAX_VOXELS, capacity=None):
    """xyz (N, >= 3) host array, 1 <= N <= 2^28, finite, only the first three columns are read (uploaded as float32, chunk_rows at a time
    into one table) -> (keep (N) bool, voxels): keep marks the one surviving row of every occupied voxel of edge `leaf` counted from the
    cloud's per-axis float32 minimum, voxels = keep.sum().  capacity: the table's slots, a power of two, by default the one >=
    2 * min(N, max_voxels); the mask does not depend on it, nor on chunk_rows.  More than max_voxels (or capacity / 2) occupied voxels,
    and a leaf below extent / (2^21 - 1), are ValueErrors."""
    xyz, origin, leaf, chunk_rows, max_voxels, capacity = check_keep_args(xyz, leaf, chunk_rows, max_voxels, capacity)
    dev = cuda_device(device, "voxel_keep")
    N = xyz.shape[0]
    with torch.cuda.device(dev):
        table = new_table(capacity, dev)
        for row0 in range(0, N, chunk_rows):
            insert(table, capacity, upload_xyz(xyz[row0:row0 + chunk_rows], dev), row0, origin, leaf)
        keep, state = mark(table, capacity, N)
        if state["out_of_range"]:
            raise ValueError(f"voxel_size = {leaf:g} is too small for this cloud: a voxel index reaches 2^21: choose a larger one")
        if state["overflow"] or state["voxels"] > max_voxels:
            raise ValueError(f"more than {min(max_voxels, capacity // 2)} voxels are occupied at voxel_size = {leaf:g}: choose a larger one")
        keep = keep.cpu().numpy().astype(bool)
    return keep, state["voxels"]


def thin_rows(rows, voxel_size: float, floor: int, uid: str, device="cuda") -> np.ndarray:
    """The rows that survive the thinning, in their order; prints the line of the command line.  Fewer than `floor` is a ValueError."""
    keep, voxels = voxel_keep(rows, voxel_size, device=device)
    print(f"{uid}: voxel grid kept {voxels} of {keep.shape[0]} points (voxel_size {voxel_size:g})")
    if voxels < floor:
        raise ValueError(f"{uid}: only {voxels} of {keep.shape[0]} points survive the voxel grid, fewer than the {floor} the encoder takes")
    return rows[keep]
