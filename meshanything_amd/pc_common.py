"""What the point-cloud modules (pc_*.py) share: the limits of the HIP library's cloud ops, the argument checks whose wording is the same
in every module, and the scaffolding between a host array and a device cloud.  It imports none of them."""
from __future__ import annotations

import numpy as np
import torch

MAX_POINTS, MAX_QUERIES = 1 << 22, 1 << 20                       # MA_PC_KNN_MAX_POINTS (= _FPS_, _PLANE_), MA_PC_KNN_MAX_QUERIES
MAX_DIM, MAX_CELLS = 128, 1 << 21                                # MA_PC_GRID_MAX_DIM, MA_PC_GRID_MAX_CELLS


def is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def is_real(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def check_int(name: str, v, lo: int, hi: int) -> int:
    if not is_int(v) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def check_want(want, names) -> tuple:
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in names for w in want):
        raise ValueError(f"want must name at least one of {names}, got {want!r}")
    return want


def need_cuda(t, what: str):
    if t.device.type != "cuda":
        raise ValueError(f"{what} runs on the GPU: points must be a CUDA tensor (there is no CPU fallback)")


def cuda_device(device, what: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{what} runs on the GPU: device must be a CUDA device (there is no CPU fallback)")
    return dev


def check_device_cloud(points, lo=None, lo_name=None):
    """A (N, 3 | 6) float32 tensor with lo <= N <= 2^22 (lo None: N is the caller's to check); lo_name: the argument lo is, for the message."""
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] not in (3, 6):
        raise ValueError(f"points must be a (N, 3) or (N, 6) tensor, got {tuple(points.shape) if hasattr(points, 'shape') else type(points).__name__}")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if lo is not None and not lo <= points.shape[0] <= MAX_POINTS:
        raise ValueError(f"need {lo_name or lo} <= N <= 2^22 points, got N = {points.shape[0]}" + (f" with {lo_name} = {lo}" if lo_name else ""))


def as_host_cloud(xyz) -> np.ndarray:
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] < 3 or not np.issubdtype(xyz.dtype, np.floating):
        raise ValueError(f"a point cloud must be a floating (N, >= 3) array, got {xyz.shape} {xyz.dtype}")
    return xyz


def check_finite(xyz):
    if not np.isfinite(xyz[:, :3]).all():
        raise ValueError("the point cloud has non-finite coordinates")


def check_host_cloud(xyz, noun: str, lo: int = 1) -> np.ndarray:
    """The checks on a host cloud that need no device: a floating (N, >= 3) array, lo <= N <= 2^22, finite xyz; returns it as an array."""
    xyz = as_host_cloud(xyz)
    if not lo <= xyz.shape[0] <= MAX_POINTS:
        raise ValueError(f"{noun} needs {lo} <= N <= 2^22 points, got N = {xyz.shape[0]}")
    check_finite(xyz)
    return xyz


def check_grid(grid):
    """grid (origin (3), cell, dims (3)) -> the same as (float32 (3), float32, int32 (3)), within the limits of the library's cell grid."""
    try:
        origin, cell, dims = grid
        origin = np.asarray(origin, dtype=np.float32).reshape(-1)
        dims_in = np.asarray(dims).reshape(-1)
        cell = np.float32(cell)
    except (TypeError, ValueError):
        raise ValueError("grid must be (origin (3), cell, dims (3))") from None
    if origin.shape != (3,) or dims_in.shape != (3,) or not np.issubdtype(dims_in.dtype, np.integer):
        raise ValueError("grid must be (origin (3) floats, cell, dims (3) integers)")
    if not np.isfinite(origin).all() or not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"the grid's origin must be finite and its cell finite and > 0, got {origin.tolist()} and {float(cell)}")
    if (dims_in < 1).any() or (dims_in > MAX_DIM).any() or int(np.prod(dims_in.astype(np.int64))) > MAX_CELLS:
        raise ValueError(f"the grid's dims must each lie in 1..{MAX_DIM} with a product of at most 2^21, got {dims_in.tolist()}")
    return origin, cell, dims_in.astype(np.int32)


def upload_xyz(xyz: np.ndarray, dev) -> torch.Tensor:
    """The first three columns of a host cloud as a contiguous float32 tensor on dev."""
    return torch.from_numpy(np.ascontiguousarray(xyz[:, :3], dtype=np.float32)).to(dev)
