"""Farthest-point sampling of a point cloud (`--point_sampling fps`): which n of the N rows of a dense cloud to keep.

`farthest_point_sample` is one call into the HIP library (csrc/pc_fps.hpp; C ABI ma_op_pc_fps, whose header comment states the
definition): start at a given row, or at the row farthest from the bounding box's centre, and pick n times the row farthest from
everything picked so far, under the float32 distance key of `pc_normals.knn` and the total order (greater distance, then lower index).
The same input gives the same indices and the same bits on every run and in both forms of the kernel, and a numpy float32 restatement
(tests/pc_fps_ref.py) gives them too.  It needs a CUDA tensor; there is no CPU fallback.  There is no reference counterpart: the
reference keeps `np.random.choice(N, n, replace=False)` rows.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .pc_common import MAX_POINTS, as_host_cloud, check_device_cloud, check_finite, cuda_device, is_int, need_cuda, upload_xyz

MAX_PICKS, ONE_MAX_POINTS = 1 << 16, 1 << 14                        # MA_PC_FPS_MAX_PICKS, _ONE_MAX_POINTS
FORM_AUTO, FORM_ONE, FORM_MANY = 0, 1, 2


def check_fps_args(N: int, n, start, form) -> tuple:
    """The checks on (n, start, form) for a cloud of N rows; returns them as ints, start = -1 for None."""
    if not is_int(n) or not 1 <= int(n) <= MAX_PICKS:
        raise ValueError(f"n must be an integer in 1..2^16, got {n!r}")
    if not int(n) <= N <= MAX_POINTS:
        raise ValueError(f"need n <= N <= 2^22 points, got N = {N} with n = {n}")
    if start is None:
        start = -1
    elif not is_int(start) or not 0 <= int(start) < N:
        raise ValueError(f"start must be None or a row in [0, {N}), got {start!r}")
    if not is_int(form) or int(form) not in (FORM_AUTO, FORM_ONE, FORM_MANY):
        raise ValueError(f"form must be 0 (automatic), 1 (one workgroup) or 2 (many workgroups), got {form!r}")
    if int(form) == FORM_ONE and N > ONE_MAX_POINTS:
        raise ValueError(f"form 1 (one workgroup) holds at most {ONE_MAX_POINTS} points, got N = {N}")
    return int(n), int(start), int(form)


def farthest_point_sample(points: torch.Tensor, n: int, start=None, form: int = 0):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns, finite -> (idx (n) int32, d2 (n) float32): the rows in pick
    order and the squared distance of each to the rows picked before it (d2[0] = inf, d2[1:] non-increasing; every row of points lies
    within sqrt(d2[n - 1]) of a picked one, up to the last pick's own update).  start: the first row, None = the row farthest from the
    bounding box's centre.  form: 0 = the library's choice, 1 = one workgroup (N <= 16 384), 2 = many workgroups; the result does not
    depend on it (ma_op_pc_fps)."""
    check_device_cloud(points)
    N = points.shape[0]
    n, start, form = check_fps_args(N, n, start, form)
    need_cuda(points, "farthest_point_sample")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        nbytes = lib.ma_pc_fps_workspace_bytes(N, n, form)
        if nbytes == 0:
            raise ValueError(f"outside the limits of ma_op_pc_fps: N = {N}, n = {n}, form = {form}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.ma_op_pc_fps(ref.data_ptr(), N, ref.shape[1], n, start, form, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return idx, d2


def check_cloud_for_fps(xyz, n_points: int) -> np.ndarray:
    """The checks of the fps branches that need no device: a floating (N, >= 3) array, n_points <= N <= 2^22, finite xyz."""
    xyz = as_host_cloud(xyz)
    if xyz.shape[0] < n_points:
        raise ValueError(f"farthest-point sampling keeps {n_points} points: the input should have at least as many, got {xyz.shape[0]}")
    if xyz.shape[0] > MAX_POINTS:
        raise ValueError(f"farthest-point sampling takes at most 2^22 points, got {xyz.shape[0]}")
    if not 1 <= n_points <= MAX_PICKS:
        raise ValueError(f"farthest-point sampling keeps at most 2^16 points, got n_points = {n_points}")
    check_finite(xyz)
    return xyz


def fps_rows(xyz, n_points: int, device="cuda") -> np.ndarray:
    """xyz (N, >= 3) host array -> the n_points rows farthest-point sampling keeps, in pick order (int64): the first three columns are
    uploaded as float32 and sampled with the automatic start and form.  Consumes no random numbers."""
    xyz = check_cloud_for_fps(xyz, n_points)
    dev = cuda_device(device, "farthest-point sampling")
    with torch.cuda.device(dev):
        idx, _ = farthest_point_sample(upload_xyz(xyz, dev), n_points)
        return idx.cpu().numpy().astype(np.int64)
