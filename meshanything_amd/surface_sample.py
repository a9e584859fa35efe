"""Surface sampling of mesh inputs on the MI355X: the opt-in device form of `mesh_input.mesh_to_pc_normal` (mesh_to_pc.py:42-57,
`mesh.sample(n, return_index=True)` + `face_normals[face_idx]`), used by `mesh_to_pc_normal(..., device=...)`,
`watertight.process_mesh_to_pc(..., device=...)`, `Dataset('mesh', ..., sample_device=...)` and `main.py --gpu_sampling`.

The draws are the host path's: `np.random.random(count)` for the faces, then `np.random.random((count, 2))` for the barycentric pairs,
from the global numpy RNG, taken only after the total area has been read back and found > 0 (else the host's ValueError, with the RNG
untouched).  The kernels (csrc/surface_sample.hpp; C ABI ma_op_surface_cdf / ma_op_sample_surface / ma_op_mc_vertices_to_frame) repeat
the host's float64 arithmetic operation for operation, so for the same draws the (count, 6) float16 cloud is the host's bit for bit.
The one exception is the cumulative sum of the face areas, a parallel scan instead of np.cumsum's sequential one: a draw that lands
within that rounding of a face boundary may pick the neighbouring face.

With `--mc` the marching-cubes output stays on the device: its vertices are mapped to the input's frame there (the float64 arithmetic
of watertight.export_to_watertight, done in a kernel so that no scalar division is rewritten as a multiplication) and sampled.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np

from . import _lib
from .watertight import check_mesh

Mesh = Tuple[np.ndarray, np.ndarray]          # vertices (V, 3) float64, faces (F, 3) int64


def cuda_device(device):
    """torch.device for `device` ("cuda", "cuda:1", an int or a torch.device); ValueError unless it names a CUDA device."""
    import torch
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"surface sampling runs on a CUDA device, got {device!r} (device=None samples on the host)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _count(sample_num) -> int:
    n = int(sample_num)
    if n < 1 or n >= 2 ** 31:
        raise ValueError(f"sample_num must be in [1, 2^31), got {sample_num}")
    return n


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def surface_cdf(verts, faces):
    """ma_op_surface_cdf on device tensors verts (V, 3) float64 and faces (F, 3) int32: (normals (F, 3) float64, cum (F,) float64), the
    unit face normals and the cumulative areas (cum[-1] = the total)."""
    import torch
    lib = _lib.load()
    nf = faces.shape[0]
    normals = torch.empty((nf, 3), dtype=torch.float64, device=verts.device)
    cum = torch.empty(nf, dtype=torch.float64, device=verts.device)
    nbytes = lib.ma_surface_sample_workspace_bytes(nf)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=verts.device)
    _lib.check(lib.ma_op_surface_cdf(verts.data_ptr(), verts.shape[0], faces.data_ptr(), nf, normals.data_ptr(), cum.data_ptr(), ws.data_ptr(),
                                     nbytes, _stream()))
    return normals, cum


def sample_draws(verts, faces, normals, cum, draws, count: int, return_index: bool = False):
    """ma_op_sample_surface: draws = a float64 device tensor of 3 * count values, u (count) followed by uv (count, 2).  Returns the
    (count, 6) float16 device tensor, and with return_index the (count,) int64 face indices."""
    import torch
    lib = _lib.load()
    out = torch.empty((count, 6), dtype=torch.float16, device=verts.device)
    idx = torch.empty(count, dtype=torch.int64, device=verts.device) if return_index else None
    _lib.check(lib.ma_op_sample_surface(verts.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0], normals.data_ptr(), cum.data_ptr(),
                                        draws.data_ptr(), draws.data_ptr() + 8 * count, count, out.data_ptr(),
                                        idx.data_ptr() if idx is not None else None, _stream()))
    return (out, idx) if return_index else out


def _sample_device_mesh(verts, faces, count: int) -> np.ndarray:
    """The cloud of a mesh already on the device: cdf, total read back (the host's no-area error before any draw), draws, sample."""
    import torch
    normals, cum = surface_cdf(verts, faces)
    total = float(cum[-1].item())
    if not total > 0:
        raise ValueError("the mesh has no surface area")
    draws = np.empty(3 * count)
    draws[:count] = np.random.random(count)                    # sample_surface's order: faces, then the barycentric pairs
    draws[count:] = np.random.random((count, 2)).reshape(-1)
    d = torch.from_numpy(draws).to(verts.device)
    return sample_draws(verts, faces, normals, cum, d, count).cpu().numpy()


def mesh_to_pc_normal(vertices, faces, sample_num: int = 4096, device="cuda") -> np.ndarray:
    """mesh_input.mesh_to_pc_normal on `device`: (sample_num, 6) float16, the host function's output for the same RNG state, and the
    RNG left in the same state.  The mesh is checked (watertight.check_mesh) before anything touches the device."""
    v, f = check_mesh(vertices, faces, need_extent=False)
    count = _count(sample_num)
    import torch
    dev = cuda_device(device)
    with torch.cuda.device(dev):
        dv = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        df = torch.from_numpy(f.astype(np.int32)).to(dev)
        return _sample_device_mesh(dv, df, count)


def watertight_pc_normal(index_verts, tris, size: int, to_orig_center, to_orig_scale, sample_num: int = 4096) -> Tuple[np.ndarray, Mesh]:
    """The sampled cloud of a marching-cubes output that is still on the device (index_verts (V, 3) float32 in index space, tris (F, 3)
    int32, as watertight's level-set step leaves them), and the host mesh export_to_watertight returns for it: (cloud, (vertices float64
    (V, 3) in the input's frame, faces int64 (F, 3)))."""
    import torch
    count = _count(sample_num)
    lib = _lib.load()
    dev = index_verts.device
    center = np.ascontiguousarray(to_orig_center, dtype=np.float64)
    verts = torch.empty((index_verts.shape[0], 3), dtype=torch.float64, device=dev)
    _lib.check(lib.ma_op_mc_vertices_to_frame(index_verts.data_ptr(), index_verts.shape[0], int(size), float(to_orig_scale), center.ctypes.data,
                                              verts.data_ptr(), _stream()))
    pc = _sample_device_mesh(verts, tris, count)
    return pc, (verts.cpu().numpy(), tris.cpu().numpy().astype(np.int64))
