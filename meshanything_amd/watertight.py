"""Watertight remeshing of mesh inputs on the MI355X: `--mc` of the reference (mesh_to_pc.py:6-57), under the reference's names.

`export_to_watertight` normalises the mesh into [-0.9, 0.9]^3, computes the distance to it on a 128^3 grid and extracts the level
set |sdf| = 2 / 128 by marching cubes: a closed two-sheet shell one cell either side of the input surface, mapped back to the input's
frame.  `process_mesh_to_pc` then samples 4096 points + face normals of it like any other mesh input (mesh_input.mesh_to_pc_normal);
with `device="cuda"` the marching-cubes output stays on the GPU and is sampled there (surface_sample.py), giving the same clouds.

The reference computes a SIGNED distance with mesh2sdf and runs scikit-image's Lewiner marching cubes on the CPU ("need several
minutes").  Only |sdf| is used there, so this package computes the unsigned distance directly, in a narrow band of two cells around
each triangle (exact wherever it can reach the surface; a zero-area face counts as its edges, within 1/128 of a cell), and runs marching cubes with its own 256-case table: two HIP passes each
(csrc/watertight.hpp; C ABI ma_op_mesh_udf / ma_op_marching_cubes).  There is no CPU path.

Parity: *unpinned*.  mesh2sdf, scikit-image and trimesh are not available to generate fixtures, and two differences are known:
the table matches Lewiner's output except in cells with an ambiguous face or body, where the topology may differ and Lewiner
may add a vertex at the cell centre (vertices on crossing edges agree up to rounding); mesh2sdf's distances are exact within about
one cell of the surface and swept beyond, the band here is exact in every cell that can affect the surface.  The sampled cloud is
statistically equivalent to the reference's, not draw-for-draw equal (mesh_input.py explains why).  What the tests pin instead
(tests/test_watertight_host.py, tests/test_gpu_watertight.py): both kernels against a numpy restatement, a closed and consistently
oriented output, and every output vertex one cell from the input surface.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .mesh_input import mesh_to_pc_normal

Mesh = Tuple[np.ndarray, np.ndarray]          # vertices (V, 3) float64, faces (F, 3) int64


def normalize_vertices(vertices: np.ndarray, scale: float = 0.9):
    """mesh_to_pc.py:6-11: centre on the bounding-box mid-point, longest side -> 2 * scale.  Returns (vertices, center, scale)."""
    bbmin, bbmax = vertices.min(0), vertices.max(0)
    center = (bbmin + bbmax) * 0.5
    scale = 2.0 * scale / (bbmax - bbmin).max()
    vertices = (vertices - center) * scale
    return vertices, center, scale


def check_mesh(vertices, faces, need_extent: bool = True) -> Mesh:
    """The input checks of the GPU path, before anything is launched: ValueError for an empty mesh, a non-finite vertex, a face
    index out of range or (need_extent) a mesh without extent.  Returns (vertices float64 (V, 3), faces int64 (F, 3))."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"expected vertices (V, 3) and faces (F, 3), got {v.shape} and {f.shape}")
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError(f"empty mesh: {v.shape[0]} vertices, {f.shape[0]} faces")
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be integer vertex indices, got {f.dtype}")
    if not np.isfinite(v).all():
        raise ValueError("non-finite vertex coordinates")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError(f"a face refers to vertex {int(f.min()) if f.min() < 0 else int(f.max())}, the mesh has {v.shape[0]}")
    if v.shape[0] >= 2 ** 31 or f.shape[0] > 2 ** 28:
        raise ValueError("meshes with 2^31 or more vertices or more than 2^28 faces are not supported")
    if need_extent and not (v.max(0) - v.min(0)).max() > 0:
        raise ValueError("the mesh has no extent (all vertices coincide)")
    return v, f


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mesh_udf(vertices: np.ndarray, faces: np.ndarray, size: int):
    """Unsigned distance to the mesh on the (size, size, size) grid of points -1 + 2 * (i, j, k) / size (ma_op_mesh_udf): a float32
    CUDA tensor, +inf outside the 2-cell band.  `vertices` are used as float32, already in the grid's frame."""
    import torch
    v, f = check_mesh(vertices, faces)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    dv = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    df = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).to(dev)
    field = torch.empty((size, size, size), dtype=torch.float32, device=dev)
    nbytes = lib.ma_mesh_udf_workspace_bytes(f.shape[0])
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.ma_op_mesh_udf(dv.data_ptr(), v.shape[0], df.data_ptr(), f.shape[0], size, field.data_ptr(), ws.data_ptr(), nbytes, _stream()))
    return field


def extract_level_set(field, level: float, count_only: bool = False):
    """The level set `field == level` of a float32 CUDA tensor (nx, ny, nz) (ma_op_marching_cubes): vertices (V, 3) float32 in index
    space and triangles (F, 3) int32, as numpy arrays; each triangle's normal points toward increasing values.  count_only: (V, F)."""
    if count_only:
        return _level_set(field, level, True)
    verts, tris = _level_set(field, level)
    return verts.cpu().numpy(), tris.cpu().numpy()


def _level_set(field, level: float, count_only: bool = False):
    """extract_level_set, leaving the vertices and triangles on the device (torch tensors)."""
    import torch
    if field.dtype != torch.float32 or field.dim() != 3 or not field.is_cuda:
        raise ValueError("field must be a 3-D float32 CUDA tensor")
    field = field.contiguous()
    lib = _lib.load()
    nx, ny, nz = field.shape
    nbytes = lib.ma_marching_cubes_workspace_bytes(nx, ny, nz)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=field.device)
    counts = (C.c_int64 * 2)()
    _lib.check(lib.ma_op_marching_cubes(field.data_ptr(), nx, ny, nz, float(level), None, 0, None, 0, counts, ws.data_ptr(), nbytes, _stream()))
    nv, nt = int(counts[0]), int(counts[1])
    if count_only:
        return nv, nt
    verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=field.device)
    tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=field.device)
    _lib.check(lib.ma_op_marching_cubes(field.data_ptr(), nx, ny, nz, float(level), verts.data_ptr(), nv, tris.data_ptr(), nt, counts,
                                        ws.data_ptr(), nbytes, _stream()))
    return verts[:nv], tris[:nt]


def _watertight_on_device(vertices, faces, octree_depth: int = 7):
    """export_to_watertight up to the marching cubes: (index-space vertices (V, 3) float32 and triangles (F, 3) int32 as CUDA tensors,
    size, to_orig_center, to_orig_scale)."""
    v, f = check_mesh(vertices, faces)
    size = 2 ** octree_depth
    level = 2 / size
    scaled_vertices, to_orig_center, to_orig_scale = normalize_vertices(v)
    field = mesh_udf(scaled_vertices, f, size)
    mv, mf = _level_set(field, level)
    if mf.shape[0] == 0:
        raise ValueError("marching cubes found no surface")
    return mv, mf, size, to_orig_center, to_orig_scale


def export_to_watertight(vertices, faces, octree_depth: int = 7) -> Mesh:
    """mesh_to_pc.py:13-40 on the GPU: the closed shell |distance| = 2 / 2^octree_depth around the normalised mesh, in the input's
    frame.  Returns (vertices float64 (V, 3), faces int64 (F, 3)); face winding gives outward normals on the outer sheet."""
    mv, mf, size, to_orig_center, to_orig_scale = _watertight_on_device(vertices, faces, octree_depth)
    mv, mf = mv.cpu().numpy(), mf.cpu().numpy()
    mv = mv.astype(np.float64) / size * 2 - 1                     # -1 to 1
    mv = mv / to_orig_scale + to_orig_center
    return mv, mf.astype(np.int64)


def process_mesh_to_pc(mesh_list: Sequence[Mesh], marching_cubes: bool = False, sample_num: int = 4096,
                       device=None) -> Tuple[List[np.ndarray], List[Mesh]]:
    """mesh_to_pc.py:42-57: for each (vertices, faces) mesh, optionally made watertight first, `sample_num` surface points + the normal
    of the face under each, (sample_num, 6) float16, drawn from the global numpy RNG.  Returns (pc_normal_list, mesh_list).

    device (e.g. "cuda"): sample on that GPU (surface_sample.py), with the same draws and the same clouds; with marching_cubes the
    remeshed surface stays on the device between the marching cubes and the sampling.  The returned meshes are the same host arrays."""
    if marching_cubes:
        mesh_list = [check_mesh(v, f) for v, f in mesh_list]      # every input checked before the first launch
    if device is not None:
        from . import surface_sample
        dev = surface_sample.cuda_device(device)
    pc_normal_list, return_mesh_list = [], []
    for vertices, faces in mesh_list:
        if marching_cubes and device is not None:
            import torch
            with torch.cuda.device(dev):
                mv, mf, size, center, scale = _watertight_on_device(vertices, faces)
                print("MC over!")
                pc, (vertices, faces) = surface_sample.watertight_pc_normal(mv, mf, size, center, scale, sample_num)
            return_mesh_list.append((vertices, faces))
            pc_normal_list.append(pc)
            print("process mesh success")
            continue
        if marching_cubes:
            vertices, faces = export_to_watertight(vertices, faces)
            print("MC over!")
        return_mesh_list.append((vertices, faces))
        pc_normal_list.append(mesh_to_pc_normal(vertices, faces, sample_num, device=device))
        print("process mesh success")
    return pc_normal_list, return_mesh_list
