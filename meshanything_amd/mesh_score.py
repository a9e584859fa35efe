"""Best-of-N sampling: score candidate meshes against the cloud they were generated from, and pick the best of each group.

`score_meshes` is one call into the HIP library (csrc/mesh_score.hpp; C ABI ma_op_score_meshes): per candidate the two directed mean
distances cloud -> mesh and mesh -> cloud, the mesh area and the number of valid faces.  `select` is the only arithmetic done in
Python: `0.5 * (cloud_to_mesh + mesh_to_cloud)` and the argmin of each group.  There is no reference counterpart: the reference draws
one mesh per cloud.

`normal_agreement` is the second call (csrc/mesh_normals.hpp; C ABI ma_op_mesh_normals): how well the face normals
of every candidate agree with the normals of the cloud -- per candidate the normal consistency NC and the share of area wound against
the cloud, per face the signed agreement.  `select` adds `normal_weight * (1 - NC)` to the total on request, and `orient_faces` winds
every face the way the cloud says.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

# The detokenizer emits coordinates in [-0.5, 0.5] (undiscretize, meshanything.py:214-223) and Dataset normalises the cloud to a
# half-extent of 0.9995 (main.py:45-58), so a mesh that fits its cloud is the cloud's frame divided by 2.  Derived from the code,
# not checked against released weights: hence an argument.
DEFAULT_MESH_SCALE = 2.0


def _check_shapes(coords, cloud, n_per_cloud: int, mesh_scale: float):
    if coords.dim() != 4 or tuple(coords.shape[2:]) != (3, 3) or coords.shape[0] < 1 or coords.shape[1] < 1:
        raise ValueError(f"coords must be (B, F, 3, 3) with B, F >= 1, got {tuple(coords.shape)}")
    if cloud.dim() != 3 or cloud.shape[2] not in (3, 6) or cloud.shape[1] < 1:
        raise ValueError(f"cloud must be (G, P, 3) or (G, P, 6) with P >= 1, got {tuple(cloud.shape)}")
    if cloud.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"cloud must be float16 or float32, got {cloud.dtype}")
    n = int(n_per_cloud)
    if n < 1 or coords.shape[0] != cloud.shape[0] * n:
        raise ValueError(f"{coords.shape[0]} candidates do not make {cloud.shape[0]} groups of n_per_cloud = {n_per_cloud}")
    s = float(mesh_scale)
    if not (s > 0 and s != float("inf")):
        raise ValueError(f"mesh_scale must be finite and > 0, got {mesh_scale}")
    return n, s


def score_meshes(coords: torch.Tensor, cloud: torch.Tensor, n_per_cloud: int = 1, mesh_scale: float = DEFAULT_MESH_SCALE,
                 return_terms: bool = False):
    """coords (B, F, 3, 3) (the detokenizer's output, NaN rows = invalid faces), cloud (B / n_per_cloud, P, 3 | 6) float16 or float32
    (a pc_normal tensor as it is) -> scores (B, 4) fp32 on coords' device: cloud-to-mesh mean distance, mesh-to-cloud mean distance,
    area, number of valid faces (ma_op_score_meshes).  Candidate b belongs to cloud b // n_per_cloud.  return_terms: also the
    kernel's per-point and per-face terms (pt_dist (B, P), face_nn (B, F), face_area (B, F), -1 = invalid), views of the workspace."""
    n, s = _check_shapes(coords, cloud, n_per_cloud, mesh_scale)
    if coords.device.type != "cuda":
        raise ValueError("score_meshes runs on the GPU: coords must be a CUDA tensor (there is no CPU fallback)")
    lib = _lib.load()
    dev = coords.device
    with torch.cuda.device(dev):
        c = coords.to(torch.float32).contiguous()
        pc = cloud.to(dev).to(torch.float32).contiguous()       # fp32 input on the device: no copy
        if not bool(torch.isfinite(pc[..., :3]).all()):
            raise ValueError("the cloud has non-finite coordinates")
        B, F, P, ld = c.shape[0], c.shape[1], pc.shape[1], pc.shape[2]
        nbytes = lib.ma_score_meshes_workspace_bytes(B, F, P)
        if nbytes == 0:
            raise ValueError(f"outside the limits of ma_op_score_meshes: B = {B}, F = {F}, P = {P} (F, P <= 2^20)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        scores = torch.empty((B, 4), dtype=torch.float32, device=dev)
        _lib.check(lib.ma_op_score_meshes(c.data_ptr(), B, F, pc.data_ptr(), ld, P, n, s, scores.data_ptr(), ws.data_ptr(), nbytes,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if not return_terms:
        return scores
    a256 = lambda b: (b + 255) & ~255                           # noqa: E731  (the layout include/meshanything_amd.h documents)
    o1 = a256(B * P * 4)
    o2 = o1 + a256(B * F * 4)
    terms = {"pt_dist": ws[:B * P * 4].view(torch.float32).view(B, P), "face_nn": ws[o1:o1 + B * F * 4].view(torch.float32).view(B, F),
             "face_area": ws[o2:o2 + B * F * 4].view(torch.float32).view(B, F)}
    return scores, terms


def normal_agreement(coords: torch.Tensor, cloud: torch.Tensor, n_per_cloud: int = 1, mesh_scale: float = DEFAULT_MESH_SCALE,
                     return_terms: bool = False):
    """coords (B, F, 3, 3) as for score_meshes, cloud (B / n_per_cloud, P, 6) float16 or float32 with the normals in columns 3..5, used as
    given -> (nscores (B, 4), face_agree (B, F)) fp32 on coords' device (ma_op_mesh_normals).  nscores: the normal consistency NC in
    [0, 1] (area-weighted mean of |face normal . normal of the nearest cloud point| over 7 points per face), the share of area whose
    face is wound against the cloud, the area, the number of valid faces.  face_agree: the signed agreement a_f of every face, 0 for
    an invalid or zero-area one.  return_terms: also views of the workspace: face_abs (B, F), face_area (B, F) (-1 = invalid) and
    nn_idx (B, F, 7) int32 (-1 = invalid)."""
    n, s = _check_shapes(coords, cloud, n_per_cloud, mesh_scale)
    if cloud.shape[2] != 6:
        raise ValueError(f"normal_agreement needs the cloud's normals: cloud must be (G, P, 6), got {tuple(cloud.shape)}")
    if cloud.device.type == "cpu" and not bool(torch.isfinite(cloud).all()):       # a host cloud: refused before any device call
        raise ValueError("the cloud has non-finite coordinates or normals")
    if coords.device.type != "cuda":
        raise ValueError("normal_agreement runs on the GPU: coords must be a CUDA tensor (there is no CPU fallback)")
    lib = _lib.load()
    dev = coords.device
    with torch.cuda.device(dev):
        c = coords.to(torch.float32).contiguous()
        pc = cloud.to(dev).to(torch.float32).contiguous()       # fp32 input on the device: no copy
        if not bool(torch.isfinite(pc).all()):
            raise ValueError("the cloud has non-finite coordinates or normals")
        B, F, P, ld = c.shape[0], c.shape[1], pc.shape[1], pc.shape[2]
        nbytes = lib.ma_mesh_normals_workspace_bytes(B, F)
        if nbytes == 0 or P > (1 << 20):
            raise ValueError(f"outside the limits of ma_op_mesh_normals: B = {B}, F = {F}, P = {P} (F, P <= 2^20)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nscores = torch.empty((B, 4), dtype=torch.float32, device=dev)
        face_agree = torch.empty((B, F), dtype=torch.float32, device=dev)
        _lib.check(lib.ma_op_mesh_normals(c.data_ptr(), B, F, pc.data_ptr(), ld, P, n, s, face_agree.data_ptr(), nscores.data_ptr(), ws.data_ptr(),
                                          nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if not return_terms:
        return nscores, face_agree
    a256 = lambda b: (b + 255) & ~255                           # noqa: E731  (the layout include/meshanything_amd.h documents)
    o1 = a256(B * F * 4)
    o2 = 2 * o1
    terms = {"face_abs": ws[:B * F * 4].view(torch.float32).view(B, F), "face_area": ws[o1:o1 + B * F * 4].view(torch.float32).view(B, F),
             "nn_idx": ws[o2:o2 + B * F * 28].view(torch.int32).view(B, F, 7)}
    return nscores, face_agree, terms


def orient_faces(coords: torch.Tensor, face_agree: torch.Tensor) -> torch.Tensor:
    """A copy of coords (..., F, 3, 3) with vertices 1 and 2 swapped wherever face_agree (..., F) < 0: every face then faces the way
    the cloud's normals do.  Faces with a_f >= 0 (a_f == 0: nothing to go by) and NaN rows are unchanged.  torch ops, any device."""
    c, a = torch.as_tensor(coords), torch.as_tensor(face_agree)
    if c.dim() < 3 or tuple(c.shape[-2:]) != (3, 3) or tuple(a.shape) != tuple(c.shape[:-2]):
        raise ValueError(f"coords must be (..., F, 3, 3) and face_agree (..., F), got {tuple(c.shape)} and {tuple(a.shape)}")
    flip = (a.to(c.device) < 0)[..., None, None]
    return torch.where(flip, c[..., [0, 2, 1], :], c)


def select(scores, n_per_cloud: int, normal_scores=None, normal_weight: float = 0.0):
    """scores (G * n_per_cloud, 4) -> (chosen (G,) int64, total (G, n_per_cloud)): total = 0.5 * (scores[:, 0] + scores[:, 1]), chosen =
    its argmin per group.  The lowest index wins ties; +inf (no valid face, no area) loses to every finite total, and a group that is
    all +inf gives index 0.  normal_weight w > 0 with normal_scores (G * n_per_cloud, 4) of normal_agreement: total += w * (1 - NC);
    the scale of w is the caller's (distances are in cloud units, 1 - NC lies in [0, 1])."""
    s = torch.as_tensor(scores)
    n = int(n_per_cloud)
    if s.dim() != 2 or s.shape[1] != 4 or n < 1 or s.shape[0] % n or s.shape[0] < 1:
        raise ValueError(f"scores must be (G * n_per_cloud, 4) with n_per_cloud = {n_per_cloud}, got {tuple(s.shape)}")
    w = float(normal_weight)
    if not (0.0 <= w < float("inf")):
        raise ValueError(f"normal_weight must be finite and >= 0, got {normal_weight}")
    total = 0.5 * (s[:, 0] + s[:, 1])
    if w > 0:
        if normal_scores is None:
            raise ValueError("normal_weight > 0 needs normal_scores (mesh_score.normal_agreement)")
        ns = torch.as_tensor(normal_scores).to(s.device)
        if tuple(ns.shape) != tuple(s.shape):
            raise ValueError(f"normal_scores must be {tuple(s.shape)} like scores, got {tuple(ns.shape)}")
        total = total + w * (1.0 - ns[:, 0])
    total = total.reshape(-1, n)
    key = torch.nan_to_num(total, nan=float("inf"), posinf=float("inf"), neginf=float("-inf"))   # (the kernel emits no NaN; one would rank last)
    best = key.min(dim=1, keepdim=True).values
    idx = torch.arange(n, device=total.device).expand_as(total)
    chosen = torch.where(key == best, idx, torch.full_like(idx, n)).min(dim=1).values        # the first index that attains the minimum
    return chosen.to(torch.int64), total
