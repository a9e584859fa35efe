"""Fit a generated mesh to the cloud it was generated from (`main.py --fit_iters`).

The detokenizer puts every vertex on a 128-step lattice, up to half a step per axis off the surface the cloud samples far more finely.
`fit_mesh` moves the MERGED vertices (`mesh_export.faces_from_coords`) by a few damped Gauss-Newton steps of the point-to-plane fit:
per iteration every cloud point is paired with the nearest admissible face within `dist` on the GPU, the per-face sums of the normal
equations come back as exact integers (`fit_pairs`, one call into the HIP library: csrc/mesh_fit.hpp, C ABI ma_op_mesh_fit_pairs), and
the host assembles them per vertex, adds `stiffness` * I and solves in float64 by conjugate gradients over the per-face blocks (numpy
only: the product imports no scipy).  A vertex never leaves the ball of radius `max_move` about the decoder's position, a vertex
without support does not move, and the result is kept only if `mesh_score.score_meshes` says the mesh came closer to the cloud.
There is no reference counterpart and no CPU fallback.

`dist` and `max_move` of `fit_mesh` are in LATTICE STEPS (1 step = mesh_scale / 128 in cloud units), `dist` of `fit_pairs` in cloud
units, as in the C ABI.  The defaults follow from the lattice (a vertex is at most sqrt(3) / 2 steps off, two steps allow for an
error of the decoder's on top; four steps reach the points of a face whose three vertices are that far off), not from measurements
on released weights, which are not available offline.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .mesh_score import DEFAULT_MESH_SCALE

LATTICE = 128                         # steps of the detokenizer's lattice across the mesh box
FLAT = 2.0 ** -20                     # inradius at or below which a face has no interior (mesh_score's and wt::tri_dist's rule)
MAX_FACES, MAX_POINTS, NSUM = 4096, 1 << 22, 48       # include/meshanything_amd.h: MA_MESH_FIT_*
MAX_ITERS, MAX_DIST_STEPS = 32, 64
DEFAULTS = {"fit_dist": 4.0, "fit_max_move": 2.0, "fit_stiffness": 1.0, "fit_normal_cos": 0.0}
STOP_MOVE = 2.0 ** -20                # an iteration that moves no vertex further ends the fit
SCORE_MAX_POINTS = 1 << 20            # mesh_score.score_meshes' limit: the guard scores a larger cloud on every n-th row
_KL = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def check_fit_args(fit_iters, fit_dist=None, fit_max_move=None, fit_stiffness=None, fit_normal_cos=None):
    """The five arguments as (iters, dist, max_move, stiffness, normal_cos), None replaced by the default; ValueError, worded as
    main.py's argument errors, for anything out of range or given without fit_iters > 0."""
    given = {"fit_dist": fit_dist, "fit_max_move": fit_max_move, "fit_stiffness": fit_stiffness, "fit_normal_cos": fit_normal_cos}
    if isinstance(fit_iters, bool) or int(fit_iters) != fit_iters or not 0 <= fit_iters <= MAX_ITERS:
        raise ValueError(f"fit_iters must be 0 (off) or in 1..{MAX_ITERS}")
    named = [k for k, v in given.items() if v is not None]
    if fit_iters == 0 and named:
        raise ValueError(f"{', '.join(named)} need{'s' if len(named) == 1 else ''} fit_iters > 0")
    v = {k: float(DEFAULTS[k] if x is None else x) for k, x in given.items()}
    if not (0.0 < v["fit_dist"] <= MAX_DIST_STEPS):
        raise ValueError(f"fit_dist must be finite, > 0 and at most {MAX_DIST_STEPS} lattice steps")
    if not (0.0 < v["fit_max_move"] <= v["fit_dist"]):
        raise ValueError("fit_max_move must be finite, > 0 and at most fit_dist")
    if not (0.0 < v["fit_stiffness"] < math.inf):
        raise ValueError("fit_stiffness must be finite and > 0")
    if not (0.0 <= v["fit_normal_cos"] < 1.0):
        raise ValueError("fit_normal_cos must be in [0, 1) (0 = off)")
    return int(fit_iters), v["fit_dist"], v["fit_max_move"], v["fit_stiffness"], v["fit_normal_cos"]


def _tensor(x):
    return x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def check_fit_inputs(verts, faces, cloud, mesh_scale=DEFAULT_MESH_SCALE):
    """Shapes, limits and contents of a mesh and its cloud, on whatever device they are: -> (verts, faces, cloud as tensors, scale)."""
    v, f, c = _tensor(verts), _tensor(faces), _tensor(cloud)
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1 or not v.dtype.is_floating_point:
        raise ValueError(f"verts must be a floating-point (V, 3) with V >= 1, got {tuple(v.shape)} {v.dtype}")
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"faces must be an int32 or int64 (M, 3) with M >= 1, got {tuple(f.shape)} {f.dtype}")
    if c.dim() != 2 or c.shape[1] != 6 or c.shape[0] < 1:
        raise ValueError(f"the fit needs the cloud's normals: cloud must be (P, 6) with P >= 1, got {tuple(c.shape)}")
    if c.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"cloud must be float16 or float32, got {c.dtype}")
    V, M, P = v.shape[0], f.shape[0], c.shape[0]
    if M > MAX_FACES or V > 3 * M or P > MAX_POINTS:
        raise ValueError(f"outside the limits of ma_op_mesh_fit_pairs: V = {V}, M = {M}, P = {P} (M <= {MAX_FACES}, V <= 3 M, P <= 2^22)")
    s = float(mesh_scale)
    if not (0 < s < math.inf):
        raise ValueError(f"mesh_scale must be finite and > 0, got {mesh_scale}")
    if not bool(torch.isfinite(v).all()):
        raise ValueError("verts has non-finite coordinates")
    if not bool(torch.isfinite(c).all()):
        raise ValueError("the cloud has non-finite coordinates or normals")
    if int(f.min()) < 0 or int(f.max()) >= V:
        raise ValueError(f"faces must index the {V} vertices: found {int(f.min())} .. {int(f.max())}")
    return v, f, c, s


def _pairs(x32, faces32, cloud32, dist, normal_cos, workspace=None):
    """The library call on prepared device arrays: x32 (V, 3) fp32 in cloud units, faces32 (M, 3) int32, cloud32 (P, 6) fp32."""
    lib = _lib.load()
    dev = x32.device
    V, M, P = x32.shape[0], faces32.shape[0], cloud32.shape[0]
    nbytes = lib.ma_mesh_fit_workspace_bytes(V, M, P)
    if nbytes == 0:
        raise ValueError(f"outside the limits of ma_op_mesh_fit_pairs: V = {V}, M = {M}, P = {P}")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if workspace is None else workspace
        if ws.device != dev or ws.dtype != torch.uint8 or ws.numel() < nbytes or not ws.is_contiguous():
            raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
        face = torch.empty(P, dtype=torch.int32, device=dev)
        w = torch.empty((P, 3), dtype=torch.float32, device=dev)
        sums = torch.empty((M, NSUM), dtype=torch.int64, device=dev)
        _lib.check(lib.ma_op_mesh_fit_pairs(x32.data_ptr(), V, faces32.data_ptr(), M, cloud32.data_ptr(), 6, P, float(dist), float(normal_cos), FLAT,
                                            face.data_ptr(), w.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    o1 = (P * 4 + 255) & ~255                                    # the layout include/meshanything_amd.h documents
    return {"face": face, "weights": w, "sums": sums, "s": ws[:P * 4].view(torch.float32), "r2": ws[o1:o1 + P * 4].view(torch.float32)}


def fit_pairs(verts, faces, cloud, dist, normal_cos=0.0, mesh_scale=DEFAULT_MESH_SCALE, workspace=None):
    """One pairing and its sums (ma_op_mesh_fit_pairs).  verts (V, 3) CUDA float tensor in MESH units (multiplied by mesh_scale in fp32
    on the way in), faces (M, 3) int, cloud (P, 6) float16 or float32, normals in columns 3..5; dist in CLOUD units, 0 < dist <= 1.
    -> dict of tensors on verts' device: face (P) int32, -1 = unpaired; weights (P, 3); s (P) = normal . (p - c); r2 (P) = |p - c|^2
    (s and r2 are views of the workspace); sums (M, 48) int64 in the header's layout.  workspace: a uint8 tensor to reuse."""
    v, f, c, s = check_fit_inputs(verts, faces, cloud, mesh_scale)
    if not (0.0 < float(dist) <= 1.0):
        raise ValueError(f"dist must be finite, > 0 and at most 1 cloud unit, got {dist}")
    if not (0.0 <= float(normal_cos) < 1.0):
        raise ValueError(f"normal_cos must be in [0, 1), got {normal_cos}")
    if v.device.type != "cuda":
        raise ValueError("fit_pairs runs on the GPU: verts must be a CUDA tensor (there is no CPU fallback)")
    dev = v.device
    x32 = (v.to(torch.float32) * torch.tensor(s, dtype=torch.float32, device=dev)).contiguous()
    return _pairs(x32, f.to(dev).to(torch.int32).contiguous(), c.to(dev).to(torch.float32).contiguous(), dist, normal_cos, workspace)


def normal_equations(sums, faces):
    """sums (M, 48) int64 -> per face the 9 x 9 block A (M, 9, 9) and right-hand side g (M, 9) of the point-to-plane normal equations,
    float64, rows ordered vertex-major (3 k + a); and the counts, sum s^2 and sum |r|^2 (M,) each."""
    q = np.asarray(sums, np.int64)
    fx = q[:, 1:].astype(np.float64) / 4294967296.0
    g = fx[:, 2:11].copy()
    H = fx[:, 11:].reshape(-1, 6, 6)
    A = np.zeros((q.shape[0], 9, 9))
    for i, (k, l) in enumerate(_KL):
        for j, (a, c) in enumerate(_KL):
            for kk, ll in {(k, l), (l, k)}:
                for aa, cc in {(a, c), (c, a)}:
                    A[:, 3 * kk + aa, 3 * ll + cc] = H[:, i, j]
    return A, g, q[:, 0], fx[:, 0], fx[:, 1]


def solve_step(A, g, faces, V, stiffness, rtol=1e-13):
    """(sum_f P_f^T A_f P_f + stiffness * I) delta = sum_f P_f^T g_f for delta (V, 3), float64, by conjugate gradients with the
    vertices' own 3 x 3 blocks as preconditioner; the matrix is never formed.  It is positive definite (A_f is a sum of squares and
    stiffness > 0); a vertex without support has a zero right-hand side, no coupling, and stays exactly 0."""
    faces = np.asarray(faces, np.int64)
    idx = faces.reshape(-1)

    def scatter(per_face):                                       # (M, 9) -> (V, 3)
        out = np.zeros((V, 3))
        np.add.at(out, idx, per_face.reshape(-1, 3))
        return out

    def matvec(x):
        return stiffness * x + scatter(np.einsum("fij,fj->fi", A, x[faces].reshape(-1, 9)))

    b = scatter(g)
    diag = np.zeros((V, 3, 3))
    np.add.at(diag, idx, np.stack([A[:, 3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(3)], 1).reshape(-1, 3, 3))
    pre = np.linalg.inv(diag + stiffness * np.eye(3))
    x = np.zeros((V, 3))
    r = b.copy()
    bnorm = math.sqrt(float((b * b).sum()))
    if bnorm == 0.0:
        return x
    z = np.einsum("vij,vj->vi", pre, r)
    p = z.copy()
    rz = float((r * z).sum())
    for _ in range(max(64, 6 * V)):
        Ap = matvec(p)
        alpha = rz / float((p * Ap).sum())
        x += alpha * p
        r -= alpha * Ap
        if math.sqrt(float((r * r).sum())) <= rtol * bnorm:
            break
        z = np.einsum("vij,vj->vi", pre, r)
        rz_new = float((r * z).sum())
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


def clamp_moves(x, x0, max_move):
    """x with every row's displacement from x0 scaled back to length max_move where it is longer."""
    d = x - x0
    n = np.sqrt((d * d).sum(1))
    k = np.where(n > max_move, max_move / np.where(n > 0, n, 1.0), 1.0)
    return x0 + d * k[:, None]


def _total(verts32, faces_t, cloud_t, scale):
    from .mesh_score import score_meshes
    stride = -(-cloud_t.shape[0] // SCORE_MAX_POINTS)
    sc = score_meshes(verts32[faces_t.long()][None], cloud_t[::stride][None], 1, scale)[0].tolist()
    return (sc[0], sc[1])


def fit_mesh(verts, faces, cloud, iters, dist=None, max_move=None, stiffness=None, normal_cos=None, mesh_scale=DEFAULT_MESH_SCALE):
    """verts (V, 3) float32 and faces (M, 3) int as `faces_from_coords` returns them (numpy, or CUDA tensors), cloud (P, 6) float16 or
    float32 with unit normals in columns 3..5 (numpy or a tensor; P up to 2^22: a caller may fit against more rows than the encoder
    saw) -> (verts', report).  iters in 1..32; dist (default 4) and max_move (default 2) in lattice steps, stiffness (default 1) in
    points, normal_cos (default 0 = off) in [0, 1).  verts' is of verts' kind and float32; when the fit is not kept it IS `verts`.
    report: {"iterations": [{"paired": share of the P points, "rms": of s over the pairs, "move": the largest step of a vertex}, ...],
    "points": P, "rms_after", "paired_after": the same after the last step, "max_move": the largest total displacement, in cloud units,
    "score_before", "score_after": (cloud -> mesh, mesh -> cloud) of mesh_score.score_meshes, "kept": whether their mean fell}."""
    iters, dist, max_move, stiffness, normal_cos = check_fit_args(iters, dist, max_move, stiffness, normal_cos)
    if iters == 0:
        raise ValueError("fit_iters must be in 1..32 to fit")
    v, f, c, scale = check_fit_inputs(verts, faces, cloud, mesh_scale)
    step = scale / LATTICE
    dist_c, move_c = dist * step, max_move * step
    if dist_c > 1.0:
        raise ValueError(f"fit_dist = {dist} steps is {dist_c} cloud units at mesh_scale = {scale}: at most 1")
    if not torch.cuda.is_available():
        raise RuntimeError("fit_mesh runs on the GPU (there is no CPU fallback)")
    dev = v.device if v.device.type == "cuda" else (c.device if c.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device()))
    faces_np = f.cpu().numpy().astype(np.int64)
    x0 = v.detach().cpu().numpy().astype(np.float64) * scale
    V, P = x0.shape[0], c.shape[0]
    with torch.cuda.device(dev):
        f32 = f.to(dev).to(torch.int32).contiguous()
        c32 = c.to(dev).to(torch.float32).contiguous()
        ws = torch.empty(_lib.load().ma_mesh_fit_workspace_bytes(V, f32.shape[0], P), dtype=torch.uint8, device=dev)

        def pairs(x):
            A, g, n, ss, _ = normal_equations(_pairs(torch.from_numpy(x.astype(np.float32)).to(dev), f32, c32, dist_c, normal_cos, ws)["sums"].cpu().numpy(),
                                              faces_np)
            n = int(n.sum())
            return A, g, n / P, math.sqrt(float(ss.sum()) / n) if n else 0.0

        x, its = x0.copy(), []
        for _ in range(iters):
            A, g, share, rms = pairs(x)
            x_new = clamp_moves(x + solve_step(A, g, faces_np, V, stiffness), x0, move_c) if share > 0 else x
            d = x_new - x
            move = math.sqrt(float((d * d).sum(1).max()))
            its.append({"paired": share, "rms": rms, "move": move})
            x = x_new
            if move <= STOP_MOVE:
                break
        moved = x - x0
        report = {"iterations": its, "points": P, "rms_after": its[-1]["rms"], "paired_after": its[-1]["paired"],
                  "max_move": math.sqrt(float((moved * moved).sum(1).max())), "kept": False}
        v_in = v.detach().to(dev).to(torch.float32)
        report["score_before"] = report["score_after"] = _total(v_in, f32, c32, scale)
        if report["max_move"] == 0.0:
            return verts, report
        _, _, report["paired_after"], report["rms_after"] = pairs(x)
        out = (x / scale).astype(np.float32)
        report["score_after"] = _total(torch.from_numpy(out).to(dev), f32, c32, scale)
    report["kept"] = bool(0.5 * sum(report["score_after"]) < 0.5 * sum(report["score_before"]))
    if not report["kept"]:
        return verts, report
    return (torch.from_numpy(out).to(v.device) if torch.is_tensor(verts) else out), report


def report_line(uid, report, mesh_scale=DEFAULT_MESH_SCALE) -> str:
    """main.py's line for one mesh."""
    its, step = report["iterations"], float(mesh_scale) / LATTICE
    tb, ta = 0.5 * sum(report["score_before"]), 0.5 * sum(report["score_after"])
    return (f"{uid}: fit {len(its)} iteration{'s' if len(its) != 1 else ''}, {round(its[0]['paired'] * report['points'])} of {report['points']} points paired, "
            f"RMS {its[0]['rms']:.3e} -> {report['rms_after']:.3e}, largest move {report['max_move'] / step:.3f} steps, total {tb:.6f} -> {ta:.6f}, "
            + ("kept" if report["kept"] else "not kept: the decoder's vertices are written"))
