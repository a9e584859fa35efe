"""Numpy restatement of ma_op_pc_register_step (include/meshanything_amd.h, csrc/pc_register.hpp) and of pc_register.register_rows, shared
by the host and the GPU tests: the float32 transform and key with every rounding explicit, brute-force pairs over ALL target rows, the 32
float64 sums (exactly rounded, math.fsum, with the sum of |term| per slot beside them), the ICP loop over them, and the test solid."""
import math
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32, F64 = np.float32, np.float64


def header_constants():
    """The constants include/meshanything_amd.h exports for the summation order."""
    text = open(os.path.join(REPO, "include", "meshanything_amd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+MA_PC_REGISTER_(\w+)\s+(\d+)", text)}


_C = header_constants()
SUMS, THREADS, ROWS_PER_THREAD = _C["SUMS"], _C["THREADS"], _C["ROWS_PER_THREAD"]
GROUP_ROWS = THREADS * ROWS_PER_THREAD                             # the source rows of one moments workgroup


def depth(M: int) -> int:
    """The longest chain of additions behind one slot: a thread's rows, the tree over the lanes, the workgroups' partials in turn."""
    return ROWS_PER_THREAD + int(math.log2(THREADS)) + -(-M // GROUP_ROWS)


def transform_ref(src, pose):
    """src (M, >= 3), pose 12 float32 -> p' (M, 3) float32: fl32(fl32(fl32(fl32(R_a0 x) + fl32(R_a1 y)) + fl32(R_a2 z)) + t_a)"""
    src, pose = np.asarray(src, F32), np.asarray(pose, F32)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    out = np.empty((src.shape[0], 3), F32)
    with np.errstate(all="ignore"):
        for a in range(3):
            r0, r1, r2, t = pose[3 * a], pose[3 * a + 1], pose[3 * a + 2], pose[9 + a]
            s = (r0 * x).astype(F32) + (r1 * y).astype(F32)
            s = s.astype(F32) + (r2 * z).astype(F32)
            out[:, a] = s.astype(F32) + t
    return out


def keys_ref(p, tgt):
    """p (m, 3), tgt (N, >= 3) float32 -> (m, N) float32 keys d = fl32(fl32(dx*dx + dy*dy) + dz*dz)"""
    with np.errstate(all="ignore"):
        dx = p[:, None, 0] - tgt[None, :, 0]
        dy = p[:, None, 1] - tgt[None, :, 1]
        dz = p[:, None, 2] - tgt[None, :, 2]
        return ((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32) + (dz * dz).astype(F32)


def pairs_ref(tgt, src, pose, dist, chunk=1024):
    """-> (nn_idx (M) int32, nn_d2 (M) float32): per source row the target row least in (key, index) among those with key <= fl32(D * D)"""
    tgt = np.asarray(tgt, F32)
    p = transform_ref(src, pose)
    r2 = F32(F32(dist) * F32(dist))
    idx, d2 = np.full(p.shape[0], -1, np.int32), np.full(p.shape[0], np.inf, F32)
    for a in range(0, p.shape[0], chunk):
        d = keys_ref(p[a:a + chunk], tgt)
        d = np.where(d <= r2, d, F32(np.inf))                          # a NaN key fails the comparison
        j = np.argmin(d, axis=1)                                      # the first of equal keys: the lowest index
        best = d[np.arange(d.shape[0]), j]
        ok = best <= r2
        idx[a:a + chunk] = np.where(ok, j, -1)
        d2[a:a + chunk] = np.where(ok, best, F32(np.inf))
    return idx, d2


def terms_ref(tgt, src, pose, centre, idx, normals=None):
    """-> (rows, 32) float64: the terms each source row adds to the sums, zero rows for the unpaired; normals (N, 3) float32: the plane metric"""
    tgt = np.asarray(tgt, F32)
    p = transform_ref(src, pose)
    M = p.shape[0]
    T = np.zeros((M, SUMS), F64)
    ok = (idx >= 0) & np.isfinite(p).all(1)
    j = np.where(ok, idx, 0)
    q = tgt[j, :3]
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
        key = (((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32) + (dz * dz).astype(F32)).astype(F64)
        c = np.asarray(centre, F32).astype(F64)
        u = p.astype(F64) - c
        if normals is None:
            v = q.astype(F64) - c
            T[:, 0], T[:, 1] = 1.0, key
            T[:, 2:5], T[:, 5:8] = u, v
            T[:, 8:17] = (u[:, :, None] * v[:, None, :]).reshape(M, 9)
        else:
            raw = np.asarray(normals, F32)[j, :3].astype(F64)
            length = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
            good = (length > 0) & np.isfinite(length)
            n = raw / np.where(good, length, 1.0)[:, None]
            e = p.astype(F64) - q.astype(F64)
            r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
            a = np.stack([u[:, 1] * n[:, 2] - u[:, 2] * n[:, 1], u[:, 2] * n[:, 0] - u[:, 0] * n[:, 2], u[:, 0] * n[:, 1] - u[:, 1] * n[:, 0]], 1)
            J = np.concatenate([a, n], 1)
            T[:, 0], T[:, 1], T[:, 2] = 1.0, key, r * r
            T[:, 3:9] = J * r[:, None]
            iu = np.triu_indices(6)
            T[:, 9:30] = J[:, iu[0]] * J[:, iu[1]]
            T[~good] = 0.0
            T[~good, 30] = 1.0
    T[~ok] = 0.0
    return T


def sums_ref(tgt, src, pose, centre, dist, normals=None):
    """-> (sums (32), sum of |term| (32), nn_idx, nn_d2): the sums exactly rounded (math.fsum)"""
    idx, d2 = pairs_ref(tgt, src, pose, dist)
    T = terms_ref(tgt, src, pose, centre, idx, normals)
    return np.array([math.fsum(T[:, s]) for s in range(SUMS)]), np.abs(T).sum(0), idx, d2


def fast_sums(tgt, src, pose, centre, dist, normals=None):
    """The sums by numpy's own order: what the ICP loop of the host tests iterates on."""
    idx, _ = pairs_ref(tgt, src, pose, dist)
    return terms_ref(tgt, src, pose, centre, idx, normals).sum(0)


# ---- the loop of pc_register.register_rows on the restatement ----------------------------------------------------------------------------
def register_ref(scans, dist, iters=30, tol=1e-6, metric="plane", min_overlap=0.3, normals=None):
    """scans: (N_j, 3 | 6) arrays; normals: per scan (N_j, 3) or None = columns 3:6 -> ([(R, t)], [icp's result per scan]); the union and
    its casts as register_rows makes them"""
    from meshanything_amd import pc_register
    plane = metric == "plane"
    nrm = [np.asarray(s[:, 3:6] if normals is None else normals[j], F32) for j, s in enumerate(scans)] if plane else None
    union, union_n = np.asarray(scans[0][:, :3], F32), (nrm[0] if plane else None)
    poses, results = [pc_register.IDENTITY], [None]
    for j in range(1, len(scans)):
        s = scans[j]
        src = np.asarray(s[:, :3], F32)
        centre = s[:, :3].astype(F64).mean(0).astype(F32)
        res = pc_register.icp(lambda p: fast_sums(union, src, pc_register.pose12(p), centre, dist, union_n), centre.astype(F64), s.shape[0], iters, tol, metric,
                              min_overlap, str(j), "ref")
        R, t = res["pose"]
        poses.append((R, t))
        results.append(res)
        union = np.concatenate([union, (s[:, :3].astype(F64) @ R.T + t).astype(F32)])
        if plane:
            union_n = np.concatenate([union_n, (nrm[j].astype(F64) @ R.T).astype(F32)])
    return poses, results


# ---- the test solid: a 1 x 0.6 x 0.3 box with a 0.3^3 box on one corner, and its cuts -----------------------------------------------------
BOXES = (((0.0, 0.0, 0.0), (1.0, 0.6, 0.3)), ((0.0, 0.0, 0.3), (0.3, 0.3, 0.6)))


def solid_surface(n, seed):
    """-> (xyz (n, 3), normals (n, 3)) float64: n uniform samples of the solid's surface with the outward face normals"""
    rng = np.random.default_rng(seed)
    faces = []
    for lo, hi in BOXES:
        lo, hi = np.array(lo), np.array(hi)
        for axis in range(3):
            for side in (0, 1):
                o = [a for a in range(3) if a != axis]
                faces.append((lo, hi, axis, side, (hi - lo)[o[0]] * (hi - lo)[o[1]]))
    area = np.array([f[4] for f in faces])
    xyz, nrm = np.empty((0, 3)), np.empty((0, 3))
    while xyz.shape[0] < n:
        pick = rng.choice(len(faces), 2 * n, p=area / area.sum())
        uvw = rng.random((2 * n, 3))
        pts, ns = np.empty((2 * n, 3)), np.zeros((2 * n, 3))
        for f, (lo, hi, axis, side, _) in enumerate(faces):
            m = pick == f
            pts[m] = lo + uvw[m] * (hi - lo)
            pts[m, axis] = hi[axis] if side else lo[axis]
            ns[m, axis] = 1.0 if side else -1.0
        keep = np.ones(2 * n, bool)
        bhi = BOXES[1][1]
        on_top = (pts[:, 2] == 0.3)                                   # the shared face: the big box's top under the small one, the small one's bottom
        inside_small_footprint = (pts[:, 0] <= bhi[0]) & (pts[:, 1] <= bhi[1])
        keep &= ~(on_top & inside_small_footprint)
        xyz, nrm = np.concatenate([xyz, pts[keep]]), np.concatenate([nrm, ns[keep]])
    return xyz[:n], nrm[:n]


def rotation(axis, degrees):
    from meshanything_amd import pc_register
    axis = np.asarray(axis, F64)
    return pc_register.exp_so3(axis / np.linalg.norm(axis) * math.radians(degrees))


SCAN_ROWS = 3072                                                   # surface samples per scan before its cut
CUTS = (lambda p: p[:, 0] < 0.75, lambda p: p[:, 0] > 0.25, lambda p: p[:, 1] > 0.1)
TRUE_POSES = ((np.eye(3), np.zeros(3)),
              (rotation((1, 2, 3), 5.0), 0.03 * np.array([2.0, -1.0, 2.0]) / 3.0),
              (rotation((-2, 1, 1), 5.0), 0.03 * np.array([-1.0, 2.0, 2.0]) / 3.0))
DIST = 0.1


def solid_scans(seed, rows=SCAN_ROWS):
    """-> three (N_j, 6) float32 scans of the solid, each its own samples and its own cut, scan j stored in the frame in which TRUE_POSES[j]
    takes it back: x_file = R^T (x - t), n_file = R^T n"""
    out = []
    for j, (cut, (R, t)) in enumerate(zip(CUTS, TRUE_POSES)):
        xyz, nrm = solid_surface(rows, 100 * seed + j)
        m = cut(xyz)
        out.append(np.concatenate([(xyz[m] - t) @ R, nrm[m] @ R], 1).astype(F32))
    return out


def pose_errors(pose, true, xyz):
    """-> (rotation error in radians, the largest displacement of a row of xyz between the two poses)"""
    R, t = pose
    Rt, tt = true
    angle = math.acos(min(max((np.trace(R @ Rt.T) - 1.0) / 2.0, -1.0), 1.0))
    x = np.asarray(xyz, F64)
    return angle, float(np.linalg.norm((x @ R.T + t) - (x @ Rt.T + tt), axis=1).max())


def pca_normals(xyz, k=16):
    """(N, 3) -> (N, 3) float32 unoriented normals from the k nearest rows: the estimate pc_xyz scans get, in plain numpy"""
    x = np.asarray(xyz, F64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    nb = np.argpartition(d, k - 1, axis=1)[:, :k]
    pts = x[nb]
    pts = pts - pts.mean(1, keepdims=True)
    _, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", pts, pts))
    return vec[:, :, 0].astype(F32)


# ---- the kernel cases -------------------------------------------------------------------------------------------------------------------
GRIDS = {"one": ((-0.5, -0.5, -0.5), 2.0, (1, 1, 1)), "flat": ((-0.1, -0.1, -0.1), 0.45, (3, 2, 1)), "fine": ((-0.0625, -0.0625, -0.0625), 0.0703125, (16, 16, 16))}
CASE_POSE = np.concatenate([rotation((1, 2, 3), 5.0).reshape(9), [0.02, -0.01, 0.015]]).astype(F32)
CENTRE = np.array([0.5, 0.4, 0.3], F32)
SHAPES = tuple([(1, 1, 3, 3), (1, 257, 6, 3), (255, 1, 3, 6), (256, 257, 6, 6), (257, 4099, 3, 6), (GROUP_ROWS - 1, 257, 6, 6), (GROUP_ROWS, 4099, 3, 6),
                (GROUP_ROWS + 1, 4099, 6, 6)])                     # (M, N, source ld, target ld)


def uniform_case(M, N, sld, tld, seed=0):
    """-> (target (N, tld), source (M, sld)) float32: uniform in the unit cube, the source reaching 0.2 beyond it on every side (rows outside
    every grid's box), columns 3:6 of a six-column cloud a random vector of any length (the target's are its normals)"""
    rng = np.random.default_rng(1000 * seed + 7 * M + N)
    tgt = rng.random((N, tld)).astype(F32)
    src = (rng.random((M, sld)) * 1.4 - 0.2).astype(F32)
    tgt[:, 3:] = rng.standard_normal((N, tld - 3)).astype(F32)
    return tgt, src


def content_case():
    """-> (target (8, 6), source (7, 3), pose, dist): the identity pose and D = 0.25, r2 = 0.0625 exactly.
    target rows 0 and 1 are duplicates (row 0 wins); rows 2 and 3 lie 0.125 either side of source row 1 (equal keys: row 2 wins); row 4 lies
    exactly 0.25 from source row 2 (key == r2: paired); row 5 has a zero normal and is source row 3's pair (counted in [30]); source row 4
    is not finite, source row 5 is 0.25000003 from row 6 only (no pair), and source row 6 pairs row 7, whose normal has a NaN (counted in [30])."""
    tgt = np.zeros((8, 6), F32)
    tgt[:, 5] = 1.0
    tgt[0, :3] = tgt[1, :3] = (0.0, 0.0, 0.0)
    tgt[2, :3], tgt[3, :3] = (2.0 - 0.125, 0.0, 0.0), (2.0 + 0.125, 0.0, 0.0)
    tgt[4, :3] = (4.0, 0.25, 0.0)
    tgt[5, :3], tgt[5, 3:] = (6.0, 0.0, 0.0), 0.0
    tgt[6, :3] = (8.0, 0.0, 0.0)
    tgt[7, :3], tgt[7, 3:] = (10.0, 0.0, 0.0), (np.nan, 0.0, 1.0)
    src = np.array([[0.0625, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0], [6.0, 0.0, 0.125], [np.nan, 0.0, 0.0], [8.0, 0.0, np.nextafter(F32(0.25), F32(1))],
                    [10.0, 0.0625, 0.0]], F32)
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(F32)
    return tgt, src, pose, 0.25


CONTENT_GRIDS = {"one": ((-1.0, -1.0, -1.0), 12.0, (1, 1, 1)), "cells": ((-0.5, -0.5, -0.5), 0.75, (15, 2, 2))}
