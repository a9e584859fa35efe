"""Numpy restatement of ma_op_pc_spfh, ma_op_pc_spfh_gather, ma_op_pc_desc_match and ma_op_pc_pose_score (include/meshanything_amd.h,
csrc/pc_coarse.hpp), shared by the host and the GPU tests: float32 with every rounding explicit, brute force over ALL rows; the ops of
`pc_coarse.coarse_pose` on top of them (`RefOps`); and the fixture, two cut scans of a bumpy ellipsoid at an arbitrary pose."""
import functools
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import pc_fps_ref                                                  # noqa: E402
import pc_register_ref as RR                                       # noqa: E402

F32, F64 = np.float32, np.float64
BINS, DESC, COLS = 11, 33, 34


# ---- the ops ------------------------------------------------------------------------------------------------------------------------------
def dot_ref(u, v):
    """fl32(fl32(fl32(u_x v_x) + fl32(u_y v_y)) + fl32(u_z v_z)) over the last axis, broadcasting"""
    s = (u[..., 0] * v[..., 0]).astype(F32) + (u[..., 1] * v[..., 1]).astype(F32)
    return s.astype(F32) + (u[..., 2] * v[..., 2]).astype(F32)


def bin_ref(v):
    w = (v * F32(BINS)).astype(F32)
    return np.where(w >= F32(BINS - 1), BINS - 1, np.where(w >= F32(BINS - 1), 0, w).astype(np.int64))


def usable_ref(n):
    return np.isfinite(n).all(-1) & (n != 0).any(-1)


def neighbours_ref(rows, xyz, radius):
    """rows (m, 3), xyz (N, 3) float32 -> (mask (m, N) of 0 < d <= fl32(F * F), the differences (m, N, 3), d)"""
    r2 = F32(F32(radius) * F32(radius))
    with np.errstate(all="ignore"):
        diff = (rows[:, None, :] - xyz[None, :, :]).astype(F32)
        d = ((diff[..., 0] * diff[..., 0]).astype(F32) + (diff[..., 1] * diff[..., 1]).astype(F32)).astype(F32) + (diff[..., 2] * diff[..., 2]).astype(F32)
        return (d > 0) & (d <= r2), diff, d


def spfh_ref(cloud, normals, radius, chunk=256):
    """cloud (N, >= 3), normals (N, >= 3) float32 -> hist (N, 34) uint32"""
    xyz, nrm = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3]), np.ascontiguousarray(np.asarray(normals, F32)[:, :3])
    N = xyz.shape[0]
    hist = np.zeros((N, COLS), np.int64)
    ok_n = usable_ref(nrm)
    for a in range(0, N, chunk):
        rows = slice(a, min(a + chunk, N))
        m = rows.stop - a
        with np.errstate(all="ignore"):
            mask, diff, d = neighbours_ref(xyz[rows], xyz, radius)
            length = np.sqrt(d).astype(F32)
            fa = (np.abs(dot_ref(nrm[rows][:, None, :], diff)) / length).astype(F32)
            fb = (np.abs(dot_ref(nrm[None, :, :], diff)) / length).astype(F32)
            fc = np.broadcast_to(np.abs(dot_ref(nrm[rows][:, None, :], nrm[None, :, :])), fa.shape)
        use = mask & ok_n[rows][:, None] & ok_n[None, :] & ~(np.isnan(fa) | np.isnan(fb) | np.isnan(fc))
        p, q = np.nonzero(use)
        for block, f in enumerate((fa, fb, fc)):
            np.add.at(hist[a:a + m], (p, block * BINS + bin_ref(f[p, q])), 1)
        hist[a:a + m, DESC] = use.sum(1)
    assert hist.max(initial=0) < 1 << 32
    return hist.astype(np.uint32)


def gather_ref(cloud, hist, radius, query, chunk=256):
    """-> desc (Q, 33) uint32: hist[p] + the sum of hist[q] over the neighbours of p = query[j], modulo 2^32"""
    xyz = np.ascontiguousarray(np.asarray(cloud, F32)[:, :3])
    h = np.asarray(hist).astype(np.uint64)[:, :DESC]
    query = np.asarray(query, np.int64)
    desc = np.zeros((query.shape[0], DESC), np.uint64)
    for a in range(0, query.shape[0], chunk):
        q = query[a:a + chunk]
        mask = neighbours_ref(xyz[q], xyz, radius)[0]
        desc[a:a + chunk] = h[q] + mask.astype(np.uint64) @ h
    return (desc & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def normalise_ref(D):
    """(K, 33) uint32 -> (K, 33) float32: every block of 11 over its integer sum, a zero block stays zero"""
    D = np.asarray(D).astype(np.uint64)
    out = np.zeros(D.shape, F32)
    for b in range(3):
        blk = D[:, b * BINS:(b + 1) * BINS]
        S = blk.sum(1)
        with np.errstate(all="ignore"):
            x = (blk.astype(F32) / S.astype(F32)[:, None]).astype(F32)
        out[:, b * BINS:(b + 1) * BINS] = np.where(S[:, None] > 0, x, F32(0))
    return out


def match_ref(A, B, chunk=256):
    """-> (idx (Ka) int32, dist (Ka) float32): the row of B least in (distance, index); the distance summed bin after bin in float32"""
    x, y = normalise_ref(A), normalise_ref(B)
    idx, dist = np.empty(x.shape[0], np.int32), np.empty(x.shape[0], F32)
    for a in range(0, x.shape[0], chunk):
        s = np.zeros((min(chunk, x.shape[0] - a), y.shape[0]), F32)
        for k in range(DESC):
            e = (x[a:a + chunk, None, k] - y[None, :, k]).astype(F32)
            s = (s + (e * e).astype(F32)).astype(F32)
        j = np.argmin(s, axis=1)                                       # the first of equal distances: the lowest index
        idx[a:a + chunk], dist[a:a + chunk] = j, s[np.arange(s.shape[0]), j]
    return idx, dist


def score_ref(poses, P, Q, dist):
    """poses (H, 12), P, Q (C, 3) -> (counts (H) int32, best): the highest count, the lowest index among equals"""
    poses, P, Q = np.asarray(poses, F32), np.asarray(P, F32), np.asarray(Q, F32)
    t2 = F32(F32(dist) * F32(dist))
    counts = np.empty(poses.shape[0], np.int32)
    with np.errstate(all="ignore"):
        for h in range(poses.shape[0]):
            d = RR.transform_ref(P, poses[h]) - Q
            key = ((d[:, 0] * d[:, 0]).astype(F32) + (d[:, 1] * d[:, 1]).astype(F32)).astype(F32) + (d[:, 2] * d[:, 2]).astype(F32)
            counts[h] = int((key <= t2).sum())
    return counts, int(np.argmax(counts))


class RefOps:
    """The device steps of pc_coarse.coarse_pose by the restatement."""

    def keypoints(self, xyz, k):
        return pc_fps_ref.fps_ref(xyz, k)[0].astype(np.int64)

    def describe(self, xyz, normals, radius, query):
        return gather_ref(xyz, spfh_ref(xyz, normals, radius), radius, query).astype(np.int64)

    def match(self, A, B):
        return match_ref(A, B)[0].astype(np.int64)

    def score(self, poses, P, Q, dist):
        return score_ref(poses, P, Q, dist)


# ---- a float64 brute force by the plain definition, for small clouds ---------------------------------------------------------------------
def spfh_plain(cloud, normals, radius):
    """hist (N, 34) by two loops in float64; it equals the restatement wherever no feature lies within rounding of a bin edge or the rim"""
    x, n = np.asarray(cloud, F64)[:, :3], np.asarray(normals, F64)[:, :3]
    N = x.shape[0]
    hist = np.zeros((N, COLS), np.int64)
    for p in range(N):
        for q in range(N):
            D = x[p] - x[q]
            d = float(D @ D)
            if not 0.0 < d <= radius * radius:
                continue
            length = math.sqrt(d)
            for block, v in enumerate((abs(n[p] @ D) / length, abs(n[q] @ D) / length, abs(n[p] @ n[q]))):
                hist[p, block * BINS + min(BINS - 1, int(v * BINS))] += 1
            hist[p, DESC] += 1
    return hist


# ---- the kernel cases ---------------------------------------------------------------------------------------------------------------------
SPFH_N = (1, 2, 63, 64, 65, 257, 4099)
GATHER_Q = (1, 257)
MATCH_SHAPES = ((1, 1), (63, 4096), (64, 65), (65, 64), (257, 63), (4096, 257), (4096, 4096))     # (Ka, Kb)
SCORE_SHAPES = ((1, 1), (255, 3), (256, 257), (257, 4096), (4096, 257), (4096, 4096))            # (H, C)


def cloud_case(N, ld):
    """-> (cloud (N, ld), normals (N, 4) or None) float32: uniform in [-0.1, 1.1)^3, so that rows lie outside every grid's box; a six-column
    cloud carries unit normals in columns 3:6, a three-column one gets a separate array of leading dimension 4"""
    rng = np.random.default_rng(31 * N + ld)
    xyz = (rng.random((N, 3)) * 1.2 - 0.1).astype(F32)
    n = rng.normal(size=(N, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    if ld == 6:
        return np.concatenate([xyz, n], 1), None
    return xyz, np.concatenate([n, rng.normal(size=(N, 1)).astype(F32)], 1)


def normals_of(cloud, normals):
    return cloud[:, 3:6] if normals is None else normals[:, :3]


def query_case(N, Q):
    """Q rows of a cloud of N, repeats included; one query: the last row"""
    return np.array([N - 1], np.int32) if Q == 1 else np.random.default_rng(N + Q).integers(0, N, Q).astype(np.int32)


CONTENT_RADIUS = 0.25                                               # r2 = 0.0625 exactly
CONTENT_GRIDS = {"one": ((-1.0, -1.0, -1.0), 12.0, (1, 1, 1)), "cells": ((-0.5, -0.5, -0.5), 0.75, (8, 8, 8))}


def content_case():
    """-> cloud (9, 6): rows 0 and 1 are duplicates (no direction between them: they do not count for each other); row 2 lies exactly 0.25
    from them (key == r2: a neighbour); row 3 is an ordinary neighbour; row 4 is alone (an all-zero histogram); row 5 has a zero normal and row 6
    a NaN in its normal (their own rows are zero and they count for nobody); row 7 lies 0.25000003 from rows 0 and 1 (no neighbour of
    theirs); row 8 has a normal of length 3 at a right angle to nothing (features above 1 go to the last bin)."""
    c = np.zeros((9, 6), F32)
    c[:, 5] = 1.0
    c[2, :3], c[2, 3:] = (0.25, 0.0, 0.0), (1.0, 0.0, 0.0)
    c[3, :3], c[3, 3:] = (0.125, 0.0625, 0.0), (0.0, 1.0, 0.0)
    c[4, :3] = (5.0, 5.0, 5.0)
    c[5, :3], c[5, 3:] = (0.125, 0.0, 0.0625), 0.0
    c[6, :3], c[6, 3:] = (0.0625, 0.125, 0.0), (np.nan, 0.0, 1.0)
    c[7, :3] = (0.0, np.nextafter(F32(0.25), F32(1)), 0.0)
    c[8, :3], c[8, 3:] = (0.125, 0.125, 0.0625), (2.0, 2.0, 1.0)
    return c


def match_case(Ka, Kb):
    """-> (A (Ka, 33), B (Kb, 33)) uint32: rows of B repeated further down and copied into A (ties at distance 0: the lowest index), an all-zero
    descriptor on either side, a zero block, and values up to 2^32 - 1"""
    rng = np.random.default_rng(7 * Ka + Kb)
    A, B = rng.integers(0, 3000, (Ka, DESC)).astype(np.uint32), rng.integers(0, 3000, (Kb, DESC)).astype(np.uint32)
    if Kb >= 63:
        B[40:60] = B[:20]
        B[7] = 0
        B[9, 22:] = 0
        B[11] = 0xFFFFFFFF
    if Ka >= 63:
        A[5] = 0
        A[6, :11] = 0
        A[12] = 0xFFFFFFFF
        A[20:40] = B[np.arange(20) % Kb]
    return A, B


def score_case(H, C):
    """-> (poses (H, 12), P, Q (C, 3) float32, T): Q is P under one pose plus noise of about T; the hypotheses scatter about that pose, which
    itself stands at H // 2 and again at H - 1 (equal counts: the lower index); (1, 1): the identity and a pair exactly T apart"""
    if (H, C) == (1, 1):
        return np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(F32)[None], np.zeros((1, 3), F32), np.array([[0.25, 0.0, 0.0]], F32), 0.25
    rng = np.random.default_rng(13 * H + C)
    P = rng.random((C, 3))
    R, t = RR.rotation(rng.normal(size=3), 75.0), rng.normal(size=3)
    Q = P @ R.T + t + 0.03 * rng.normal(size=(C, 3))
    poses = np.stack([np.concatenate([(RR.rotation(rng.normal(size=3), 3.0 * rng.random()) @ R).reshape(9), t + 0.02 * rng.normal(size=3)]) for _ in range(H)])
    poses[H // 2] = poses[H - 1] = np.concatenate([R.reshape(9), t])
    return poses.astype(F32), P.astype(F32), Q.astype(F32), 0.05


# ---- the fixture: two cut scans of a bumpy ellipsoid ------------------------------------------------------------------------------------------
CENTRES = np.array([[1, .2, .1], [-.3, .9, .2], [.1, -.5, .8], [-.6, -.6, -.5], [.5, .5, -.7], [0, -.2, -1]], F64)
CENTRES /= np.linalg.norm(CENTRES, axis=1, keepdims=True)
AMPS = np.array([.35, -.2, .3, .25, -.25, .4])
WIDTHS = np.array([.35, .5, .3, .45, .4, .25])
SCAN_ROWS = 3072
SEEDS = tuple(range(6))
RADIUS, POINTS, ITERS, DIST = 0.15, 512, 4096, 0.04                # F, K, H, T of the check
ICP_DIST = 0.1


def ellipsoid(n, seed):
    """(n, 3) float64 samples of the surface x = u r(u) (1, 0.8, 0.6), r = 0.5 + 0.5 sum A_i exp(-(1 - u . C_i) / W_i^2)"""
    u = np.random.default_rng(seed).normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.5 + 0.5 * (AMPS * np.exp(-(1.0 - u @ CENTRES.T) / WIDTHS ** 2)).sum(1)
    return u * r[:, None] * np.array([1.0, 0.8, 0.6])


def true_pose(s):
    """The pose that takes scan 1 of seed s back onto scan 0: a turn by 30 + 30 s degrees about a random axis and a shift of 0.5 normal(3)"""
    g = np.random.default_rng(1000 + s)
    R = RR.rotation(g.normal(size=3), 30.0 + 30.0 * s)
    return R, 0.5 * g.normal(size=3)


@functools.lru_cache(maxsize=None)
def scans(s):
    """-> two (N_j, 6) float32 scans with UNORIENTED normals in columns 3:6 (pc_register_ref.pca_normals of each scan alone), scan 1 stored
    in the frame from which true_pose(s) takes it back: x_file = R^T (x - t).  Built once per seed; nobody writes to them."""
    a, b = ellipsoid(SCAN_ROWS, 10 * s), ellipsoid(SCAN_ROWS, 10 * s + 1)
    a, b = a[a[:, 0] < 0.35], b[b[:, 0] > -0.35]
    R, t = true_pose(s)
    b = (b - t) @ R
    out = tuple(np.concatenate([x, RR.pca_normals(x)], 1).astype(F32) for x in (a, b))
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def coarse_ref(s):
    """pc_coarse.coarse_pose of scan 1 onto scan 0 of seed s by the restatement, computed once"""
    from meshanything_amd import pc_coarse
    a, b = scans(s)
    return pc_coarse.coarse_pose(a[:, :3], a[:, 3:6], b[:, :3], b[:, 3:6], RADIUS, POINTS, ITERS, DIST, ops=RefOps(), scan="1", uid=f"seed{s}")


@functools.lru_cache(maxsize=None)
def icp_ref(s, coarse=True):
    """pc_register.icp over the restatement's sums from the coarse pose (or the identity), plane metric, D = ICP_DIST"""
    from meshanything_amd import pc_register
    a, b = scans(s)
    centre = b[:, :3].astype(F64).mean(0).astype(F32)
    start = coarse_ref(s)["pose"] if coarse else pc_register.IDENTITY
    return pc_register.icp(lambda p: RR.fast_sums(a[:, :3], b[:, :3], pc_register.pose12(p), centre, ICP_DIST, a[:, 3:6]), centre.astype(F64), b.shape[0],
                           30, 1e-6, "plane", 0.3, "1", f"seed{s}", pose=start)
