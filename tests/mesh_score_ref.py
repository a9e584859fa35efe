"""Numpy restatement of the candidate scores (meshanything_amd/csrc/mesh_score.hpp) that the mesh-score tests compare against.

* `score_ref`: float64, the definitions of DESIGN.md section 9 by another route than the kernel's: the point-triangle distance is
  `watertight_ref.true_dist` (barycentric projection, no flatness rule), the nearest cloud point a plain minimum over all points.
* `score_f32`: the kernel's own order in float32 (`watertight_ref.tri_dist` with flat = 2^-20, squared distances, seven square roots
  summed in order, times float32(1/7)); its deviation from `score_ref` on the tests' inputs is the measure of what fp32 can resolve
  there, from which the GPU test derives its tolerance.
Plus the crafted inputs the tests share.  A mesh is coords (F, 3, 3) float32 as the detokenizer emits it (NaN rows = invalid faces);
every vertex is multiplied by the float32 mesh_scale first.
"""
import numpy as np

import watertight_ref as W

REPO = W.REPO
FLAT = np.float32(2.0 ** -20)


def valid_rows(coords):
    c = np.asarray(coords, np.float32)
    return np.isfinite(c.reshape(c.shape[0], 9)).all(1)


def _pair_min(dist, tri, pts, chunk=1 << 18):
    """min over the faces tri (F, 3, 3) of dist(A, B, C, p) for every p of pts (P, 3); +inf for F = 0."""
    P = pts.shape[0]
    out = np.full(P, np.inf, pts.dtype)
    step = max(1, chunk // P)
    for f0 in range(0, tri.shape[0], step):
        t = tri[f0:f0 + step]
        n = t.shape[0]
        A, B, C = (np.repeat(t[:, k], P, axis=0) for k in range(3))
        d = dist(A, B, C, np.tile(pts, (n, 1))).reshape(n, P)
        out = np.minimum(out, d.min(0))
    return out


def _quad_points(tri, dtype):
    """(F, 7, 3): the vertices, the edge midpoints AB, BC, CA and the centroid, in the kernel's order and arithmetic."""
    A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
    half, third = dtype(0.5), dtype(1.0) / dtype(3.0)
    return np.stack([A, B, C, half * (A + B), half * (B + C), half * (C + A), (A + B + C) * third], 1).astype(dtype)


def _nearest(q, pts, dtype, chunk=1 << 20):
    """distance from every q (N, 3) to the nearest of pts (P, 3): squared differences summed x, y, z, minimum, then the root"""
    out = np.empty(q.shape[0], dtype)
    step = max(1, chunk // pts.shape[0])
    for i in range(0, q.shape[0], step):
        d = q[i:i + step, None, :] - pts[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        out[i:i + step] = np.sqrt(d2.min(1))
    return out


def _terms(coords, cloud, mesh_scale, dtype):
    c32 = np.asarray(coords, np.float32)
    keep = valid_rows(c32)
    if dtype is np.float32:
        tri = c32[keep] * np.float32(mesh_scale)                       # the kernel scales in float32
        dist = lambda A, B, C, p: W.tri_dist(A, B, C, p, FLAT)         # noqa: E731
    else:
        tri = c32[keep].astype(np.float64) * np.float64(np.float32(mesh_scale))
        dist = W.true_dist
    pts = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3]).astype(dtype)
    pt = _pair_min(dist, tri, pts)
    q = _quad_points(tri, dtype)
    nn = _nearest(q.reshape(-1, 3), pts, dtype).reshape(-1, 7)
    if dtype is np.float32:
        s = np.zeros(nn.shape[0], np.float32)
        for k in range(7):
            s = s + nn[:, k]
        face_nn = s * (np.float32(1.0) / np.float32(7.0))
    else:
        face_nn = nn.mean(1)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = (dtype(0.5) * np.sqrt((n * n).sum(-1))).astype(dtype)
    return keep, pt, face_nn, area


def _scores(keep, pt, face_nn, area):
    nvalid = int(keep.sum())
    a64, m64 = area.astype(np.float64), face_nn.astype(np.float64)
    tot = float(a64.sum())
    c2m = float(pt.astype(np.float64).mean()) if nvalid else np.inf
    m2c = float((a64 * m64).sum() / tot) if nvalid and tot > 0 else np.inf
    return np.array([c2m, m2c, tot, nvalid], np.float64)


def score_ref(coords, cloud, mesh_scale=2.0):
    """One candidate against one cloud in float64: dict(scores (4,), pt_dist (P,), face_nn (F,), face_area (F,)); the per-face arrays
    hold 0 and -1 at the invalid rows, like the kernel's workspace."""
    return _full(coords, *_terms(coords, cloud, mesh_scale, np.float64))


def score_f32(coords, cloud, mesh_scale=2.0):
    """The same in the kernel's float32 order (sums of the terms in float64, as the kernel's reduction)."""
    return _full(coords, *_terms(coords, cloud, mesh_scale, np.float32))


def _full(coords, keep, pt, face_nn, area):
    F = np.asarray(coords).shape[0]
    fn, fa = np.zeros(F), np.full(F, -1.0)
    fn[keep], fa[keep] = face_nn, area
    return {"scores": _scores(keep, pt, face_nn, area), "pt_dist": pt.astype(np.float64), "face_nn": fn, "face_area": fa}


def batch(fn, coords, cloud, n_per_cloud=1, mesh_scale=2.0):
    """fn (score_ref / score_f32) over a batch: coords (B, F, 3, 3), cloud (B / n_per_cloud, P, 3 | 6) -> dict of stacked arrays"""
    rows = [fn(coords[b], cloud[b // n_per_cloud], mesh_scale) for b in range(coords.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---- crafted inputs ------------------------------------------------------------------------------------------------------------
def cube(half=48):
    """(12, 3, 3) float32: a cube of half-extent half / 128 (0.375; 0.75 after the default scale 2), vertices on the 1/128 grid"""
    s = half / 128.0
    v = np.array([[x, y, z] for z in (-s, s) for y in (-s, s) for x in (-s, s)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v[np.array(f)]


def cube_cloud(P=4096, half=96, seed=0, ld=6):
    """(P, ld) float32: points on the surface of the cube of half-extent half / 128 (0.75), on the 1/128 grid; columns 3.. = the normal"""
    rng = np.random.default_rng(seed)
    axis, sign = rng.integers(0, 3, P), rng.integers(0, 2, P) * 2 - 1
    uv = rng.integers(-half, half + 1, (P, 3)).astype(np.float64)
    uv[np.arange(P), axis] = sign * half
    out = np.zeros((P, ld), np.float32)
    out[:, :3] = uv / 128.0
    if ld == 6:
        out[np.arange(P), 3 + axis] = sign
    return out


def soup(F, seed, nan_rows=None):
    """(F, 3, 3) float32 random triangles with vertices on the 1/64 grid in [-1, 1] after the scale 2 (so on the 1/128 grid in
    [-0.5, 0.5] here); nan_rows: indices set to NaN"""
    rng = np.random.default_rng(seed)
    c = (rng.integers(-64, 65, (F, 3, 3)) / 128.0).astype(np.float32)
    if nan_rows is not None:
        c[np.asarray(nan_rows)] = np.nan
    return c


def points(P, seed, ld=3):
    """(P, ld) float32 uniform in [-1, 1]"""
    return np.random.default_rng(seed).uniform(-1, 1, (P, ld)).astype(np.float32)


def voronoi():
    """One triangle (scale 1) and query points in each of its seven Voronoi regions (the face, three edges, three vertices), above the
    face and in its plane, then random ones up to 67 points: (coords (1, 1, 3, 3), cloud (1, 67, 3))"""
    tri = np.array([[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]]], np.float32)
    q = [[0.125, 0.125, 0.25], [0.125, 0.125, 0.0],                   # face: above it, in its plane
         [0.25, -0.25, 0.125], [0.25, -0.25, 0.0],                    # edge AB
         [0.5, 0.5, -0.125], [0.5, 0.5, 0.0],                         # edge BC
         [-0.25, 0.25, 0.125], [-0.25, 0.25, 0.0],                    # edge CA
         [-0.25, -0.25, 0.125], [-0.25, -0.25, 0.0],                  # vertex A
         [0.75, -0.125, 0.125], [0.75, -0.125, 0.0],                  # vertex B
         [-0.125, 0.75, 0.125], [-0.125, 0.75, 0.0]]                  # vertex C
    q = np.array(q, np.float32)
    return tri[None], np.concatenate([q, points(67 - len(q), 11)])[None]


def degenerate_batch():
    """(coords (3, 5, 3, 3), cloud (3, 67, 6)), scale 2: row 0 all NaN; row 1 zero-area faces only (a repeated vertex, three equal
    vertices, exactly collinear ones, NaN rows); row 2 a repeated-vertex face, a collinear face and three proper ones"""
    c = np.full((3, 5, 3, 3), np.nan, np.float32)
    seg = np.array([[0.25, 0.0, 0.125], [-0.25, 0.25, 0.0], [-0.25, 0.25, 0.0]], np.float32)
    dot = np.array([[0.125, -0.25, 0.25]] * 3, np.float32)
    col = np.array([[-0.375, -0.375, 0.0], [0.0, -0.125, 0.125], [0.375, 0.125, 0.25]], np.float32)
    c[1, 0], c[1, 2], c[1, 3] = seg, dot, col
    c[2, 0], c[2, 1] = seg, col
    c[2, 2:] = soup(3, 5)
    return c, np.stack([points(67, 20 + g, 6) for g in range(3)])


def cases():
    """name -> (coords (B, F, 3, 3), cloud (G, P, ld), n_per_cloud, mesh_scale): the kernel-against-reference cases.  F in {1, 5, 130,
    800}, P in {1, 67, 4096}, B in {1, 3, 12}, n_per_cloud in {1, 4} with distinct clouds, cloud_ld 3 and 6."""
    out = {}
    tri, q = voronoi()
    out["voronoi"] = (tri, q, 1, 1.0)
    out["one_point"] = (soup(1, 1)[None], points(1, 2)[None], 1, 2.0)
    out["cube"] = (cube()[None], cube_cloud()[None], 1, 2.0)
    out["degenerate"] = degenerate_batch() + (1, 2.0)
    nan_rows = np.flatnonzero(np.random.default_rng(3).random(800) < 0.4)
    mixed = soup(800, 4, nan_rows)
    out["nan_interleaved"] = (mixed[None], points(67, 5)[None], 1, 2.0)
    out["nan_compacted"] = (mixed[valid_rows(mixed)][None], points(67, 5)[None], 1, 2.0)
    out["soup_800"] = (soup(800, 6)[None], points(4096, 7)[None], 1, 2.0)
    groups = np.stack([soup(130, 30 + b, np.arange(130 - 9 * (b % 5), 130) if b % 5 else None) for b in range(12)])
    out["groups"] = (groups, np.stack([points(67, 40 + g, 6) for g in range(3)]), 4, 2.0)
    out["five_faces"] = (np.stack([soup(5, 50 + b) for b in range(3)]), np.stack([points(1, 60 + g) for g in range(3)]), 1, 2.0)
    return out


def ranking():
    """(coords (4, 12, 3, 3), cloud (1, 4096, 6)) for the cube's cloud: the cube, the cube shifted by 0.1 (cloud units), the cube with
    every second face NaN, the cube scaled by 0.5"""
    c = cube()
    half = c.copy()
    half[1::2] = np.nan
    return np.stack([c, c + np.float32(0.05), half, c * np.float32(0.5)]), cube_cloud()[None]
