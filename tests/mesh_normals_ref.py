"""Numpy restatement of the normal agreement between a mesh and its cloud (meshanything_amd/csrc/mesh_normals.hpp, DESIGN.md section
12) that the mesh-normals tests compare against, done twice:

* `agree_f32`: float32 in the kernel's order -- the nearest cloud index of every quadrature point by the pair (d, p), d = fl(fl(dx*dx +
  dy*dy) + dz*dz); t_k, a_f and u_f summed in order and multiplied by float32(1/7); the sums over faces in float64 in the reduction's
  order (the c-th valid face into accumulator c mod 256, then one tree).  numpy evaluates every float32 operation on its own, which is
  the kernel's arithmetic without FMA contraction.
* `agree_f64`: float64 by the plain definitions (argmin, mean, area-weighted mean); `idx=` evaluates it on given nearest indices, so
  that a comparison of values is not a comparison of tie-breaks.
Plus the crafted inputs the tests share.  A mesh is coords (F, 3, 3) float32 (NaN rows = invalid faces), every vertex is multiplied by
the float32 mesh_scale first; a cloud is (P, 6) float32, xyz then the normal, used as given.
"""
import numpy as np

import mesh_score_ref as S

REPO = S.REPO
SEVENTH = np.float32(1.0) / np.float32(7.0)


def nearest_f32(q, pts):
    """(N,) int32: argmin over p of the pair (d, p) in float32; a NaN key never wins and all-(inf | NaN) gives 0"""
    out = np.empty(q.shape[0], np.int32)
    step = max(1, (1 << 20) // pts.shape[0])
    with np.errstate(all="ignore"):
        for i in range(0, q.shape[0], step):
            d = q[i:i + step, None, :] - pts[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == np.float32
            d2 = np.where(np.isnan(d2), np.float32(np.inf), d2)
            out[i:i + step] = np.argmin(d2, axis=1)                # the first index that attains the minimum
    return out


def nearest_f64(q, pts):
    q, pts = q.astype(np.float64), pts.astype(np.float64)
    out = np.empty(q.shape[0], np.int32)
    step = max(1, (1 << 20) // pts.shape[0])
    with np.errstate(all="ignore"):
        for i in range(0, q.shape[0], step):
            d2 = ((q[i:i + step, None, :] - pts[None, :, :]) ** 2).sum(-1)
            out[i:i + step] = np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1)
    return out


def _reduce_kernel_order(valid, meas, area, u, a):
    """the reduction of reduce_normals_kernel in float64: valid face number c -> accumulator c mod 256, then the tree"""
    acc = np.zeros((3, 256), np.float64)
    c = 0
    for f in np.flatnonzero(valid):
        if meas[f]:
            s = c & 255
            acc[0, s] += float(area[f]) * float(u[f])
            acc[1, s] += float(area[f]) if a[f] < 0 else 0.0
            acc[2, s] += float(area[f])
        c += 1
    o = 128
    while o:
        acc[:, :o] += acc[:, o:2 * o]
        o >>= 1
    tot = acc[2, 0]
    nc = np.float32(acc[0, 0] / tot) if tot > 0 else np.float32(0)
    fl = np.float32(acc[1, 0] / tot) if tot > 0 else np.float32(0)
    return np.array([nc, fl, np.float32(min(tot, float(np.finfo(np.float32).max))), c], np.float64)


def agree_f32(coords, cloud, mesh_scale=2.0, idx=None):
    """One candidate against one cloud in the kernel's float32 order: dict(nscores (4,), face_agree (F,), face_abs (F,), face_area (F,)
    with -1 at invalid rows and 0 where the face is not measurable, nn_idx (F, 7) int32 with -1 at invalid rows)"""
    c32 = np.asarray(coords, np.float32)
    cl = np.asarray(cloud, np.float32)
    F = c32.shape[0]
    valid = S.valid_rows(c32)
    with np.errstate(all="ignore"):
        tri = c32[valid] * np.float32(mesh_scale)
        q = S._quad_points(tri, np.float32)
        j = nearest_f32(q.reshape(-1, 3), np.ascontiguousarray(cl[:, :3])).reshape(-1, 7) if idx is None else np.asarray(idx)[valid]
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        meas = np.isfinite(l2) & (l2 > 0)
        area = np.where(meas, np.float32(0.5) * np.sqrt(l2), np.float32(0)).astype(np.float32)
        nh = n / np.sqrt(l2)[:, None]
        m = cl[:, 3:6][j]                                             # (Fv, 7, 3)
        t = (nh[:, None, 0] * m[..., 0] + nh[:, None, 1] * m[..., 1]) + nh[:, None, 2] * m[..., 2]
        s, sa = np.zeros(t.shape[0], np.float32), np.zeros(t.shape[0], np.float32)
        for k in range(7):
            s = s + t[:, k]
            sa = sa + np.abs(t[:, k])
        a = np.where(meas, s * SEVENTH, np.float32(0)).astype(np.float32)
        u = np.where(meas, sa * SEVENTH, np.float32(0)).astype(np.float32)
    assert a.dtype == np.float32 and t.dtype == np.float32
    out = {"face_agree": np.zeros(F, np.float64), "face_abs": np.zeros(F, np.float64), "face_area": np.full(F, -1.0), "nn_idx": np.full((F, 7), -1, np.int32)}
    out["face_agree"][valid], out["face_abs"][valid], out["face_area"][valid], out["nn_idx"][valid] = a, u, area, j
    m_full = np.zeros(F, bool)
    m_full[valid] = meas
    out["nscores"] = _reduce_kernel_order(valid, m_full, out["face_area"], out["face_abs"], out["face_agree"])
    return out


def agree_f64(coords, cloud, mesh_scale=2.0, idx=None):
    """The same by the plain definitions in float64; idx (F, 7): evaluate on these nearest indices instead of the float64 argmin"""
    c32 = np.asarray(coords, np.float32)
    cl = np.asarray(cloud, np.float32).astype(np.float64)
    F = c32.shape[0]
    valid = S.valid_rows(c32)
    with np.errstate(all="ignore"):
        tri = c32[valid].astype(np.float64) * np.float64(np.float32(mesh_scale))
        A, B, C = tri[:, 0], tri[:, 1], tri[:, 2]
        q = np.stack([A, B, C, (A + B) / 2, (B + C) / 2, (C + A) / 2, (A + B + C) / 3], 1)
        j = nearest_f64(q.reshape(-1, 3), cl[:, :3]).reshape(-1, 7) if idx is None else np.asarray(idx)[valid]
        n = np.cross(B - A, C - A)
        ln = np.linalg.norm(n, axis=1)
        meas32 = agree_measurable(c32, mesh_scale)[valid]            # which faces count is fp32's call (an fp32 overflow is finite in fp64)
        t = np.einsum("fc,fkc->fk", n / ln[:, None], cl[:, 3:6][j])
        a = np.where(meas32, t.mean(1), 0.0)
        u = np.where(meas32, np.abs(t).mean(1), 0.0)
        area = np.where(meas32, 0.5 * ln, 0.0)
    out = {"face_agree": np.zeros(F), "face_abs": np.zeros(F), "face_area": np.full(F, -1.0), "nn_idx": np.full((F, 7), -1, np.int32)}
    out["face_agree"][valid], out["face_abs"][valid], out["face_area"][valid], out["nn_idx"][valid] = a, u, area, j
    w = area[meas32]
    tot = float(w.sum())
    nc = float((w * u[meas32]).sum() / tot) if tot > 0 else 0.0
    fl = float(w[a[meas32] < 0].sum() / tot) if tot > 0 else 0.0
    out["nscores"] = np.array([nc, fl, tot, int(valid.sum())], np.float64)
    return out


def agree_measurable(coords, mesh_scale=2.0):
    """(F,) bool: valid, and the float32 squared length of the face's normal is finite and > 0"""
    c32 = np.asarray(coords, np.float32)
    valid = S.valid_rows(c32)
    with np.errstate(all="ignore"):
        tri = c32 * np.float32(mesh_scale)
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return valid & np.isfinite(l2) & (l2 > 0)


def batch(fn, coords, cloud, n_per_cloud=1, mesh_scale=2.0, idx=None):
    rows = [fn(coords[b], cloud[b // n_per_cloud], mesh_scale, None if idx is None else idx[b]) for b in range(coords.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def tie_share(coords, cloud, mesh_scale=2.0):
    """the share of the quadrature points of the valid faces whose least float32 distance is attained by more than one cloud point"""
    c32 = np.asarray(coords, np.float32)
    q = S._quad_points(c32[S.valid_rows(c32)] * np.float32(mesh_scale), np.float32).reshape(-1, 3)
    pts = np.asarray(cloud, np.float32)[:, :3]
    d = q[:, None, :] - pts[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return float(((d2 == d2.min(1, keepdims=True)).sum(1) > 1).mean())


# ---- crafted inputs ------------------------------------------------------------------------------------------------------------
GRID_F = (1, 63, 64, 65, 130)                  # around the 64 faces of a workgroup
GRID_P = (1, 1023, 1024, 1025, 2500)           # around the 1024 points of an LDS tile
NAMED = {"soup_130": ((130, 31), (2500, 41)), "soup_800": ((800, 6), (4096, 7)), "soup_65": ((65, 8), (1025, 9))}


def tripled_cloud(P=400, seed=70):
    """(3 * P, 6): every point three times (rows p, p + P, p + 2 P, so that the copies lie in different LDS tiles) with three normals"""
    base = S.points(P, seed, 6)
    rng = np.random.default_rng(seed + 1)
    rows = []
    for _ in range(3):
        c = base.copy()
        c[:, 3:] = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
        rows.append(c)
    return np.concatenate(rows)


def degenerate6():
    """(coords (4, 5, 3, 3), cloud (4, 67, 6)), scale 2: the three rows of mesh_score_ref.degenerate_batch (all NaN; zero-area faces
    only; two zero-area faces and three proper ones) and a row near FLT_MAX: faces whose scaled vertices stay finite while their
    differences and products overflow, faces whose vertices overflow in the scaling, and one NaN row"""
    c3, cl3 = S.degenerate_batch()
    rng = np.random.default_rng(77)
    big = np.full((5, 3, 3), np.nan, np.float32)
    big[0:2] = (rng.choice([-1.0, 1.0], (2, 3, 3)) * rng.uniform(0.9e38, 1.6e38, (2, 3, 3))).astype(np.float32)      # finite after the scale
    big[2:4] = (rng.choice([-1.0, 1.0], (2, 3, 3)) * rng.uniform(2.0e38, 3.3e38, (2, 3, 3))).astype(np.float32)      # +-inf after the scale
    return np.concatenate([c3, big[None]]), np.concatenate([cl3, S.points(67, 23, 6)[None]])


def cases():
    """name -> (coords (B, F, 3, 3), cloud (G, P, 6), n_per_cloud, mesh_scale)"""
    out = {}
    for F in GRID_F:
        for P in GRID_P:
            out[f"grid_{F}_{P}"] = (S.soup(F, 100 + F)[None], S.points(P, 200 + P, 6)[None], 1, 2.0)
    for B, n in ((1, 1), (3, 1), (3, 3), (6, 1), (6, 3)):
        c = np.stack([S.soup(65, 300 + 10 * B + b, np.arange(b % 3, 65, 7)) for b in range(B)])
        out[f"batch_{B}_{n}"] = (c, np.stack([S.points(1025, 400 + 10 * B + g, 6) for g in range(B // n)]), n, 2.0)
    nan_rows = np.flatnonzero(np.random.default_rng(3).random(130) < 0.4)
    mixed = S.soup(130, 4, nan_rows)
    out["nan_interleaved"] = (mixed[None], S.points(1025, 5, 6)[None], 1, 2.0)
    out["nan_compacted"] = (mixed[S.valid_rows(mixed)][None], S.points(1025, 5, 6)[None], 1, 2.0)
    out["cube"] = (S.cube()[None], S.cube_cloud()[None], 1, 2.0)
    out["tripled"] = (S.soup(130, 71)[None], tripled_cloud()[None], 1, 2.0)
    for name, ((F, fs), (P, ps)) in NAMED.items():
        out[name] = (S.soup(F, fs)[None], S.points(P, ps, 6)[None], 1, 2.0)
    out["degenerate"] = degenerate6() + (1, 2.0)
    return out


def swap12(coords, rows):
    c = np.array(coords, copy=True)
    c[rows] = c[rows][:, [0, 2, 1]]
    return c


def outward(coords):
    """(F,) the sign of (face normal . face centroid) of the valid faces of a mesh around the origin: +1 = away from the centre"""
    c = np.asarray(coords, np.float64)
    c = c[np.isfinite(c.reshape(len(c), 9)).all(1)]
    return np.sign(np.einsum("fc,fc->f", np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), c.mean(1)))


def orientation():
    """(coords (2, 12, 3, 3), cloud (1, 4096, 6)): the cube with a seeded random half of its faces flipped, and the same with its
    top two faces NaN (an open box), against the cube's cloud"""
    flipped = swap12(S.cube(), np.sort(np.random.default_rng(5).permutation(12)[:6]))
    box = flipped.copy()
    box[2:4] = np.nan                                                 # the quad z = +s
    return np.stack([flipped, box]), S.cube_cloud()[None]


STRIPS, STEP = 12, 8                            # 12 strips of 8 / 128 mesh units = 0.125 cloud units across the footprint [-0.75, 0.75]^2
DELTA = 8                                       # the flat mesh is lifted by 8 / 128 mesh units = 0.125 cloud units
AMPLITUDE = 8                                   # the accordion's ridges: 8 / 128 mesh units = 0.125 cloud units, a fold angle of 45 degrees


def _strips(z_of_edge):
    x = [-48 + STEP * i for i in range(STRIPS + 1)]
    faces = []
    for i in range(STRIPS):
        a, b, c, d = (x[i], -48, z_of_edge(i)), (x[i + 1], -48, z_of_edge(i + 1)), (x[i + 1], 48, z_of_edge(i + 1)), (x[i], 48, z_of_edge(i))
        faces += [(a, b, c), (a, c, d)]
    return (np.array(faces, np.float64) / 128.0).astype(np.float32)


def ranking():
    """(coords (2, 24, 3, 3), cloud (1, 2048, 6)): a flat square cloud z = 0 with normals +z; candidate 0 the flat mesh lifted by
    DELTA, candidate 1 an accordion over the same footprint whose edges alternate between z = 0 and z = AMPLITUDE.  Every cloud point
    is DELTA (0.125 cloud units) from the flat mesh, but a point at horizontal offset x from the nearest valley of the accordion is
    x / sqrt(2) from it: at most AMPLITUDE / sqrt(2) (0.088 cloud units), 0.044 on average, so the accordion wins on distance; its
    faces are tilted by 45 degrees, so its NC is sqrt(1/2) = 0.71 against 1."""
    rng = np.random.default_rng(9)
    cl = np.zeros((2048, 6), np.float32)
    cl[:, :2] = rng.uniform(-0.75, 0.75, (2048, 2)).astype(np.float32)
    cl[:, 5] = 1.0
    return np.stack([_strips(lambda i: DELTA), _strips(lambda i: AMPLITUDE * (i % 2))]), cl[None]
