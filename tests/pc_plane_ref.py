"""Numpy restatement of the dominant-plane kernels (meshanything_amd/csrc/pc_plane.hpp, C ABI ma_op_pc_plane_score / ma_op_pc_plane_apply,
meshanything_amd/pc_plane.py) that the pc_plane tests compare against, and the clouds they share.

* `rhs_of`, `inliers_ref`: the inlier rule in float32, every product and sum a numpy operation of its own (numpy rounds each and fuses
  none): len2 = (nx*nx + ny*ny) + nz*nz, rhs = t2 * len2, s = (nx*dx + ny*dy) + nz*dz, inlier iff s*s <= rhs; a degenerate plane
  (!(len2 > 0) or rhs not finite) has none.
* `planes_ref`, `score_ref`: the plane of a row triple (a = p_i, n = (p_j - p_i) x (p_k - p_i), six zeros for an index outside [0, N)),
  the counts (-1 for a degenerate hypothesis) and best (greatest count, lowest index, -1 if all are degenerate).  The kernels must give
  EQUAL integers and planes.
* `moments_ref`: the ten float64 moments of the inliers about a, and the sum of the terms' magnitudes for the bound
  |got - want| <= n * 2^-52 * sum|term|.
* `remove_ref`: the loop of `pc_plane.remove_planes` over these, with its own draw and its own refit.
* `scene`: a sphere that stands on a table: what `--plane_threshold` is for.
"""
import functools

import numpy as np

import pc_normals_ref as PN

REPO = PN.REPO
SEED = 0x706c616e65
F32 = np.float32


def t2_of(threshold):
    t = F32(threshold)
    t2 = t * t
    assert t2.dtype == np.float32
    return t2


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def rhs_of(normals, threshold):
    """normals (..., 3) float32 -> (rhs (...) float32, degenerate (...) bool)"""
    n = np.asarray(normals, F32)
    with np.errstate(all="ignore"):
        len2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        rhs = t2_of(threshold) * len2
    assert rhs.dtype == np.float32
    return rhs, ~(len2 > 0) | ~np.isfinite(rhs)


def inliers_ref(xyz, planes, threshold):
    """xyz (N, >= 3), planes (H, 6) or (6) -> (H, N) or (N) bool"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], F32)
    pl = np.asarray(planes, F32)
    one = pl.ndim == 1
    pl = pl.reshape(-1, 6)
    rhs, deg = rhs_of(pl[:, 3:], threshold)
    with np.errstate(all="ignore"):
        dx = p[None, :, 0] - pl[:, None, 0]
        dy = p[None, :, 1] - pl[:, None, 1]
        dz = p[None, :, 2] - pl[:, None, 2]
        s = (pl[:, None, 3] * dx + pl[:, None, 4] * dy) + pl[:, None, 5] * dz
        assert s.dtype == np.float32
        inl = (s * s <= rhs[:, None]) & ~deg[:, None]                # a NaN or infinite s*s compares false
    return inl[0] if one else inl


def planes_ref(xyz, tri):
    """-> planes (H, 6) float32: (p_i, e1 x e2), six zeros where an index is outside [0, N)"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], F32)
    tri = np.asarray(tri, np.int64)
    ok = ((tri >= 0) & (tri < p.shape[0])).all(1)
    t = np.where(ok[:, None], tri, 0)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    out = np.concatenate([a, n], 1)
    assert out.dtype == np.float32
    out[~ok] = 0
    return out


def best_of(counts):
    counts = np.asarray(counts)
    return int(np.argmax(counts)) if (counts >= 0).any() else -1     # argmax: the first of the greatest


def score_ref(xyz, tri, threshold, chunk=128):
    """-> (planes (H, 6) float32, counts (H) int32, best int)"""
    planes = planes_ref(xyz, tri)
    _, deg = rhs_of(planes[:, 3:], threshold)
    counts = np.concatenate([inliers_ref(xyz, planes[h:h + chunk], threshold).sum(1) for h in range(0, planes.shape[0], chunk)]).astype(np.int32)
    counts[deg] = -1
    return planes, counts, best_of(counts)


def moments_ref(xyz, mask, a):
    """-> (moments (10) float64, sum|term| (10) float64) over the rows of mask with q = float64(p) - float64(a)"""
    q = np.asarray(xyz)[:, :3].astype(F32).astype(np.float64)[np.asarray(mask, bool)] - np.asarray(a, F32).astype(np.float64)[None, :]
    terms = np.stack([np.ones(q.shape[0]), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2], q[:, 1] * q[:, 1],
                      q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]], 1)
    return terms.sum(0), np.abs(terms).sum(0)


def moments_bound(xyz, mask, a):
    """the contract's bound per moment: n * 2^-52 * sum|term|"""
    return float(np.asarray(mask, bool).sum()) * 2.0 ** -52 * moments_ref(xyz, mask, a)[1]


def draw_ref(N, iters, round_):
    return np.random.Generator(np.random.PCG64([SEED, round_])).integers(0, N, (iters, 3)).astype(np.int32)


def fit_ref(moments, a):
    m = np.asarray(moments, np.float64)
    mean = m[1:4] / m[0]
    cov = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / m[0] - mean[:, None] * mean[None, :]
    w, v = np.linalg.eigh(cov)
    return (np.asarray(a, np.float64) + mean).astype(F32), v[:, int(np.argmin(w))].astype(F32)


def distance64(xyz, plane):
    """signed distance of every row to the plane, in float64 with a unit normal: the geometry the rule approximates"""
    pl = np.asarray(plane, np.float64)
    return (np.asarray(xyz)[:, :3].astype(np.float64) - pl[None, :3]) @ (pl[3:] / np.linalg.norm(pl[3:]))


def remove_ref(xyz, threshold, iters=1024, count=1, min_fraction=0.2):
    """-> (kept rows int64, [per removed plane: dict(plane, count, first, refit, gap)], stopped: bool): `pc_plane.remove_planes` restated.
    gap: the least | |distance64| - threshold | over the round's rows and both planes."""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], F32)
    kept = np.arange(p.shape[0], dtype=np.int64)
    found = []
    for r in range(count):
        rows = p[kept]
        if rows.shape[0] < 3:
            break
        planes, counts, best = score_ref(rows, draw_ref(rows.shape[0], iters, r), threshold)
        if best < 0 or counts[best] < min_fraction * rows.shape[0]:
            return kept, found, True
        first = planes[best]
        m0 = inliers_ref(rows, first, threshold)
        refit = np.concatenate(fit_ref(moments_ref(rows, m0, first[:3])[0], first[:3]))
        m1 = inliers_ref(rows, refit, threshold)
        gap = min(np.abs(np.abs(distance64(rows, pl)) - threshold).min() for pl in (first, refit))
        plane, mask = (refit, m1) if m1.sum() > m0.sum() else (first, m0)
        found.append({"plane": plane, "count": int(mask.sum()), "first": int(m0.sum()), "refit": int(m1.sum()), "gap": float(gap), "ties": int((counts == counts[best]).sum())})
        kept = kept[~mask]
    return kept, found, False


# ---- clouds -----------------------------------------------------------------------------------------------------------------------------
SCORE_N = (3, 63, 64, 65, 255, 256, 257, 1025, 2500)                 # around the wave, the workgroup and the 2 048-row tile
SCORE_H = (1, 63, 64, 65, 300)                                       # around the wave and the 256-hypothesis chunk
UNIFORM_T = 0.1


def uniform_cloud(N, ld, seed=0):
    return np.random.default_rng([seed, N, ld]).uniform(-1, 1, (N, ld)).astype(F32)


def uniform_triples(N, H, seed=0):
    """random triples; for H >= 63 with a repeated index, an index equal to N and a negative one mixed in; H = 1: rows 0, 1, 2"""
    tri = np.random.default_rng([seed, N, H, 1]).integers(0, N, (H, 3)).astype(np.int32)
    tri[0] = (0, 1, 2)
    if H >= 63:
        tri[5] = (tri[5, 0], tri[5, 0], tri[5, 2])
        tri[7] = (0, 1, N)
        tri[9] = (-1, 0, 1)
    return tri


@functools.lru_cache(maxsize=None)
def uniform_case(N, ld, H):
    """-> (cloud (N, ld), tri (H, 3), threshold, (planes, counts, best))"""
    cloud, tri = uniform_cloud(N, ld), uniform_triples(N, H)
    return cloud, tri, UNIFORM_T, score_ref(cloud, tri, UNIFORM_T)


LATTICE_T = 0.125


@functools.lru_cache(maxsize=None)
def lattice_case():
    """The 10 x 10 x 10 lattice of spacing 1/8, shuffled; hypotheses through three lattice points of one axis-aligned layer, e1 and e2 two
    steps long: n = 1/16 along the axis, len2 = 2^-8, and at threshold 1/8 rhs = 2^-14 = s*s EXACTLY for the rows of the two neighbouring
    layers: 300 inliers for an inner layer, 200 for an outer one.  With them collinear lattice triples, a repeated index and indices
    outside [0, N).  -> (cloud (1000, 3), tri, threshold, (planes, counts, best), expect (H) int32)"""
    g = np.random.default_rng(7)
    ijk = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)[g.permutation(1000)]
    cloud = (ijk / 8.0).astype(F32)
    row = {tuple(v): r for r, v in enumerate(ijk.tolist())}
    tri, expect = [], []
    for axis in range(3):
        u, v = [(1, 2), (2, 0), (0, 1)][axis]
        for layer in range(10):
            pts = []
            for du, dv in ((0, 0), (2, 0), (0, 2)):
                c = [0, 0, 0]
                c[axis], c[u], c[v] = layer, 3 + du, 4 + dv
                pts.append(row[tuple(c)])
            tri.append(pts)
            expect.append(300 if 0 < layer < 9 else 200)
    tri += [[row[(0, 0, 0)], row[(1, 1, 1)], row[(5, 5, 5)]], [row[(2, 0, 7)], row[(2, 4, 7)], row[(2, 9, 7)]], [17, 17, 40], [3, 4, 1000], [-5, 4, 6]]
    expect += [-1] * 5
    tri = np.array(tri, np.int32)
    return cloud, tri, LATTICE_T, score_ref(cloud, tri, LATTICE_T), np.array(expect, np.int32)


@functools.lru_cache(maxsize=None)
def twin_case():
    """2 500 rows, 1 500 of them with z = 0 exactly; the triple of three such rows stands at h = 10 AND h = 3 among random triples: both
    hold at least 1 500 rows, more than any other, and best must be 3.  -> (cloud, tri, threshold, (planes, counts, best))"""
    g = np.random.default_rng(11)
    cloud = g.uniform(-1, 1, (2500, 3)).astype(F32)
    perm = g.permutation(2500)
    flat = perm[:1500]
    cloud[flat, 2] = 0
    tri = perm[1500:][g.integers(0, 1000, (64, 3))].astype(np.int32)   # the other triples: rows off that plane
    tri[10] = tri[3] = flat[:3]
    return cloud, tri, 0.05, score_ref(cloud, tri, 0.05)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """every hypothesis degenerate: best = -1"""
    cloud = uniform_cloud(257, 3, seed=3)
    tri = np.array([[h, h, (h * 7) % 257] for h in range(70)] + [[0, 1, 257], [-1, 2, 3]], np.int32)
    return cloud, tri, UNIFORM_T, score_ref(cloud, tri, UNIFORM_T)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """a NaN row and an infinite row: never inliers, and the hypotheses through them are degenerate"""
    cloud = uniform_cloud(257, 6, seed=4)
    cloud[5, 1] = np.nan
    cloud[9, 0] = np.inf
    tri = uniform_triples(257, 65, seed=4)
    tri[2] = (5, 20, 30)
    tri[3] = (20, 9, 30)
    tri[4] = (20, 30, 9)
    return cloud, tri, 0.3, score_ref(cloud, tri, 0.3)


SCENE_T = 0.02
SCENE_TILT = 0.3
SCENE_SHIFT = (3.0, -2.0, 5.0)


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    """-> (xyz (M, 3) float32, normals (M, 3) float64, kind (M) int8: 0 = table, 1 = sphere): a table of 6 000 rows uniform in [-1, 1]^2
    with |z| <= 0.2 t, and 9 000 rows on a sphere of radius 0.4 that TOUCHES the plane z = 0; every row whose distance to that plane
    lies in (0.6 t, 1.6 t) is left out, so that a plane close to the true one decides every row with room to spare; then everything is
    tilted by 0.3 rad about the x axis, shifted by (3, -2, 5), permuted and cast to float32.  t = SCENE_T.  Nobody writes to it."""
    t = SCENE_T
    g = np.random.default_rng([seed, 16])
    table = np.concatenate([g.uniform(-1, 1, (6000, 2)), g.uniform(-0.2 * t, 0.2 * t, (6000, 1))], 1)
    d = g.normal(size=(9000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = d * 0.4 + [0.0, 0.0, 0.4]
    xyz = np.concatenate([table, sphere], 0)
    normals = np.concatenate([np.tile([0.0, 0.0, 1.0], (6000, 1)), d], 0)
    kind = np.concatenate([np.zeros(6000), np.ones(9000)]).astype(np.int8)
    dist = np.abs(xyz[:, 2])
    keep = ~((dist > 0.6 * t) & (dist < 1.6 * t))
    c, s = np.cos(SCENE_TILT), np.sin(SCENE_TILT)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    xyz, normals, kind = xyz[keep] @ rot.T + np.array(SCENE_SHIFT), normals[keep] @ rot.T, kind[keep]
    perm = g.permutation(xyz.shape[0])
    return xyz[perm].astype(F32), normals[perm].copy(), kind[perm].copy()


@functools.lru_cache(maxsize=None)
def scene_reference(seed=0, min_fraction=0.2):
    """remove_ref of the scene at the defaults of the command line"""
    return remove_ref(scene(seed)[0], SCENE_T, 1024, 1, min_fraction)
