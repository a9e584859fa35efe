"""Numpy restatement of the watertight kernels (meshanything_amd/csrc/watertight.hpp) that the watertight tests compare against.

* `band_udf`: the narrow-band unsigned distance in float64 -- the same band (index-space bounding boxes computed in float32 exactly
  as the kernel does, widened by 2 cells), the same closest-point-by-region distance; `brute_udf` evaluates every triangle at every
  grid point.
* `marching_cubes`: the library's own table (ma_mc_table, host only), the same emission order (vertices per grid point in x, y, z
  order; triangles in cell-linear order, table order inside a cell) and the same float32 interpolation.
Plus the mesh-property checks and the procedural meshes the tests share.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

BAND = 2
_TABLE = None


def mc_table():
    """(tris (256, 3 * max_tris) int8 edge ids, -1 padded; edges (12, 4) int8 = corner dx, dy, dz, axis; ntris (256,)) from the library."""
    global _TABLE
    if _TABLE is None:
        from meshanything_amd import _lib, build
        build.build(force=False, verbose=False)
        lib = _lib.load()
        m = C.c_int32()
        assert lib.ma_mc_table(None, None, C.byref(m)) == 0
        tris = np.zeros((256, 3 * m.value), np.int8)
        edges = np.zeros((12, 4), np.int8)
        assert lib.ma_mc_table(tris.ctypes.data, edges.ctypes.data, None) == 0
        ntris = (tris >= 0).sum(1) // 3
        _TABLE = tris, edges, ntris
    return _TABLE


# ---- distance --------------------------------------------------------------------------------------------------------------
FLAT_CELLS = 1.0 / 128.0            # csrc/watertight.hpp UDF_FLAT_CELLS: inradius (in cells) below which a face counts as its edges


def _dot(a, b):
    return (a * b).sum(-1)


def _seg(a, e):
    """|closest point of segment a .. a + e| (a relative to the query point), in the inputs' dtype."""
    l2 = _dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l2 > 0, -_dot(a, e) / np.where(l2 > 0, l2, 1), 0)
    t = np.clip(t, 0, 1).astype(a.dtype)
    q = a + t[:, None] * e
    return np.sqrt(_dot(q, q))


def tri_dist(A, B, C, p, flat):
    """The kernel's tri_dist, in the inputs' dtype (float64 for the reference, float32 to restate the kernel's arithmetic): vertices
    A, B, C and points p (N, 3).  Edges from the vertex coordinates, normal from the two shorter edges, a face with inradius <= flat
    taken as its edges; otherwise the plane distance when p projects inside."""
    e0, e1, e2 = B - A, C - B, A - C
    a, b, c = A - p, B - p, C - p
    dseg = np.minimum(_seg(a, e0), np.minimum(_seg(b, e1), _seg(c, e2)))
    l0, l1, l2 = _dot(e0, e0), _dot(e1, e1), _dot(e2, e2)
    n = np.where(((l0 >= l1) & (l0 >= l2))[:, None], np.cross(e1, e2), np.where((l1 >= l2)[:, None], np.cross(e2, e0), np.cross(e0, e1)))
    n2 = _dot(n, n)
    fp = np.asarray(flat, a.dtype) * (np.sqrt(l0) + np.sqrt(l1) + np.sqrt(l2))
    solid = n2 > fp * fp
    inside = solid & (_dot(np.cross(a, e0), n) >= 0) & (_dot(np.cross(b, e1), n) >= 0) & (_dot(np.cross(c, e2), n) >= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        face = np.abs(_dot(a, n)) / np.sqrt(n2)
    return np.where(inside, np.minimum(dseg, face), dseg)


def true_dist(A, B, C, p):
    """Point-triangle distance by another route, float64, no flatness rule: the least of the three segment distances and, when the
    barycentric coordinates of p's projection (2x2 Gram system, Cramer) are all >= 0, the distance to that projection."""
    A, B, C, p = (np.asarray(x, np.float64) for x in (A, B, C, p))
    u, v, w = B - A, C - A, p - A
    uu, uv, vv, wu, wv = _dot(u, u), _dot(u, v), _dot(v, v), _dot(w, u), _dot(w, v)
    det = uu * vv - uv * uv
    d = np.minimum(_seg(A - p, u), np.minimum(_seg(B - p, C - B), _seg(C - p, A - C)))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (vv * wu - uv * wv) / det
        t = (uu * wv - uv * wu) / det
        ok = (det > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
    q = A + np.where(ok, s, 0)[:, None] * u + np.where(ok, t, 0)[:, None] * v - p
    return np.where(ok, np.minimum(d, np.sqrt(_dot(q, q))), d)


def grid_points(idx, size):
    """Grid coordinates of integer indices, float32 like the kernel: i * (2 / size) - 1."""
    return idx.astype(np.float32) * np.float32(2.0 / size) - np.float32(1.0)


def band_boxes(verts32, faces, size):
    """Per triangle: inclusive index boxes lo (F, 3), hi (F, 3) of the band, float32 arithmetic as in udf_boxes_kernel."""
    g = (verts32[faces].astype(np.float32) + np.float32(1.0)) * np.float32(0.5 * size)       # (F, 3 corners, 3 axes)
    mn = np.clip(g.min(1), -4, size + 4)
    mx = np.clip(g.max(1), -4, size + 4)
    lo = np.maximum(0, np.floor(mn).astype(np.int64) - BAND)
    hi = np.minimum(size - 1, np.ceil(mx).astype(np.int64) + BAND)
    return lo, hi


def band_udf(verts32, faces, size, batch=1 << 21, dtype=np.float64):
    """The kernel's band unsigned distance (float64; dtype=np.float32 restates the kernel's own arithmetic): (size,) * 3, +inf outside
    every triangle's band box."""
    verts32 = np.asarray(verts32, np.float32)
    faces = np.asarray(faces, np.int64)
    v64 = verts32.astype(dtype)
    flat = np.float32(2.0 / size) * np.float32(FLAT_CELLS)
    lo, hi = band_boxes(verts32, faces, size)
    ext = hi - lo + 1
    counts = np.where((ext > 0).all(1), ext.prod(1), 0)
    starts = np.concatenate([[0], np.cumsum(counts)])
    field = np.full(size ** 3, np.inf)
    total = int(starts[-1])
    for s in range(0, total, batch):
        e = min(total, s + batch)
        pair = np.arange(s, e)
        t = np.searchsorted(starts, pair, side="right") - 1
        local = pair - starts[t]
        nz, ny = ext[t, 2], ext[t, 1]
        k = local % nz
        j = (local // nz) % ny
        i = local // (nz * ny)
        gi, gj, gk = lo[t, 0] + i, lo[t, 1] + j, lo[t, 2] + k
        p = np.stack([grid_points(gi, size), grid_points(gj, size), grid_points(gk, size)], -1).astype(dtype)
        tri = v64[faces[t]]
        d = tri_dist(tri[:, 0], tri[:, 1], tri[:, 2], p, flat).astype(np.float64)
        np.minimum.at(field, (gi * size + gj) * size + gk, d)
    return field.reshape(size, size, size)


def brute_udf(verts32, faces, size):
    """Distance from every grid point to the nearest triangle, float64, no band, by true_dist (not the kernel's route)."""
    v64 = np.asarray(verts32, np.float32).astype(np.float64)
    idx = np.arange(size)
    g = grid_points(idx, size).astype(np.float64)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    out = np.full(p.shape[0], np.inf)
    for f in np.asarray(faces, np.int64):
        a, b, c = (np.broadcast_to(x, p.shape) for x in v64[f])
        out = np.minimum(out, true_dist(a, b, c, p))
    return out.reshape(size, size, size)


# ---- marching cubes --------------------------------------------------------------------------------------------------------
_POP3 = np.array([0, 1, 1, 2, 1, 2, 2, 3], np.int64)


def marching_cubes(field, level):
    """(verts (V, 3) float32 in index space, tris (F, 3) int64) in the kernel's order and arithmetic."""
    tris_t, edges_t, ntris_t = mc_table()
    f = np.ascontiguousarray(field, np.float32)
    nx, ny, nz = f.shape
    lev = np.float32(level)
    up = f >= lev
    emask = np.zeros(f.shape, np.int64)
    emask[:-1, :, :] |= (up[:-1] != up[1:]).astype(np.int64)
    emask[:, :-1, :] |= (up[:, :-1] != up[:, 1:]).astype(np.int64) << 1
    emask[:, :, :-1] |= (up[:, :, :-1] != up[:, :, 1:]).astype(np.int64) << 2
    em = emask.ravel()
    vcount = _POP3[em]
    voff = np.concatenate([[0], np.cumsum(vcount)])
    nv = int(voff[-1])
    flat = f.ravel()
    strides = (ny * nz, nz, 1)
    verts = np.zeros((nv, 3), np.float32)
    for axis in range(3):
        p = np.flatnonzero((em >> axis) & 1)
        a, b = flat[p], flat[p + strides[axis]]
        with np.errstate(all="ignore"):
            t = np.where(~np.isfinite(a), np.float32(1), np.where(~np.isfinite(b), np.float32(0), (lev - a) / (b - a))).astype(np.float32)
        ijk = np.stack(np.unravel_index(p, f.shape), -1).astype(np.float32)
        ijk[:, axis] += t
        verts[voff[p] + _POP3[em[p] & ((1 << axis) - 1)]] = ijk
    # cube index of every cell (bit c = corner (c & 1, c >> 1 & 1, c >> 2 & 1) is above)
    ci = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        ci |= up[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci = ci.ravel()
    nt = ntris_t[ci]
    cells = np.flatnonzero(nt)
    rep = np.repeat(cells, nt[cells])
    first = np.concatenate([[0], np.cumsum(nt[cells])])[:-1]
    tri_in_cell = np.arange(rep.size) - np.repeat(first, nt[cells])
    cijk = np.stack(np.unravel_index(rep, (nx - 1, ny - 1, nz - 1)), -1)
    origin = (cijk[:, 0] * ny + cijk[:, 1]) * nz + cijk[:, 2]
    tris = np.zeros((rep.size, 3), np.int64)
    for c in range(3):
        e = tris_t[ci[rep], 3 * tri_in_cell + c].astype(np.int64)
        d = edges_t[e].astype(np.int64)
        owner = origin + d[:, 0] * strides[0] + d[:, 1] * strides[1] + d[:, 2]
        tris[:, c] = voff[owner] + _POP3[em[owner] & ((1 << d[:, 3]) - 1)]
    return verts, tris


# ---- mesh properties -------------------------------------------------------------------------------------------------------
def closed_and_oriented(tris):
    """(every undirected edge in exactly 2 triangles, every directed edge at most once) -- together: closed and consistently oriented."""
    t = np.asarray(tris, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    nvert = int(t.max()) + 1 if t.size else 1
    dk = d[:, 0] * nvert + d[:, 1]
    uk = np.minimum(d[:, 0], d[:, 1]) * nvert + np.maximum(d[:, 0], d[:, 1])
    _, ucount = np.unique(uk, return_counts=True)
    _, dcount = np.unique(dk, return_counts=True)
    return bool((ucount == 2).all()), bool((dcount == 1).all())


def components(tris):
    """Connected components of the triangles (sharing a vertex): a label per triangle."""
    t = np.asarray(tris, np.int64)
    parent = np.arange(int(t.max()) + 1)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in t:
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    roots = np.array([find(a) for a in t[:, 0]])
    return np.unique(roots, return_inverse=True)[1]


def euler(tris):
    t = np.asarray(tris, np.int64)
    d = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return np.unique(t).size - np.unique(d, axis=0).shape[0] + t.shape[0]


def face_normals(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


# ---- procedural meshes (vertices float64, faces int64) ------------------------------------------------------------------
def icosphere(subdiv=2, r=0.8):
    phi = (1 + 5 ** 0.5) / 2
    v = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
         (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def midp(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = midp(a, b), midp(b, c), midp(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * r, np.array(f, np.int64)


def open_box(s=0.7):
    """A unit-ish box without its top (+z) face: 10 triangles, an open surface."""
    v = np.array([[x, y, z] for z in (-s, s) for y in (-s, s) for x in (-s, s)], float)
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(f, np.int64)


def torus(n_major=32, n_minor=16, R=0.6, r=0.25):
    u = np.linspace(0, 2 * np.pi, n_major, endpoint=False)
    w = np.linspace(0, 2 * np.pi, n_minor, endpoint=False)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    f = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b = i * n_minor + j, ((i + 1) % n_major) * n_minor + j
            c, d = ((i + 1) % n_major) * n_minor + (j + 1) % n_minor, i * n_minor + (j + 1) % n_minor
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, np.int64)


def sliver_soup(n=60, seed=0):
    """Random thin triangles (width 1-5 % of their length) plus exactly degenerate ones: a repeated vertex (a segment), all three
    vertices equal (a point) and three collinear vertices."""
    rng = np.random.default_rng(seed)
    v, f = [], []
    for _ in range(n):
        a = rng.uniform(-0.8, 0.8, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        L = rng.uniform(0.1, 0.6)
        b = a + L * d
        side = np.cross(d, rng.normal(size=3))
        side /= np.linalg.norm(side)
        c = a + rng.uniform(0.2, 0.8) * L * d + rng.uniform(0.01, 0.05) * L * side
        k = len(v)
        v += [a, b, c]
        f.append((k, k + 1, k + 2))
    k = len(v)
    v += [[0.1, 0.2, 0.3], [0.5, -0.2, 0.1]]
    f += [(k, k + 1, k + 1)]                                   # a segment
    v += [[-0.3, 0.4, -0.5]]
    f += [(k + 2, k + 2, k + 2)]                               # a point
    v += [[-0.5, -0.5, 0.25], [0.0, -0.5, 0.25], [0.25, -0.5, 0.25]]
    f += [(k + 3, k + 4, k + 5)]                               # collinear
    return np.array(v, float), np.array(f, np.int64)


def spanning(seed=1):
    """A few triangles that span the whole grid and a small closed tetrahedron."""
    v = np.array([[-0.9, -0.9, -0.85], [0.9, -0.9, 0.1], [-0.9, 0.9, 0.85], [0.9, 0.9, -0.2], [0.0, -0.9, 0.9],
                  [0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [0.1, 0.1, 0.3]], float)
    f = np.array([[0, 1, 2], [1, 3, 2], [0, 4, 3], [5, 7, 6], [5, 6, 8], [5, 8, 7], [6, 7, 8]], np.int64)
    return v, f


def collinear(seed=2):
    """The open box plus zero-area faces in general position: 6 with three collinear vertices (the middle one first, last or
    between) and 2 near-collinear ones (one vertex 1e-6 off the line) -- T-junction fillers and the like from other tools."""
    rng = np.random.default_rng(seed)
    v, f = open_box()
    v, f = list(v), [tuple(t) for t in f]
    for i in range(8):
        a = rng.uniform(-0.5, 0.5, 3)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        s = [(0.0, 0.25, 0.4), (0.0, 0.4, 0.15), (0.3, 0.0, 0.45)][i % 3]
        pts = [a + si * u for si in s]
        if i >= 6:
            side = np.cross(u, rng.normal(size=3))
            pts[1] = pts[1] + 1e-6 * side / np.linalg.norm(side)
        k = len(v)
        v += pts
        f.append((k, k + 1, k + 2))
    return np.array(v, float), np.array(f, np.int64)


MESHES = {"icosphere": icosphere, "open_box": open_box, "torus": torus, "sliver_soup": sliver_soup, "spanning": spanning,
          "collinear": collinear}


def normalized32(v):
    """normalize_vertices(v)[0] as float32: what export_to_watertight uploads."""
    from meshanything_amd.watertight import normalize_vertices
    return normalize_vertices(np.asarray(v, np.float64))[0].astype(np.float32)


def write_obj(path, v, f):
    with open(path, "w") as fh:
        for p in v:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for t in f:
            fh.write(f"f {t[0] + 1} {t[1] + 1} {t[2] + 1}\n")
