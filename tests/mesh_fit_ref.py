"""What the mesh-fit tests compare against (csrc/mesh_fit.hpp, meshanything_amd/mesh_fit.py).  Test infrastructure only.

(a) `pairs_ref` / `step_ref` / `fit_ref`: the DEFINITION in float64 by another route than the kernel's: the closest point of a triangle
    by Voronoi regions (Ericson, Real-Time Collision Detection 5.1.5), the admissibility rules from their wording (inradius = 2 area /
    perimeter), the argmin over faces, DENSE 3V x 3V normal equations accumulated point by point and `numpy.linalg.solve`.
(b) `pairs_f32`: the kernel's pairing and sums restated in float32 numpy, operation by operation in the kernel's order, with the int64
    2^-32 fixed-point sums.  The GPU test demands equality with it, bit for bit.
Plus the crafted inputs both test files share.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

F32 = np.float32
FLAT = 2.0 ** -20
STEP = 2.0 / 128.0                    # one lattice step in cloud units at the default mesh_scale
NSUM = 48
KL = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# ---- (a) float64, another route ------------------------------------------------------------------------------------------------
def closest_voronoi(A, B, C, p):
    """Closest point of triangle A, B, C (3,) to every p (N, 3) by Voronoi regions, float64: barycentric weights (N, 3)."""
    ab, ac, ap = B - A, C - A, p - A
    d1, d2 = ap @ ab, ap @ ac
    bp = p - B
    d3, d4 = bp @ ab, bp @ ac
    cp = p - C
    d5, d6 = cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    w = np.zeros((p.shape[0], 3))
    done = np.zeros(p.shape[0], bool)

    def put(mask, w0, w1, w2):
        m = mask & ~done
        w[m] = np.stack([np.broadcast_to(w0, m.shape)[m], np.broadcast_to(w1, m.shape)[m], np.broadcast_to(w2, m.shape)[m]], -1)
        done[m] = True
    with np.errstate(divide="ignore", invalid="ignore"):
        put((d1 <= 0) & (d2 <= 0), 1.0, 0.0, 0.0)
        put((d3 >= 0) & (d4 <= d3), 0.0, 1.0, 0.0)
        v = d1 / (d1 - d3)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1 - v, v, 0.0)
        put((d6 >= 0) & (d5 <= d6), 0.0, 0.0, 1.0)
        u = d2 / (d2 - d6)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), 1 - u, 0.0, u)
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 0.0, 1 - t, t)
        den = va + vb + vc
        put(np.ones_like(done), va / den, vb / den, vc / den)
    return w


def admissible_ref(verts, faces, flat=FLAT):
    """(M,) bool and the unit normals (M, 3), float64: distinct indices and inradius = 2 area / perimeter above flat."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(B - A, C - A)
    twice_area = np.linalg.norm(n, axis=1)
    per = np.linalg.norm(B - A, axis=1) + np.linalg.norm(C - B, axis=1) + np.linalg.norm(A - C, axis=1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = distinct & (per > 0) & (twice_area / np.where(per > 0, per, 1) > flat)
        nh = n / np.where(twice_area > 0, twice_area, 1)[:, None]
    return ok, nh


def pairs_ref(verts, faces, cloud, dist, min_cos=0.0, flat=FLAT):
    """The pairing by definition, float64: dict(face (P,) int, -1 = unpaired; w (P, 3); c (P, 3) the nearest point; r2; s; gap (P,) =
    the squared-distance margin to the runner-up face, +inf without one)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    cl = np.asarray(cloud, np.float64)
    p, m = cl[:, :3], cl[:, 3:6]
    P = p.shape[0]
    ok, nh = admissible_ref(v, f, flat)
    best, second = np.full(P, np.inf), np.full(P, np.inf)
    face, w = np.full(P, -1, np.int64), np.zeros((P, 3))
    live = (m * m).sum(1) > 0
    for i in np.flatnonzero(ok):
        A, B, C = v[f[i]]
        wi = closest_voronoi(A, B, C, p)
        c = wi @ np.stack([A, B, C])
        d2 = ((p - c) ** 2).sum(1)
        cand = live if min_cos <= 0 else live & (np.abs(m @ nh[i]) >= min_cos)
        d2 = np.where(cand, d2, np.inf)
        better = d2 < best
        second = np.where(better, best, np.minimum(second, d2))
        best = np.where(better, d2, best)
        face[better] = i
        w[better] = wi[better]
    paired = (face >= 0) & (best <= float(dist) ** 2)
    face = np.where(paired, face, -1)
    w = np.where(paired[:, None], w, 0.0)
    tri = v[f[np.maximum(face, 0)]]
    c = np.einsum("pk,pka->pa", w, tri)
    r = np.where(paired[:, None], p - c, 0.0)
    gap = np.where(np.isfinite(second), second - np.where(np.isfinite(best), best, 0.0), np.inf)
    return {"face": face, "w": w, "c": c, "r2": (r * r).sum(1), "s": (m * r).sum(1), "gap": gap, "best": best}


def dense_system(pr, faces, cloud, V, stiffness):
    """(3V, 3V) matrix and (3V,) right-hand side of the damped point-to-plane normal equations, accumulated point by point."""
    f = np.asarray(faces, np.int64)
    m = np.asarray(cloud, np.float64)[:, 3:6]
    H, g = stiffness * np.eye(3 * V), np.zeros(3 * V)
    for q in np.flatnonzero(pr["face"] >= 0):
        cols = (3 * f[pr["face"][q]][:, None] + np.arange(3)[None]).reshape(-1)
        j = (pr["w"][q][:, None] * m[q][None]).reshape(-1)         # d(m . c) / d(vertex k, axis a) = w_k m_a
        H[np.ix_(cols, cols)] += np.outer(j, j)
        g[cols] += j * pr["s"][q]
    return H, g


def step_ref(verts, faces, cloud, dist, stiffness=1.0, min_cos=0.0):
    pr = pairs_ref(verts, faces, cloud, dist, min_cos)
    H, g = dense_system(pr, faces, cloud, len(verts), stiffness)
    return np.linalg.solve(H, g).reshape(-1, 3), pr


def fit_ref(verts, faces, cloud, iters, dist=4.0, max_move=2.0, stiffness=1.0, min_cos=0.0, scale=2.0):
    """The whole fit by (a): verts in MESH units, dist and max_move in lattice steps -> (verts' in mesh units, float64; per-iteration
    list of (paired share, rms of s, largest move))."""
    step = scale / 128.0
    x0 = np.asarray(verts, np.float64) * scale
    x, its = x0.copy(), []
    for _ in range(iters):
        delta, pr = step_ref(x, faces, cloud, dist * step, stiffness, min_cos)
        n = int((pr["face"] >= 0).sum())
        d = x + delta - x0
        ln = np.linalg.norm(d, axis=1)
        d *= np.where(ln > max_move * step, max_move * step / np.where(ln > 0, ln, 1), 1.0)[:, None]
        move = float(np.linalg.norm(x0 + d - x, axis=1).max())
        x = x0 + d
        its.append((n / len(pr["face"]), float(np.sqrt((pr["s"] ** 2).sum() / n)) if n else 0.0, move))
        if move <= 2.0 ** -20:
            break
    return x / scale, its


# ---- (b) the kernel in float32 numpy -----------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def prep_f32(verts32, faces, flat=FLAT):
    """prep_face for every face: (admissible (M,), nh (M, 3) float32)."""
    v = np.asarray(verts32, F32)
    f = np.asarray(faces, np.int64)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e0, e1, e2 = B - A, C - B, A - C
    l0, l1, l2 = _dot(e0, e0), _dot(e1, e1), _dot(e2, e2)
    n = np.where(((l0 >= l1) & (l0 >= l2))[:, None], _cross(e1, e2), np.where((l1 >= l2)[:, None], _cross(e2, e0), _cross(e0, e1)))
    n2 = _dot(n, n)
    fp = F32(flat) * ((np.sqrt(l0) + np.sqrt(l1)) + np.sqrt(l2))
    ok = (n2 > fp * fp) & (n2 < np.inf) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = n / np.sqrt(n2)[:, None]
    assert nh.dtype == F32
    return ok, nh


def _edge(v, e):
    l = _dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(l > 0, -_dot(v, e) / l, F32(0))
    u = np.minimum(np.maximum(u, F32(0)), F32(1)).astype(F32)
    q = v + u[:, None] * e
    return _dot(q, q), u, q


def _pair_face_f32(A, B, C, nh, p):
    """pair_face for one face against every point: (d2, w (P, 3), r (P, 3)), float32."""
    e0, e1, e2 = (B - A)[None], (C - B)[None], (A - C)[None]
    a, b, c = A[None] - p, B[None] - p, C[None] - p
    s0, s1, s2 = _dot(_cross(a, e0), nh[None]), _dot(_cross(b, e1), nh[None]), _dot(_cross(c, e2), nh[None])
    S = (s0 + s1) + s2
    inside = (s0 >= 0) & (s1 >= 0) & (s2 >= 0) & (S > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = np.stack([s1 / S, s2 / S, s0 / S], -1)
    ri = -((wi[:, 0:1] * a + wi[:, 1:2] * b) + wi[:, 2:3] * c)
    di = _dot(ri, ri)
    d0, t0, q0 = _edge(a, np.broadcast_to(e0, a.shape))
    d1, t1, q1 = _edge(b, np.broadcast_to(e1, a.shape))
    d2, t2, q2 = _edge(c, np.broadcast_to(e2, a.shape))
    z, one = np.zeros_like(t0), F32(1)
    d, q, w = d0, q0, np.stack([one - t0, t0, z], -1)
    m1 = d1 < d
    d, q, w = np.where(m1, d1, d), np.where(m1[:, None], q1, q), np.where(m1[:, None], np.stack([z, one - t1, t1], -1), w)
    m2 = d2 < d
    d, q, w = np.where(m2, d2, d), np.where(m2[:, None], q2, q), np.where(m2[:, None], np.stack([t2, z, one - t2], -1), w)
    out = np.where(inside, di, d), np.where(inside[:, None], wi, w), np.where(inside[:, None], ri, -q)
    assert all(x.dtype == F32 for x in out)
    return out


def fixed32(x):
    return np.rint(np.asarray(x, F32).astype(np.float64) * 4294967296.0).astype(np.int64)


def pairs_f32(verts32, faces, cloud, dist, min_cos=0.0, flat=FLAT):
    """pair_kernel and sum_kernel: dict(face (P,) int32, w (P, 3), s, r2 float32, sums (M, 48) int64).  cloud: float16 or float32."""
    v = np.asarray(verts32, F32)
    f = np.asarray(faces, np.int64)
    cl = np.asarray(cloud).astype(F32)
    p, m = np.ascontiguousarray(cl[:, :3]), np.ascontiguousarray(cl[:, 3:6])
    P, M = p.shape[0], f.shape[0]
    ok, nh = prep_f32(v, f, flat)
    live = _dot(m, m) > 0
    best, bs = np.full(P, np.inf, F32), np.zeros(P, F32)
    bf, bw = np.full(P, -1, np.int32), np.zeros((P, 3), F32)
    for i in np.flatnonzero(ok):
        d2, w, r = _pair_face_f32(v[f[i, 0]], v[f[i, 1]], v[f[i, 2]], nh[i], p)
        cand = live & (d2 < best)
        if min_cos > 0:
            cand &= ~(np.abs(_dot(nh[i][None], m)) < F32(min_cos))
        best = np.where(cand, d2, best)
        bf[cand] = i
        bw[cand] = w[cand]
        bs[cand] = _dot(m, r)[cand]
    paired = (bf >= 0) & (best <= F32(dist) * F32(dist))
    face = np.where(paired, bf, -1).astype(np.int32)
    w = np.where(paired[:, None], bw, F32(0))
    s, r2 = np.where(paired, bs, F32(0)), np.where(paired, best, F32(0))
    sums = np.zeros((M, NSUM), np.int64)
    q = np.flatnonzero(paired)
    terms = np.zeros((q.size, NSUM), np.int64)
    terms[:, 0] = 1
    terms[:, 1], terms[:, 2] = fixed32(s[q] * s[q]), fixed32(r2[q])
    for k in range(3):
        ws = w[q, k] * s[q]
        for a in range(3):
            terms[:, 3 + 3 * k + a] = fixed32(ws * m[q, a])
    for i, (k, l) in enumerate(KL):
        ww = w[q, k] * w[q, l]
        for j, (a, c) in enumerate(KL):
            terms[:, 12 + 6 * i + j] = fixed32(ww * (m[q, a] * m[q, c]))
    np.add.at(sums, face[q], terms)
    return {"face": face, "w": w.astype(F32), "s": s.astype(F32), "r2": r2.astype(F32), "sums": sums}


# ---- crafted inputs ------------------------------------------------------------------------------------------------------------------
def cube_mesh(half=0.4):
    """(verts (8, 3) float64, faces (12, 3)): merged vertices, outward winding."""
    v = np.array([[x, y, z] for z in (-half, half) for y in (-half, half) for x in (-half, half)], np.float64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return v, np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)


def cube_cloud(P=4096, half=0.4, seed=0, dtype=np.float32, skip_side=None):
    """(P, 6): exact points of the cube's surface with their outward normals; skip_side = (axis, sign): no points on that side."""
    rng = np.random.default_rng(seed)
    axis, sign = rng.integers(0, 3, P), rng.integers(0, 2, P) * 2 - 1
    if skip_side is not None:
        hit = (axis == skip_side[0]) & (sign == skip_side[1])
        sign = np.where(hit, -sign, sign)
    out = np.zeros((P, 6))
    out[:, :3] = rng.uniform(-half, half, (P, 3))
    out[np.arange(P), axis] = sign * half
    out[np.arange(P), 3 + axis] = sign
    return out.astype(dtype)


def jittered_cube(seed=1):
    """The issue's case in MESH units (cloud units / 2): the cube of half-extent 0.4 cloud units, every vertex moved by up to one
    lattice step per axis; float32 as the detokenizer's output is."""
    v, f = cube_mesh()
    rng = np.random.default_rng(seed)
    return ((v + rng.uniform(-STEP, STEP, v.shape)) / 2.0).astype(F32), f


def pulled_cube(steps=6.0):
    """The exact cube with vertex 7 (+,+,+) pulled `steps` lattice steps outward along the diagonal; mesh units, float32."""
    v, f = cube_mesh()
    v[7] += steps * STEP / np.sqrt(3.0)
    return (v / 2.0).astype(F32), f


def fin_cube():
    """The jittered cube plus a fin: one more face on the edge 6-7 (the top's y = +half edge) reaching 0.2 cloud units up and out, where
    the cloud has no points; its apex (vertex 8) has no support."""
    v, f = jittered_cube()
    apex = np.array([[0.0, 0.3, 0.3]], F32)                          # mesh units: (0, 0.6, 0.6) in cloud units
    return np.concatenate([v, apex]), np.concatenate([f, [[6, 7, 8]]])


def soup(M, P, seed, dist=0.05, f16=False):
    """A soup for the kernel shapes, CLOUD units: M faces of which some repeat an index, have zero area or are slivers; P points, most
    near a face, with unit-ish normals; one zero normal when P > 2.  -> (verts32 (3M, 3), faces (M, 3), cloud (P, 6), dist)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.45, 0.45, (M, 3))
    tri = a[:, None] + rng.uniform(-0.12, 0.12, (M, 3, 3))
    tri[:, 0] = a
    faces = np.arange(3 * M).reshape(M, 3)
    for i in range(M):
        kind = i % 11 if M > 4 else -1
        if kind == 3:
            faces[i, 2] = faces[i, 0]                                    # repeats a vertex index
        elif kind == 5:
            tri[i, 2] = 0.5 * (tri[i, 0] + tri[i, 1])                   # zero area (collinear up to rounding)
        elif kind == 7:
            tri[i, 2] = 0.3 * tri[i, 0] + 0.7 * tri[i, 1] + 2e-4 * rng.normal(size=3)   # a sliver, well above the flatness rule
        elif kind == 9:
            tri[i, 1] = tri[i, 0]                                        # two equal vertices under distinct indices
    v32 = tri.reshape(-1, 3).astype(F32)
    on = rng.integers(0, M, P)
    w = rng.dirichlet([1, 1, 1], P)
    t = v32.astype(np.float64)[faces[on]]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 1e-9, n / np.where(ln > 1e-9, ln, 1), [0.0, 0.0, 1.0])
    pts = np.einsum("pk,pka->pa", w, t) + n * rng.uniform(-1.4 * dist, 1.4 * dist, (P, 1))
    nr = n + 0.3 * rng.normal(size=(P, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    cloud = np.concatenate([pts, nr], 1)
    if P > 2:
        cloud[P // 2, 3:] = 0.0                                          # a zero normal pairs with nothing
    return v32, faces, cloud.astype(np.float16 if f16 else F32), dist


def quad_case(P=63):
    """Two faces sharing the edge (0,0,0)-(1/4,1/4,0) of a square in z = 0, with points whose answers are known by hand: [0] over the
    shared edge and [1] over a shared vertex (both faces at the same distance: face 0 wins), [2] just inside and [3] just outside dist
    (0.0625 = 4 steps; heights 0.0625 and 0.0625 + 2^-20, exact in float32), [4] a zero normal; the rest random near the square."""
    v32 = np.array([[0, 0, 0], [0.25, 0, 0], [0.25, 0.25, 0], [0, 0.25, 0]], F32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-0.05, 0.3, (P, 2)), rng.uniform(-0.07, 0.07, (P, 1))], 1)
    nrm = np.tile([0.0, 0.0, 1.0], (P, 1))
    pts[0] = [0.125, 0.125, 0.03125]
    pts[1] = [0.0, 0.0, 0.03125]
    pts[2] = [0.1875, 0.0625, 0.0625]
    pts[3] = [0.1875, 0.0625, 0.0625 + 2.0 ** -20]
    pts[4] = [0.0625, 0.1875, 0.01]
    nrm[4] = 0.0
    return v32, faces, np.concatenate([pts, nrm], 1).astype(F32), 0.0625


def kernel_cases():
    """name -> (verts32 in cloud units, faces, cloud, dist, min_cos): M around the 256-face tile, P around the wave and the block."""
    c = {}
    c["m1_p1"] = soup(1, 1, 10) + (0.0,)
    c["quad_p63"] = quad_case(63) + (0.0,)
    c["m2_p64_cos"] = soup(2, 64, 11) + (0.5,)
    c["m255_p65"] = soup(255, 65, 12) + (0.0,)
    c["m256_p257_f16"] = soup(256, 257, 13, f16=True) + (0.0,)
    c["m257_p257_cos"] = soup(257, 257, 14) + (0.7,)
    c["m600_p4096"] = soup(600, 4096, 15) + (0.0,)
    c["m3_p262145"] = soup(3, (1 << 18) + 1, 17) + (0.0,)          # one point past a chunk of the sum pass: two workgroups per face
    v, f, cl, d = soup(257, 65, 16)
    cl = cl.copy()
    cl[:, :3] += 3.0                                                 # nowhere near the mesh: nothing pairs, every sum is zero
    c["unpaired"] = (v, f, cl, d, 0.0)
    jv, jf = jittered_cube()
    c["cube_p4096"] = ((jv * F32(2.0)).astype(F32), jf, cube_cloud(), 4 * STEP, 0.0)
    return c


def deviation(b, a, verts, faces):
    """The largest deviation of a float32 result `b` (pairs_f32's dict, or the kernel's under the same keys) from (a) = pairs_ref's dict
    over the points both pair with the same face: per point the largest of the differences in s, in r2 and in the nearest point c =
    sum_k w_k v_k (the weights themselves are ill-conditioned on a sliver; the point they name is not); and the indices of the points
    whose faces differ."""
    same = (b["face"] == a["face"])
    both = same & (a["face"] >= 0)
    dev = 0.0
    if both.any():
        tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[a["face"][both]]]
        cb = np.einsum("pk,pka->pa", b["w"][both].astype(np.float64), tri)
        dev = max(float(np.abs(b["s"][both] - a["s"][both]).max()), float(np.abs(b["r2"][both] - a["r2"][both]).max()),
                  float(np.abs(cb - a["c"][both]).max()))
    return dev, np.flatnonzero(~same)


def shifted_cloud(steps=10.0):
    """cube_cloud() with every point moved `steps` lattice steps off the surface along its own normal.  (A rigid translation cannot
    unpair the cloud of a closed cube: the sides parallel to it slide in their own planes and stay at distance 0.)"""
    cl = cube_cloud().astype(np.float64)
    cl[:, :3] += steps * STEP * cl[:, 3:]
    return cl.astype(F32)


def open_cube():
    """The jittered cube without its two +z faces (faces 2 and 3), against the full cube_cloud(): a cloud side the mesh does not cover."""
    v, f = jittered_cube()
    return v, np.delete(f, [2, 3], axis=0)


_FIGURES = None


def figures():
    """The yardstick of the GPU test: the largest deviation of (b) from (a) on kernel_cases() -> (per point, per face, mismatches).
    Per point: deviation()'s figure.  Per face: the largest difference of a sum of sums_ref() from (b)'s, divided by the face's count,
    over the faces none of whose points are paired differently.  mismatches: {case: [(point, face of a, face of b, gap of a)]}."""
    global _FIGURES
    if _FIGURES is None:
        pt, fc, mism = 0.0, 0.0, {}
        for name, (v, f, cl, d, mc) in kernel_cases().items():
            cl32 = np.asarray(cl).astype(F32)
            b, a = pairs_f32(v, f, cl, d, mc), pairs_ref(v, f, cl32, d, mc)
            dp, df, diff = compare(b, a, v, f, cl32)
            pt, fc = max(pt, dp), max(fc, df)
            mism[name] = [(int(q), int(a["face"][q]), int(b["face"][q]), float(a["gap"][q])) for q in diff]
        _FIGURES = pt, fc, mism
    return _FIGURES


def compare(b, a, verts, faces, cloud32):
    """A float32 result b (keys face, w, s, r2, sums) against (a): (per-point deviation, per-face deviation, differently paired points)."""
    dp, diff = deviation(b, a, verts, faces)
    sa, sb = sums_ref(a, faces, cloud32), sums_as_float(b["sums"])
    clean = np.ones(len(sa), bool)
    for q in diff:
        for x in (a["face"][q], b["face"][q]):
            if x >= 0:
                clean[x] = False
    assert np.array_equal(sa[clean, 0], sb[clean, 0])
    df = float((np.abs(sa - sb) / np.maximum(sa[:, :1], 1.0))[clean].max()) if clean.any() else 0.0
    return dp, df, diff


def sums_as_float(sums):
    q = np.asarray(sums, np.int64)
    return np.concatenate([q[:, :1].astype(np.float64), q[:, 1:].astype(np.float64) / 4294967296.0], 1)


def sums_ref(pr, faces, cloud):
    """(a)'s per-face sums in the kernel's layout, float64 (M, 48)."""
    f = np.asarray(faces, np.int64)
    m = np.asarray(cloud, np.float64)[:, 3:6]
    out = np.zeros((f.shape[0], NSUM))
    q = np.flatnonzero(pr["face"] >= 0)
    w, s = pr["w"][q], pr["s"][q]
    t = np.zeros((q.size, NSUM))
    t[:, 0], t[:, 1], t[:, 2] = 1, s * s, pr["r2"][q]
    for k in range(3):
        for a in range(3):
            t[:, 3 + 3 * k + a] = w[:, k] * s * m[q, a]
    for i, (k, l) in enumerate(KL):
        for j, (a, c) in enumerate(KL):
            t[:, 12 + 6 * i + j] = w[:, k] * w[:, l] * m[q, a] * m[q, c]
    np.add.at(out, pr["face"][q], t)
    return out
