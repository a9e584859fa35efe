"""Numpy restatement of the upsampling (meshanything_amd/csrc/pc_upsample.hpp, C ABI ma_op_pc_upsample, meshanything_amd/pc_upsample.py)
that the pc_upsample tests compare against, and the clouds they share.

* `frame_ref`: the in-plane axes u, v of a normal, float64, every operation rounded on its own as the header states them.
* `upsample_ref`: brute force.  Per seed the lattice candidates in float64, rounded once to float32; per candidate the float32 key
  (dx*dx + dy*dy) + dz*dz against ALL rows, no grid (numpy rounds every operation and fuses none), a NaN key as +inf; kept iff the seed
  is the first row in the order (key, index), which is what `argmin` returns.  The normals are an input, so every bit is determined: the
  kernel must give EQUAL xyz, seed and counts, order included.
* the clouds, and the grids every case is run over (`pc_smooth_ref.grids_for`).
"""
import functools
import math

import numpy as np

import pc_smooth_ref as SR

REPO = SR.REPO
LADDER = (2, 4, 8, 16, 32, 64)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def frame_ref(n):
    """n (3) -> (u (3), v (3)) as Python floats (IEEE float64, one rounding per operation)"""
    n = [float(x) for x in n]
    mag = [abs(x) for x in n]
    a = 0 if (mag[0] <= mag[1] and mag[0] <= mag[2]) else (1 if mag[1] <= mag[2] else 2)   # the smallest |n_a|, ties to the lowest axis
    u0 = [(1.0 if k == a else 0.0) - n[a] * n[k] for k in range(3)]
    length = math.sqrt((u0[0] * u0[0] + u0[1] * u0[1]) + u0[2] * u0[2])
    u = [x / length for x in u0]
    v = [n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]]
    return u, v


def lattice(m):
    """-> (a, b) int64 arrays: the slots in loop order, a outer and b inner, (0, 0) left out, a^2 + b^2 <= m^2"""
    a, b = np.meshgrid(np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    keep = ((a != 0) | (b != 0)) & (a * a + b * b <= m * m)
    return a[keep], b[keep]


def candidates_ref(q, n, step, m):
    """the seed at q (3) float32 with normal n -> (c (K, 3) float32, a, b) in loop order, non-finite candidates not yet dropped"""
    u, v = frame_ref(n)
    a, b = lattice(m)
    da, db = a.astype(np.float64) * step, b.astype(np.float64) * step
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.stack([np.float64(q[k]) + (da * u[k] + db * v[k]) for k in range(3)], 1)
        return p.astype(np.float32), a, b


def keys_ref(c, p):
    """c (K, 3), p (N, 3) float32 -> (K, N) float32, the key of ma_op_pc_knn, NaN -> +inf"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (c[:, None, k] - p[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return np.where(np.isnan(d), np.float32(np.inf), d)


def upsample_ref(cloud, normals, radius, m, active=None, with_ab=False):
    """cloud (N, >= 3) float32, normals (N, 3) float64 -> dict of xyz (T, 3) float32, seed (T) int32, counts (N) int32 (and, with_ab, the
    kept (seed, a, b) as a list of tuples)"""
    p = np.ascontiguousarray(np.asarray(cloud)[:, :3], np.float32)
    normals = np.asarray(normals, np.float64)
    N = p.shape[0]
    step = float(radius) / m                                         # what upsample_points passes
    xyz, seed, ab, counts = [], [], [], np.zeros(N, np.int32)
    for i in range(N):
        if (active is not None and not active[i]) or not np.isfinite(p[i]).all() or not np.isfinite(normals[i]).all():
            continue
        c, a, b = candidates_ref(p[i], normals[i], step, m)
        finite = np.isfinite(c).all(1)
        c, a, b = c[finite], a[finite], b[finite]
        kept = np.argmin(keys_ref(c, p), axis=1) == i                # argmin: the first index of the smallest key
        counts[i] = int(kept.sum())
        xyz.append(c[kept])
        seed.append(np.full(counts[i], i, np.int32))
        ab += [(i, int(x), int(y)) for x, y in zip(a[kept], b[kept])]
    out = {"xyz": np.concatenate(xyz, 0) if xyz else np.zeros((0, 3), np.float32), "seed": np.concatenate(seed) if seed else np.zeros(0, np.int32),
           "counts": counts}
    if with_ab:
        out["ab"] = ab
    return out


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def sphere(n=300, seed=0):
    """-> (xyz (n, 3) float32 on the unit sphere, normals (n, 3) float64 = the float32 position normalised in float64)"""
    g = np.random.default_rng(seed)
    p = unit(g.normal(size=(n, 3))).astype(np.float32)
    return p, unit(p)


@functools.lru_cache(maxsize=None)
def cube(per_face=64, per_edge=8):
    """the faces of [-1, 1]^3 with their own normals, and points ON the twelve edges with the diagonal normal between the two faces"""
    g = np.random.default_rng(1)
    pts, nrm = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = g.uniform(-0.95, 0.95, (per_face, 3))
            p[:, axis] = sign
            n = np.zeros((per_face, 3))
            n[:, axis] = sign
            pts.append(p)
            nrm.append(n)
    for a0 in range(3):
        for a1 in range(a0 + 1, 3):
            for s0 in (-1.0, 1.0):
                for s1 in (-1.0, 1.0):
                    p = g.uniform(-1.0, 1.0, (per_edge, 3))
                    p[:, a0], p[:, a1] = s0, s1
                    n = np.zeros((per_edge, 3))
                    n[:, a0], n[:, a1] = s0, s1
                    pts.append(p)
                    nrm.append(n)
    return np.concatenate(pts).astype(np.float32), unit(np.concatenate(nrm))


@functools.lru_cache(maxsize=None)
def sheets(side=12, gap=0.05):
    """two parallel jittered sheets z = 0 and z = gap, closer than the radius the case uses"""
    g = np.random.default_rng(2)
    i = np.arange(side, dtype=np.float64) / (side - 1) * 2 - 1
    flat = np.stack(np.meshgrid(i, i, indexing="ij"), -1).reshape(-1, 2)
    lo = np.concatenate([flat + g.normal(scale=0.01, size=flat.shape), np.zeros((flat.shape[0], 1))], 1)
    hi = np.concatenate([flat + g.normal(scale=0.01, size=flat.shape), np.full((flat.shape[0], 1), gap)], 1)
    p = np.concatenate([lo, hi]).astype(np.float32)
    return p, np.tile(np.array([[0.0, 0.0, 1.0]]), (p.shape[0], 1))


@functools.lru_cache(maxsize=None)
def scattered(n, seed=3):
    """n rows uniform in [-1, 1]^3 with random unit normals"""
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, (n, 3)).astype(np.float32), unit(g.normal(size=(n, 3)))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud (N, 3 | 6) float32, normals (N, 3) float64, radius, m, active (N) bool or None, grids).  Built once; nobody writes
    to the arrays."""
    out = {}
    p, n = sphere()
    noise = np.random.default_rng(4).uniform(-1, 1, p.shape).astype(np.float32)   # columns the kernel must not read
    out["sphere_ld3"] = (p, n, 0.3, 8, None, SR.grids_for(-1.1, 2.2, 0.3))
    out["sphere_ld6"] = (np.concatenate([p, noise], 1), n, 0.3, 3, None, SR.grids_for(-1.1, 2.2, 0.3))
    p, n = cube()
    some = np.arange(p.shape[0]) % 5 != 0                           # every fifth row seeds nothing but still owns its neighbourhood
    out["cube"] = (p, n, 0.25, 3, some, SR.grids_for(-1.1, 2.2, 0.25))
    p, n = sheets()
    out["sheets"] = (p, n, 0.2, 8, None, SR.grids_for(-1.1, 2.2, 0.2))
    p, n = sphere(100, seed=5)
    order = np.random.default_rng(6).permutation(300)
    out["duplicated"] = (np.concatenate([p] * 3)[order], np.concatenate([n] * 3)[order], 0.4, 3, None, SR.grids_for(-1.1, 2.2, 0.4))
    for N in (1, 257, 5000):                                        # one workgroup per seed, 256 per build workgroup, 1024 per scan tile
        p, n = scattered(N)
        r = float(min(0.5, 1.5 / np.cbrt(N)))
        grids = SR.grids_for(-1.1, 2.2, r)
        if N == 5000:
            grids = {k: grids[k] for k in ("auto", "odd")}
        out[f"n{N}_m1"] = (p, n, r, 1, None, grids)
    p, n = scattered(8, seed=7)
    out["n8_m64"] = (p, n, 1.0, 64, None, SR.grids_for(-1.1, 2.2, 1.0))
    p, n = sphere()
    out["inactive"] = (p, n, 0.3, 3, np.zeros(p.shape[0], bool), SR.grids_for(-1.1, 2.2, 0.3))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> upsample_ref of the case, computed once; nobody writes to it"""
    cloud, normals, radius, m, active, _ = cases()[name]
    return upsample_ref(cloud, normals, radius, m, active)


# ---- the input side --------------------------------------------------------------------------------------------------------------------
FILE_ROWS, FILE_RADIUS = 1500, 0.2                                  # spacing sqrt(4 pi / 1500) = 0.09: about 15 rows within the radius of each


@functools.lru_cache(maxsize=None)
def fibonacci(n):
    """-> (xyz (n, 3) float32, normals (n, 3) float64): the Fibonacci lattice on the unit sphere, evenly spaced, so that every row has a plane"""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return p, unit(p)


def file_rows(dtype, ld, n=FILE_ROWS):
    """a unit sphere of n rows as a file of that dtype; with 6 columns its normals"""
    p, true = fibonacci(n)
    if ld == 3:
        return p.astype(dtype)
    return np.concatenate([p.astype(np.float64), true], 1).astype(dtype)
