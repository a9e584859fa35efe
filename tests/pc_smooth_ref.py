"""Numpy restatement of the moving-least-squares smoothing (meshanything_amd/csrc/pc_smooth.hpp, C ABI ma_op_pc_smooth,
meshanything_amd/pc_smooth.py) that the pc_smooth tests compare against, and the clouds they share.

* `count_ref`: chunked brute force with the float32 key of `pc_cluster_ref.edges_ref`, (dx*dx + dy*dy) + dz*dz (numpy rounds every
  operation and fuses none): per row the number of rows, itself included, with d <= r2, r2 = fl32(fl32(radius) * fl32(radius)).  The
  kernel must give EQUAL counts.
* `smooth_ref`: the same key, the weights and the ten moments in float64 exactly as the header states them (every term is the kernel's
  bit for bit; a row that is no neighbour enters the sums as an exact 0), `np.linalg.eigh`, the sign rule of `pc_normals_ref`, the
  projection.  `perm` sums over the rows in another order: `smooth_ref(..., perm=shuffle(N))` is the second restatement, and the spread
  between the two on the same cloud measures what float64 resolves there; the GPU test derives its tolerance from it.
* the clouds: a unit sphere and the surface of the cube [-1, 1]^3, jittered with sigma 0.01, an integer lattice, a tripled cloud, and
  the grids every case is smoothed over.
"""
import functools

import numpy as np

import pc_cluster_ref as CR
import pc_normals_ref as PN

REPO = PN.REPO
MIN_COUNT = 6                                                        # pc_smooth.DEFAULT_MIN_COUNT
SIGMA = 0.01
SPHERE_RADIUS, CUBE_RADIUS = 0.2, 0.25
COUNT_N = (1, 2, 6, 255, 256, 257, 1025, 3000)                       # around the 256-query workgroup
GAP = 0.05


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _key(q, p):
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return dx, dy, dz, d


def count_ref(xyz, radius, chunk=512):
    """-> (N) int32: the rows within the radius of every row, itself included; a NaN key is not a neighbour"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    r2 = CR.r2_of(radius)
    out = np.empty(p.shape[0], np.int32)
    for i0 in range(0, p.shape[0], chunk):
        out[i0:i0 + chunk] = (_key(p[i0:i0 + chunk], p)[3] <= r2).sum(1)
    return out


def smooth_ref(xyz, radius, min_count=MIN_COUNT, perm=None, chunk=512):
    """xyz (N, >= 3) -> dict of moved (N, 3), normals (N, 3), eigvals (N, 3) float64 and count (N) int32.  perm: the order (a permutation
    of the rows) in which the neighbours enter the sums, None = the row order."""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    N = p.shape[0]
    r2 = CR.r2_of(radius)
    other = p if perm is None else p[np.asarray(perm)]
    count, same = np.empty(N, np.int32), np.empty(N, bool)
    S0, S1, S2 = np.empty(N), np.empty((N, 3)), np.empty((N, 3, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i0 in range(0, N, chunk):
            sl = slice(i0, i0 + chunk)
            dx, dy, dz, d = _key(p[sl], other)
            near = d <= r2
            count[sl] = near.sum(1)
            same[sl] = ~(near & ((dx != 0) | (dy != 0) | (dz != 0))).any(1)
            s = d.astype(np.float64) / np.float64(r2)
            u = 1.0 - s
            w = np.where(near, (u * u) * u, 0.0)
            e = [np.where(near, v, 0).astype(np.float64) for v in (dx, dy, dz)]   # (0 * a non-finite difference would be NaN)
            S0[sl] = w.sum(1)
            for a in range(3):
                we = w * e[a]
                S1[sl, a] = we.sum(1)
                for b in range(a, 3):
                    S2[sl, a, b] = S2[sl, b, a] = (we * e[b]).sum(1)
        mu = S1 / S0[:, None]
        C = S2 / S0[:, None, None] - mu[:, :, None] * mu[:, None, :]
        stays = (count < min_count) | same | ~np.isfinite(C).all((1, 2))
        C[stays] = np.eye(3)
        lam, vec = np.linalg.eigh(C)
        n = PN.sign_rule(vec[:, :, 0])
        t = (mu[:, 0] * n[:, 0] + mu[:, 1] * n[:, 1]) + mu[:, 2] * n[:, 2]
        q = p.astype(np.float64)
        moved = q - t[:, None] * n
        stays |= ~(np.isfinite(moved).all(1) & np.isfinite(n).all(1) & np.isfinite(lam).all(1))
    moved[stays], n[stays], lam[stays] = q[stays], (0.0, 0.0, 1.0), 0.0
    return {"moved": moved, "normals": n, "eigvals": lam, "count": count}


def shuffle(N, seed=7):
    return np.random.default_rng(seed).permutation(N)


def deviations(got, want, radius):
    """-> (|moved - want| / radius, the sine of the angle between the normals, max |eigenvalue - want| / want's largest), each (N)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        lam = np.abs(got["eigvals"] - want["eigvals"]).max(1) / want["eigvals"][:, 2]
    return np.linalg.norm(got["moved"] - want["moved"], axis=1) / radius, PN.sine(got["normals"], want["normals"]), lam


def well_posed(want, min_count=MIN_COUNT):
    """the rows whose normal float64 resolves: enough neighbours and the two smallest eigenvalues apart"""
    return (want["count"] >= min_count) & (PN.gap_ratio(want["eigvals"]) >= GAP)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_sphere(n=3000):
    """-> (xyz (n, 3) float32, the true normals (n, 3) float64): a unit sphere with isotropic Gaussian jitter, sigma 0.01"""
    g = np.random.default_rng(0)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d + SIGMA * g.normal(size=(n, 3))).astype(np.float32), d


@functools.lru_cache(maxsize=None)
def noisy_cube(n=3000):
    """-> (xyz, the true normals): the surface of the cube [-1, 1]^3 with the same jitter"""
    g = np.random.default_rng(0)
    face = g.integers(0, 6, n)
    axis, sign = face // 2, (face % 2) * 2.0 - 1.0
    p = g.uniform(-1.0, 1.0, (n, 3))
    nrm = np.zeros((n, 3))
    p[np.arange(n), axis] = sign
    nrm[np.arange(n), axis] = sign
    return (p + SIGMA * g.normal(size=(n, 3))).astype(np.float32), nrm


def integer_lattice(m=8):
    """m^3 points with integer coordinates: at radius 1 every one of a point's six neighbours has a key EQUAL to r2"""
    i = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3).copy()


def radius_for(N):
    """about 30 neighbours on the unit sphere, N * R^2 / 4; for the smallest clouds a radius beyond the whole cloud"""
    return SPHERE_RADIUS if N == 3000 else float(min(2.5, np.sqrt(120.0 / N)))


def cell_for_ratio_8(radius):
    """the smallest float32 cell with radius / cell <= 8"""
    cell = np.float32(radius / 8)
    while radius / float(cell) > 8:
        cell = np.nextafter(cell, np.float32(np.inf))
    return float(cell)


def grids_for(lo, size, radius):
    """name -> grid or None over the box [lo, lo + size]^3: the automatic grid, one cell, radius / cell = 8 (a search of nine or ten
    rings), and dims (5, 1, 17)"""
    fine = cell_for_ratio_8(radius)
    n = int(min(128, max(1, np.ceil(size / fine))))
    return {"auto": None, "one": ((lo, lo, lo), size, (1, 1, 1)), "ratio8": ((lo, lo, lo), fine, (n, n, n)), "odd": ((lo, lo, lo), size / 5, (5, 1, 17))}


@functools.lru_cache(maxsize=None)
def count_cases():
    """name -> (cloud (N, 3 | 6) float32, radius, grids).  Built once; nobody writes to the arrays."""
    cases = {}
    sphere = noisy_sphere()[0]
    noise = np.random.default_rng(1).uniform(-1, 1, sphere.shape).astype(np.float32)   # columns the kernel must not read
    for N in COUNT_N:
        for ld in (3, 6):
            cloud = sphere[:N].copy() if ld == 3 else np.concatenate([sphere[:N], noise[:N]], 1)
            cases[f"n{N}_ld{ld}"] = (cloud, radius_for(N), grids_for(-1.1, 2.2, radius_for(N)))
    cases["tripled"] = (np.concatenate([sphere[:600]] * 3, 0), 0.45, grids_for(-1.1, 2.2, 0.45))
    lat = integer_lattice(8)
    for name, radius in (("lattice_1", 1.0), ("lattice_sqrt2", float(np.sqrt(2.0))), ("lattice_2", 2.0)):
        cases[name] = (lat, radius, dict(grids_for(-0.5, 8.0, radius), faces=((0.0, 0.0, 0.0), 1.0, (8, 8, 8))))
    cases["whole"] = (sphere[:257].copy(), 2.5, grids_for(-1.1, 2.2, 2.5))
    cases["cube"] = (noisy_cube()[0], CUBE_RADIUS, grids_for(-1.1, 2.2, CUBE_RADIUS))
    return cases


@functools.lru_cache(maxsize=None)
def reference(name, shuffled=False):
    """-> smooth_ref of the case, computed once; nobody writes to it"""
    cloud, radius, _ = count_cases()[name]
    return smooth_ref(cloud, radius, perm=shuffle(cloud.shape[0]) if shuffled else None)


@functools.lru_cache(maxsize=None)
def spread(name):
    """the largest deviation between the two restatement orders on the well-posed rows: (moved, sine, eigenvalues)"""
    a, b = reference(name), reference(name, True)
    rows = well_posed(a)
    return tuple(float(v[rows].max()) if rows.any() else 0.0 for v in deviations(b, a, count_cases()[name][1]))


def tolerance(name):
    return tuple(max(1e-12, 100.0 * s) for s in spread(name))
