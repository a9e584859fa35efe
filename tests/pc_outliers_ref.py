"""Numpy restatements of statistical outlier removal (meshanything_amd/pc_outliers.py) and of the cell-grid neighbour search under it
(meshanything_amd/csrc/pc_grid.hpp, C ABI ma_op_pc_knn_grid) that the pc_outliers tests compare against, and the clouds they share.

* `mean_dist_ref`: per point the mean of float64 `np.sqrt` over its neighbour list, summed in list order as the kernel sums it.
* `sor_ref`: `pc_normals_ref.knn_ref` over every point, `mean_dist_ref`, threshold = mean + std_ratio * population sigma, keep = m <= T.
* `grid_knn_ref`: the grid search itself: the same float32 faces, the same cell rule (comparisons against the faces), the block that
  grows by one ring per round clipped to the grid, and the strict stop rule.  It must equal `knn_ref`, which shows the stop rule exact
  before any kernel runs.
* `noisy`: a surface of `pc_normals_ref.CLOUDS` plus strays uniform in [-2, 2]^3, shuffled.
"""
import functools

import numpy as np

import pc_normals_ref as PN

REPO = PN.REPO


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy(name, n, n_out, seed):
    """-> (xyz (n + n_out, 3) float32, normals (n + n_out, 3) float64 (a stray's is (0, 0, 1)), stray (n + n_out) bool).  The surface is
    CLOUDS[name](n, seed), the strays come from default_rng(seed + 4), which also shuffles the rows.  Built once; nobody writes to it."""
    p, nrm = PN.CLOUDS[name](n, seed=seed)
    g = np.random.default_rng(seed + 4)
    strays = g.uniform(-2, 2, (n_out, 3)).astype(np.float32)
    xyz = np.concatenate([p, strays], 0)
    normals = np.concatenate([nrm, np.tile([0.0, 0.0, 1.0], (n_out, 1))], 0)
    stray = np.arange(n + n_out) >= n
    perm = g.permutation(n + n_out)
    return xyz[perm].copy(), normals[perm].copy(), stray[perm].copy()


def repeated_point(seed=11):
    """500 uniform points with one position repeated 40 times among them: with k = 32 the k-th key of a copy is 0 and only the index decides"""
    g = np.random.default_rng(seed)
    p = g.uniform(-1, 1, (540, 3)).astype(np.float32)
    at = g.choice(540, 40, replace=False)
    p[at] = p[at[0]]
    return p


# ---- the filter --------------------------------------------------------------------------------------------------------------------
def mean_dist_ref(d2):
    d2 = np.asarray(d2)
    s = np.zeros(d2.shape[0], np.float64)
    for j in range(d2.shape[1]):
        s = s + np.sqrt(d2[:, j].astype(np.float64))
    return s / d2.shape[1]


@functools.lru_cache(maxsize=None)
def _knn16_of_noisy(name, n, n_out, seed):
    return PN.knn_ref(noisy(name, n, n_out, seed)[0], None, 16)


def _knn_of_noisy(name, n, n_out, seed, k):
    """the k best are the first k of the 16 best: one brute force serves every k <= 16"""
    idx, d2 = _knn16_of_noisy(name, n, n_out, seed) if k <= 16 else PN.knn_ref(noisy(name, n, n_out, seed)[0], None, k)
    return idx[:, :k], d2[:, :k]


def threshold_ref(m, std_ratio):
    m = np.asarray(m, np.float64)
    return float(m.mean() + std_ratio * m.std())


def sor_ref(xyz, k=16, std_ratio=2.0, knn=None):
    """-> (keep (N) bool, mean_dist (N) float64, threshold); knn: the (idx, d2) of knn_ref(xyz, None, k) when the caller has them"""
    _, d2 = PN.knn_ref(xyz, None, k) if knn is None else knn
    m = mean_dist_ref(d2)
    T = threshold_ref(m, std_ratio)
    return m <= T, m, T


def sor_of_noisy(name, n, n_out, seed, k, std_ratio):
    return sor_ref(None, k, std_ratio, knn=_knn_of_noisy(name, n, n_out, seed, k))


# ---- the grid search ---------------------------------------------------------------------------------------------------------------
def faces(origin, cell, dim):
    """face[i] = fl32(origin + fl32(i * cell)), i = 0 .. dim"""
    f = np.float32(origin) + np.arange(dim + 1, dtype=np.float32) * np.float32(cell)
    assert f.dtype == np.float32 and (np.diff(f) >= 0).all()
    return f


def cells_ref(x, face):
    """the largest i in [0, dim - 1] with i = 0 or face[i] <= x; NaN -> 0"""
    dim = face.shape[0] - 1
    c = np.searchsorted(face[1:dim], x, side="right")                # how many of face[1 .. dim - 1] are <= x
    return np.where(np.isnan(x), 0, c).astype(np.int64)


def grid_knn_ref(ref, k, origin, cell, dims, return_rounds=False):
    """ref (N, >= 3) float32 -> (nbr_idx (N, k) int32, nbr_d2 (N, k) float32), every row a query, by the grid search: all queries advance
    one round at a time; a query's list after a round is the k best by (d, index) of the points whose cell lies in its block."""
    r = np.ascontiguousarray(np.asarray(ref)[:, :3], np.float32)
    N = r.shape[0]
    dims = [int(d) for d in dims]
    assert 3 <= k <= 32 and k <= N and all(1 <= d <= 128 for d in dims) and np.float32(cell) > 0
    fc = [faces(origin[a], cell, dims[a]) for a in range(3)]
    pc = np.stack([cells_ref(r[:, a], fc[a]) for a in range(3)], 1)  # (N, 3) the cell of every point
    dx = r[:, None, 0] - r[None, :, 0]
    dy = r[:, None, 1] - r[None, :, 1]
    dz = r[:, None, 2] - r[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    d[np.isnan(d)] = np.inf
    final = np.zeros((N, N), bool)                                   # final[q]: the points the search of q looked at
    rounds = np.zeros(N, np.int64)
    active = np.arange(N)
    ring = 0
    while active.size:
        qc = pc[active]
        lo = np.maximum(qc - ring, 0)
        hi = np.minimum(qc + ring, np.asarray(dims) - 1)
        inside = np.ones((active.size, N), bool)
        for a in range(3):
            inside &= (pc[None, :, a] >= lo[:, a, None]) & (pc[None, :, a] <= hi[:, a, None])
        whole = ((lo == 0) & (hi == np.asarray(dims) - 1)).all(1)
        dm = np.where(inside, d[active], np.float32(np.inf))
        full = inside.sum(1) >= k
        kth = np.partition(dm, k - 1, axis=1)[:, k - 1]
        bound = np.full(active.size, np.inf, np.float32)
        for a in range(3):
            q = r[active, a]
            b = q - fc[a][lo[:, a]]
            bound = np.where(lo[:, a] > 0, np.minimum(bound, b * b), bound)
            b = q - fc[a][hi[:, a] + 1]
            bound = np.where(hi[:, a] < dims[a] - 1, np.minimum(bound, b * b), bound)
        assert bound.dtype == np.float32
        stop = whole | (full & (kth < bound))                        # strictly below
        final[active[stop]] = inside[stop]
        rounds[active[stop]] = ring + 1
        active = active[~stop]
        ring += 1
    dm = np.where(final, d, np.float32(np.inf))
    order = np.argsort(dm, axis=1, kind="stable")[:, :k]             # stable: equal keys stay in index order
    assert final.sum(1).min() >= k
    out = order.astype(np.int32), np.take_along_axis(dm, order, 1)
    return out + (rounds,) if return_rounds else out


def uniform_grid_cases(cloud):
    """name -> (origin, cell, dims): the grids every uniform cloud of [-1, 1]^3 is searched over, the automatic one aside"""
    return {
        "1x1x1": ((-1.0, -1.0, -1.0), 2.0, (1, 1, 1)),
        "2x1x1": ((-1.0, -1.0, -1.0), 1.0, (2, 1, 1)),
        "7x5x3": ((-1.0, -1.0, -1.0), 0.3, (7, 5, 3)),
        "16x16x16": ((-1.0, -1.0, -1.0), 0.125, (16, 16, 16)),
        "128x1x1": ((-1.0, -1.0, -1.0), 2.0 / 128, (128, 1, 1)),
        "octant": ((0.0, 0.0, 0.0), 0.125, (8, 8, 8)),               # most points clamp into the border cells
        "disjoint": ((3.0, 3.0, 3.0), 0.25, (4, 4, 4)),              # every point lands in the corner cell (0, 0, 0)
    }


GRID_SIZES_K = PN.KNN_K


def grid_sizes(k):
    return (k, k + 1, 255, 257, 1025, 2500)
