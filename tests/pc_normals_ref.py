"""Numpy restatements of the raw-point-cloud normals (meshanything_amd/csrc/pc_normals.hpp, meshanything_amd/pc_normals.py) that the
pc_normals tests compare against, and the clouds they share.

* `knn_ref`: brute force in float32 with the kernel's distance key `fl32(fl32(dx*dx + dy*dy) + dz*dz)` (numpy rounds every operation
  and fuses none), sorted by the pair (d, index): the kernel must give the same indices and the same bits.
* `normals_eigh`: float64, the centroid and the covariance summed by numpy over the neighbours in REVERSE list order,
  `np.linalg.eigh`, then the sign rule.
* `normals_in_kernel_order`: the same with the centroid and the covariance summed one neighbour after the other, as the kernel sums
  them.  The deviation between the two on the same inputs measures what float64 resolves there; the GPU test derives its tolerance
  from it.
* clouds with their true normals: sphere, torus (R 0.6, r 0.25), cube surface; and a lattice, where most distances are shared by many
  pairs, so that only the index decides the order.
"""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def sphere(n, seed=0, radius=1.0, center=(0.0, 0.0, 0.0)):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * radius + np.asarray(center)).astype(np.float32), d


def torus(n, seed=0, R=0.6, r=0.25):
    g = np.random.default_rng(seed)
    u, v = g.uniform(0, 2 * np.pi, n), g.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    ring = np.stack([R * np.cos(u), R * np.sin(u), np.zeros(n)], 1)
    return (ring + r * nrm).astype(np.float32), nrm


def cube(n, seed=0, half=0.5):
    g = np.random.default_rng(seed)
    face = g.integers(0, 6, n)
    axis, sign = face // 2, (face % 2) * 2.0 - 1.0
    p = g.uniform(-half, half, (n, 3))
    nrm = np.zeros((n, 3))
    p[np.arange(n), axis] = sign * half
    nrm[np.arange(n), axis] = sign
    return p.astype(np.float32), nrm


def lattice(m=10):
    """m^3 points on a grid of spacing 1/8 (exact in float32): 6 neighbours at the same distance, 12 at the next, ..."""
    i = np.arange(m, dtype=np.float32) / np.float32(8)
    return np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3).copy()


def tripled(n, seed=0):
    """every point three times, the copies far apart in index"""
    p, _ = sphere(n, seed)
    return np.concatenate([p, p, p], 0)


CLOUDS = {"sphere": sphere, "torus": torus, "cube": cube}

# the shapes of the neighbour-search tests: around the 256-query workgroup, the 1024-point tile and the smallest clouds k allows
KNN_K = (3, 8, 16, 32)
KNN_Q = (1, 63, 64, 65, 256, 257)
SPLITS = (1, 2, 7, 0)


def knn_sizes(k):
    return (k, k + 1, 255, 256, 257, 1023, 1024, 1025, 2500)


@functools.lru_cache(maxsize=None)
def knn_cases():
    """name -> (ref (N, 3 | 6) float32, query_idx (Q) int32 or None, k); the cases of one (k, N, ld) share their ref array.  Built once:
    every call returns the same arrays, which nobody writes to."""
    cases = {}
    for k in KNN_K:
        for N in knn_sizes(k):
            g = np.random.default_rng(1000 * k + N)
            for ld in (3, 6):
                ref = g.uniform(-1, 1, (N, ld)).astype(np.float32)   # the columns after xyz are noise the kernel must not read
                cases[f"k{k}_n{N}_ld{ld}_all"] = (ref, None, k)
                for Q in KNN_Q:
                    cases[f"k{k}_n{N}_ld{ld}_q{Q}"] = (ref, g.integers(0, N, Q).astype(np.int32), k)
    for k in (8, 32):
        cases[f"tripled_k{k}"] = (tripled(400, seed=4), None, k)
        cases[f"lattice_k{k}"] = (lattice(10), None, k)
    return cases


# ---- nearest neighbours ------------------------------------------------------------------------------------------------------------
def knn_ref(ref, query_idx, k, chunk=512):
    """ref (N, >= 3) float32, query_idx (Q) or None -> (nbr_idx (Q, k) int32, nbr_d2 (Q, k) float32) ordered by (d, index)"""
    r = np.ascontiguousarray(np.asarray(ref)[:, :3], np.float32)
    qi = np.arange(r.shape[0]) if query_idx is None else np.asarray(query_idx)
    idx = np.empty((qi.shape[0], k), np.int32)
    d2 = np.empty((qi.shape[0], k), np.float32)
    for q0 in range(0, qi.shape[0], chunk):
        q = r[qi[q0:q0 + chunk]]
        dx = q[:, None, 0] - r[None, :, 0]
        dy = q[:, None, 1] - r[None, :, 1]
        dz = q[:, None, 2] - r[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        d[np.isnan(d)] = np.inf
        # the k smallest of a row by (d, index) without sorting the row: everything up to the k-th smallest value, then a sort of those
        kth = np.partition(d, k - 1, axis=1)[:, k - 1:k]
        rows, cols = np.nonzero(d <= kth)
        vals = d[rows, cols]
        order = np.lexsort((cols, vals, rows))
        rows, cols, vals = rows[order], cols[order], vals[order]
        keep = np.arange(rows.shape[0]) - np.searchsorted(rows, np.arange(q.shape[0]))[rows] < k
        idx[q0:q0 + chunk] = cols[keep].reshape(-1, k)
        d2[q0:q0 + chunk] = vals[keep].reshape(-1, k)
    return idx, d2


# ---- normals -----------------------------------------------------------------------------------------------------------------------
def sign_rule(v):
    """the component of largest magnitude positive, the lowest axis on ties"""
    v = np.array(v, np.float64)
    lead = np.take_along_axis(v, np.argmax(np.abs(v), axis=1)[:, None], 1)[:, 0]
    v[lead < 0] *= -1.0
    return v


def _from_cov(cov, pts):
    w, vec = np.linalg.eigh(cov)
    n = sign_rule(vec[:, :, 0])
    same = (pts == pts[:, :1]).all((1, 2))
    n[same] = (0.0, 0.0, 1.0)
    w[same] = 0.0
    return n, w


def normals_eigh(ref, nbr_idx):
    """-> (normals (Q, 3), eigvals (Q, 3) ascending), float64"""
    pts = np.asarray(ref)[:, :3].astype(np.float64)[np.asarray(nbr_idx)]          # (Q, k, 3)
    rev = np.ascontiguousarray(pts[:, ::-1])
    d = rev - rev.mean(1, keepdims=True)
    return _from_cov(np.einsum("qki,qkj->qij", d, d) / pts.shape[1], pts)


def normals_in_kernel_order(ref, nbr_idx):
    pts = np.asarray(ref)[:, :3].astype(np.float64)[np.asarray(nbr_idx)]
    k = pts.shape[1]
    s = np.zeros((pts.shape[0], 3))
    for j in range(k):
        s = s + pts[:, j]
    c = s / k
    cov = np.zeros((pts.shape[0], 3, 3))
    for j in range(k):
        d = pts[:, j] - c
        cov = cov + d[:, :, None] * d[:, None, :]
    return _from_cov(cov / k, pts)


def gap_ratio(eigvals):
    """(l1 - l0) / l2: how well the smallest eigenvector is separated; 0 where l2 is 0"""
    w = np.asarray(eigvals, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (w[:, 1] - w[:, 0]) / w[:, 2]
    return np.where(w[:, 2] > 0, g, 0.0)


def sine(a, b):
    """|a x b| of unit vectors: the sine of the angle between the two LINES"""
    return np.linalg.norm(np.cross(a, b), axis=1)


def signed_share(normals, true_normals):
    return float((np.einsum("ij,ij->i", np.asarray(normals, np.float64), true_normals) > 0).mean())
