"""Numpy restatement of farthest-point sampling (meshanything_amd/csrc/pc_fps.hpp, C ABI ma_op_pc_fps) that the pc_fps tests compare
against, and the clouds they share.

`fps_ref` is the definition, float32 operation by float32 operation (numpy rounds every operation and fuses none):
key(a, b) = (dx*dx + dy*dy) + dz*dz; m = +inf; per pick: idx[t] = s, d2[t] = m[s], m = minimum(m, key(p, p[s])), m[s] = -1,
s = argmax(m) (np.argmax returns the lowest index among equals).  start = -1: the row of greatest key to c = (lo + hi) * 0.5 of the
bounding box.  The kernels must give the same indices and the same bits.
"""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_MAX = 1 << 14            # MA_PC_FPS_ONE_MAX_POINTS: the one-workgroup bound B
MANY_SLICE = 512             # points per workgroup of the many-workgroup form while N <= 2^19 (csrc/pc_fps.hpp: MIN_SLICE)


def key_to(p, q):
    """p (N, 3) float32, q (3) float32 -> (N) float32"""
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def start_ref(p):
    lo, hi = p.min(axis=0), p.max(axis=0)
    c = (lo + hi) * np.float32(0.5)
    assert c.dtype == np.float32
    return int(np.argmax(key_to(p, c)))


def fps_ref(points, n, start=-1):
    """points (N, >= 3) float32 -> (idx (n) int32, d2 (n) float32, m (N) float32 after the n-th update)"""
    p = np.ascontiguousarray(np.asarray(points)[:, :3], np.float32)
    N = p.shape[0]
    assert 1 <= n <= N and -1 <= start < N
    s = start_ref(p) if start < 0 else int(start)
    m = np.full(N, np.inf, np.float32)
    idx = np.empty(n, np.int32)
    d2 = np.empty(n, np.float32)
    with np.errstate(over="ignore"):
        for t in range(n):
            idx[t], d2[t] = s, m[s]
            m = np.minimum(m, key_to(p, p[s]))
            m[s] = -1
            s = int(np.argmax(m))
    return idx, d2, m


def nearest_key(points, kept_idx):
    """(N) float32: the smallest key of every point to a kept point, by brute force with the definition's float32 key"""
    p = np.ascontiguousarray(np.asarray(points)[:, :3], np.float32)
    best = np.full(p.shape[0], np.inf, np.float32)
    for j in np.asarray(kept_idx):
        best = np.minimum(best, key_to(p, p[j]))
    return best


def covering_radius(points, kept_idx, chunk=4096):
    """the largest distance from any point to its nearest kept point, in float64 (|a|^2 + |b|^2 - 2 a.b per chunk)"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    k = p[np.asarray(kept_idx)]
    kk = (k * k).sum(1)
    worst = 0.0
    for i in range(0, p.shape[0], chunk):
        a = p[i:i + chunk]
        d = ((a * a).sum(1)[:, None] + kk[None, :] - 2.0 * (a @ k.T)).min(1)
        worst = max(worst, float(d.max()))
    return float(np.sqrt(max(worst, 0.0)))


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def uniform_cloud(N, ld=3, seed=0):
    """(N, ld) float32 in [-1, 1); the columns after xyz are noise the kernel must not read"""
    return np.random.default_rng(seed).uniform(-1, 1, (N, ld)).astype(np.float32)


def lattice(m=8):
    """m^3 points on an integer grid: massive ties, every pick is the lowest index among equals"""
    i = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3).copy()


def few_positions(N=300, distinct=7, seed=3):
    """N rows with only `distinct` different positions"""
    g = np.random.default_rng(seed)
    pos = g.uniform(-1, 1, (distinct, 3)).astype(np.float32)
    return pos[g.integers(0, distinct, N)].copy()


def uneven_sphere():
    """18 000 points on the cap z > 0.8 of the unit sphere, then 2 000 over the whole sphere (float64): the density of a scan"""
    d = np.random.default_rng(0).normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([d[d[:, 2] > 0.8][:18000], d[:2000]])


def sphere(n, seed=0):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.astype(np.float32), d


# the shapes of the GPU test: around a wave, a 256-thread workgroup, the 1024 threads of the one-workgroup form, its bound B, and the
# slices of the many-workgroup form (B + 1: 32 whole slices and one point; B + 512 + 37: 33 whole slices and 37 points)
FPS_N = (255, 256, 257, 1023, 1024, 1025, 2500, ONE_MAX - 1, ONE_MAX, ONE_MAX + 1, ONE_MAX + MANY_SLICE + 37)
FPS_PICKS = (1, 2, 64, 300)


def forms_for(N):
    return (0, 1, 2) if N <= ONE_MAX else (0, 2)


@functools.lru_cache(maxsize=None)
def fps_cases():
    """name -> (cloud (N, 3 | 6) float32, n, start); the cases of one (N, ld) share their array.  Built once: every call returns the same
    arrays, which nobody writes to."""
    cases = {}
    sizes = sorted(set(FPS_N) | {k for k in FPS_PICKS} | {k + 1 for k in FPS_PICKS})
    for N in sizes:
        for ld in (3, 6):
            cloud = uniform_cloud(N, ld, seed=7 * N + ld)
            for n in FPS_PICKS:
                if n > N:
                    continue
                for start in (-1, 0, N - 1):
                    cases[f"n{N}_ld{ld}_k{n}_s{start}"] = (cloud, n, start)
    cases["lattice"] = (lattice(8), 512, -1)
    cases["lattice_from_0"] = (lattice(8), 64, 0)
    cases["few_positions"] = (few_positions(), 64, -1)
    cases["large"] = (uniform_cloud(70000, 3, seed=11), 512, -1)
    return cases


@functools.lru_cache(maxsize=None)
def _longest(cloud_id, start):
    """the reference of the longest case over one (cloud, start): a shorter case is its prefix, pick t does not depend on n"""
    cloud, n = max(((c, k) for c, k, s in fps_cases().values() if id(c) == cloud_id and s == start), key=lambda ck: ck[1])
    return fps_ref(cloud, n, start)[:2]


def reference(name):
    """-> (idx (n) int32, d2 (n) float32) of the case, computed once per (cloud, start)"""
    cloud, n, start = fps_cases()[name]
    idx, d2 = _longest(id(cloud), start)
    return idx[:n], d2[:n]
