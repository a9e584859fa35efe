"""What the surface-sampling tests share: the host sampler restated with explicit draws (mesh_input.sample_surface takes them from the
global RNG), and the meshes beyond tests/watertight_ref.py's that pin the sampler's edge cases."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd.mesh_input import face_normals_and_areas  # noqa: E402

import watertight_ref as W  # noqa: E402


def host_sample(v, f, u, uv):
    """mesh_input.mesh_to_pc_normal on given draws u (count,) and uv (count, 2): (cloud (count, 6) float16, face index (count,) int64,
    normals (F, 3), cum (F,))."""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    normals, areas = face_normals_and_areas(v, f)
    cum = np.cumsum(areas)
    pick = u * cum[-1]
    idx = np.minimum(np.searchsorted(cum, pick, side="right"), len(cum) - 1)
    uv = np.array(uv, np.float64)
    fold = uv.sum(axis=1) > 1.0
    uv[fold] = 1.0 - uv[fold]
    tri = v[f[idx]]
    points = tri[:, 0] + uv[:, :1] * (tri[:, 1] - tri[:, 0]) + uv[:, 1:] * (tri[:, 2] - tri[:, 0])
    return np.concatenate([points, normals[idx]], axis=-1, dtype=np.float16), idx, normals, cum


def right_triangle(o, a, b, axes=(0, 1)):
    """The right triangle at o with legs a and b along two coordinate axes: area a * b / 2, computed exactly for dyadic a, b."""
    o = np.asarray(o, np.float64)
    p, q = o.copy(), o.copy()
    p[axes[0]] += a
    q[axes[1]] += b
    return [o, p, q]


def boundary_mesh():
    """8 faces with areas 0, 1/2, 0, 1, 1/4, 0, 1/4, 0: cum = 0, .5, .5, 1.5, 1.75, 1.75, 2, 2 exactly, total 2."""
    v, f = [], []
    for i, (a, b) in enumerate([(0.0, 1.0), (1.0, 1.0), (1.0, 0.0), (1.0, 2.0), (0.5, 1.0), (0.0, 0.0), (1.0, 0.5), (0.5, 0.0)]):
        f.append((len(v), len(v) + 1, len(v) + 2))
        v += right_triangle((i, 0.0, 0.5 * i), a, b, axes=(0, 1) if i % 2 else (1, 2))
    return np.array(v), np.array(f, np.int64)


def dyadic_mesh(n=100_000, seed=5):
    """n right triangles with dyadic legs in the three axis planes (a quarter of them zero-area): every area, every partial sum and
    every cross product is exact, so any summation order gives np.cumsum's values."""
    rng = np.random.default_rng(seed)
    legs = 2.0 ** rng.integers(-4, 2, size=(n, 2))
    legs[rng.random(n) < 0.25, 0] = 0.0
    org = np.round(rng.uniform(-1, 1, (n, 3)) * 64) / 64
    axes = [(0, 1), (1, 2), (2, 0)]
    v = np.empty((3 * n, 3))
    for i in range(n):
        v[3 * i:3 * i + 3] = right_triangle(org[i], legs[i, 0], legs[i, 1], axes[i % 3])
    return v, np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def heightfield(nx=512, ny=1024, seed=7):
    """A random height field of 2 * nx * ny triangles (2^20 with the defaults)."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(-1, 1, nx + 1), np.linspace(-1, 1, ny + 1), indexing="ij")
    z = 0.1 * rng.standard_normal(x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    b, c, d = a + ny + 1, a + ny + 2, a + 1
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    return v, f.astype(np.int64)


def open_box_degenerate():
    """The open box with zero-area faces spliced in: repeated vertices and a collinear triple, before, between and after."""
    v, f = W.open_box()
    v = np.vstack([v, [[0.0, -0.7, -0.7], [0.7, -0.7, -0.7]]])         # midpoint of edge 0-1 and a copy of vertex 1
    deg = np.array([[0, 0, 0], [0, 8, 1], [2, 2, 3], [1, 9, 1]], np.int64)
    f = np.vstack([deg[:2], f[:5], deg[2:3], f[5:], deg[3:]])
    return v, f


def single_triangle():
    return np.array([[0.1, 0.2, 0.3], [0.9, -0.1, 0.2], [0.3, 0.8, -0.4]]), np.array([[0, 1, 2]], np.int64)


def no_area():
    """Three faces on one line: no surface to sample."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.5, 0.5, 0.5]])
    return v, np.array([[0, 1, 2], [1, 3, 2], [0, 0, 3]], np.int64)


MESHES = {"icosphere": W.icosphere, "torus": W.torus, "sliver_soup": W.sliver_soup, "collinear": W.collinear,
          "open_box_degenerate": open_box_degenerate, "single_triangle": single_triangle, "heightfield_1m": heightfield,
          "dyadic": dyadic_mesh, "boundary": boundary_mesh}
