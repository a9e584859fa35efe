"""Numpy restatement of voxel thinning (meshanything_amd/csrc/pc_voxel.hpp, C ABI ma_op_pc_voxel_insert / ma_op_pc_voxel_mark,
meshanything_amd/pc_voxel.py) that the pc_voxel tests compare against, the clouds they share, and a writer of .ply point files.

* `voxel_ref`: the rule in float32, every operation a numpy operation of its own (numpy rounds each and fuses none): per axis
  t = (x - o) / L, i = floor(t); a row is skipped when a coordinate is not finite, some t is not >= 0, or some i >= 2^21 (which also
  raises the out-of-range flag); key = ix << 42 | iy << 21 | iz; e = t - (i + 0.5), d = (ex*ex + ey*ey) + ez*ez; the survivor of a voxel
  is its row with the least (d, row index), found by `np.lexsort` over (row index, d, key), by no hash table.  The kernels must give
  the same mask byte for byte.
* the clouds: `hand_cloud` with its hand-listed mask, `face_lattice`, `ties`, `one_voxel`, `one_per_row`, `sphere_cloud`, `shifted`,
  `occupied` (exactly m voxels), gathered by `cases`.
* `write_ply`: ascii, binary little and big endian, float or double, with or without normals, colours and faces.
"""
import functools

import numpy as np

import pc_normals_ref as PN

REPO = PN.REPO
F32 = np.float32
LIMIT = 1 << 21
SHIFT = (1e4, -2e4, 5e3)


def voxel_ref(ref, leaf, origin=None):
    """ref (N, >= 3), leaf -> (keep (N) bool, voxels, out_of_range); origin None: the per-axis minimum of the float32 xyz, what
    `pc_voxel.voxel_keep` passes."""
    xyz = np.ascontiguousarray(np.asarray(ref)[:, :3], F32)
    o = xyz.min(axis=0) if origin is None else np.asarray(origin, F32)
    L = F32(leaf)
    with np.errstate(all="ignore"):
        t = (xyz - o[None, :]) / L
        i = np.floor(t)
        assert t.dtype == np.float32 and i.dtype == np.float32
        ok = np.isfinite(xyz).all(axis=1) & (t >= 0).all(axis=1)
        beyond = ok & (i >= F32(LIMIT)).any(axis=1)
        ok &= ~beyond
        e = t - (i + F32(0.5))
        d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        assert d.dtype == np.float32
    rows = np.flatnonzero(ok)
    ii = i[rows].astype(np.int64)
    key = (ii[:, 0] << 42) | (ii[:, 1] << 21) | ii[:, 2]
    order = np.lexsort((rows, d[rows], key))                         # by key, then d, then row index
    first = np.ones(order.shape[0], bool)
    first[1:] = key[order][1:] != key[order][:-1]
    keep = np.zeros(xyz.shape[0], bool)
    keep[rows[order[first]]] = True
    return keep, int(first.sum()), bool(beyond.any())


# ---- the clouds ---------------------------------------------------------------------------------------------------------------------------
def hand_cloud():
    """(cloud (12, 3), leaf 1, the mask listed by hand); the minimum is the origin (0, 0, 0) and every value is exact in float32"""
    rows = [
        (0.0, 0.0, 0.0),       # 0  voxel (0,0,0), its corner: d = 0.75                                  loses to row 1
        (0.5, 0.5, 0.5),       # 1  voxel (0,0,0), its centre: d = 0                                     KEPT
        (1.0, 0.25, 0.25),     # 2  on the face x = 1: t = 1, floor 1: voxel (1,0,0), d = 0.375          loses to row 3
        (1.75, 0.25, 0.25),    # 3  voxel (1,0,0), d = 0.1875                                            KEPT
        (2.25, 0.5, 0.5),      # 4  voxel (2,0,0), d = 0.0625                                            KEPT: the lower index of two rows at one position
        (2.25, 0.5, 0.5),      # 5  the same position
        (0.25, 1.5, 0.5),      # 6  voxel (0,1,0), d = 0.0625                                            KEPT: the lower index of two mirrored rows
        (0.75, 1.5, 0.5),      # 7  its mirror image about the centre (0.5, 1.5, 0.5), d = 0.0625
        (0.3, 0.3, 2.6),       # 8  alone in voxel (0,0,2)                                               KEPT
        (0.75, 2.5, 0.5),      # 9  voxel (0,2,0), d = 0.0625                                            KEPT: the index decides, not the side
        (0.25, 2.5, 0.5),      # 10 its mirror image
        (2.0, 2.0, 2.0),       # 11 on three faces at once: voxel (2,2,2), alone                         KEPT
    ]
    return np.asarray(rows, F32), 1.0, np.array([0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1], bool)


def face_lattice(m=9):
    """The points k / 8, k = 0 .. m - 1, on all three axes, each also nudged one ulp down and one ulp up on all axes at once (the row of
    (0, 0, 0) stays, so the origin is 0): with leaf 1 / 8 every t is a whole number or one ulp from it, which pins division and floor"""
    k = np.arange(m, dtype=F32) / F32(8)
    lat = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    down = np.maximum(np.nextafter(lat, F32(-np.inf)), F32(0))
    up = np.nextafter(lat, F32(np.inf))
    return np.concatenate([lat, down, up], 0).astype(F32)


def ties(n=600, seed=2):
    """n rows in [0, 4)^3, each followed by a copy and by its mirror image about its voxel's centre (leaf 1), shuffled: only the index decides"""
    g = np.random.default_rng(seed)
    p = (g.integers(0, 4 * 64, (n, 3)) / 64.0).astype(F32)              # multiples of 1 / 64: the mirror image is exact
    mirror = (2 * (np.floor(p) + F32(0.5)) - p).astype(F32)
    rows = np.concatenate([np.zeros((1, 3), F32), p, p, mirror], 0)
    return np.concatenate([rows[:1], rows[1:][g.permutation(3 * n)]], 0)


def one_voxel(n=5000, seed=3):
    """n rows in one voxel of leaf 1 (the origin's): every atomic lands on one slot"""
    p = np.random.default_rng(seed).uniform(0.0, 0.999, (n, 3)).astype(F32)
    p[n // 2] = 0.0
    return p


def one_per_row(n, seed=4):
    """n rows, each alone in its voxel of leaf 1: row 0 at the origin, the others anywhere inside n - 1 different voxels of a 32^3 block"""
    g = np.random.default_rng(seed)
    cells = 1 + g.permutation(32 * 32 * 32 - 1)[:n - 1]                 # voxel (0,0,0) is row 0's
    p = np.stack([cells // 1024, cells // 32 % 32, cells % 32], 1).astype(F32) + g.uniform(0.1, 0.9, (n - 1, 3)).astype(F32)
    return np.concatenate([np.zeros((1, 3), F32), p], 0).astype(F32)


def sphere_cloud(n=20000, ld=3, seed=5, jitter=0.01):
    """a unit sphere with radial jitter; ld 6: the unit normals in the last three columns"""
    p, nrm = PN.sphere(n, seed=seed)
    p = (p.astype(np.float64) * (1 + jitter * np.random.default_rng(seed + 1).normal(size=(n, 1)))).astype(F32)
    return p if ld == 3 else np.concatenate([p, nrm.astype(F32)], 1)


def shifted(cloud, by=SHIFT):
    out = np.array(cloud, F32)
    out[:, :3] = (out[:, :3].astype(np.float64) + np.asarray(by)).astype(F32)
    return out


def occupied(m, per=5, seed=6):
    """m occupied voxels of leaf 1 along the x axis, `per` rows in each, shuffled"""
    g = np.random.default_rng(seed)
    p = np.concatenate([np.stack([j + g.uniform(0.05, 0.95, per), g.uniform(0.05, 0.95, per), g.uniform(0.05, 0.95, per)], 1) for j in range(m)], 0)
    p = p[g.permutation(p.shape[0])].astype(F32)
    p[0] = 0.0
    return p


SPHERE_LEAF = 0.08


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (cloud, leaf).  Built once; nobody writes to the arrays."""
    out = {"hand": hand_cloud()[:2], "face_lattice": (face_lattice(), 1 / 8), "ties": (ties(), 1.0), "one_voxel": (one_voxel(), 1.0),
           "one_per_row_257": (one_per_row(257), 1.0), "one_row": (np.array([[3.0, -2.0, 7.5]], F32), 0.25), "sphere_ld3": (sphere_cloud(ld=3), SPHERE_LEAF),
           "sphere_ld6": (sphere_cloud(ld=6), SPHERE_LEAF), "shifted": (shifted(sphere_cloud(ld=3)), SPHERE_LEAF), "load_limit": (occupied(8), 1.0)}
    for cloud, _ in out.values():
        cloud.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    cloud, leaf = cases()[name]
    keep, voxels, beyond = voxel_ref(cloud, leaf)
    assert not beyond
    keep.setflags(write=False)
    return keep, voxels


# ---- .ply point files -----------------------------------------------------------------------------------------------------------------------
def write_ply(path, fmt, xyz, normals=None, real="float", colours=False, faces=False, leave_out=()):
    """fmt: ascii | binary_little_endian | binary_big_endian; real: float | double; colours: three uchar properties between xyz and the
    normals; faces: a face element of two triangles after the vertices; leave_out: property names not written."""
    cols = [("x", real, xyz[:, 0]), ("y", real, xyz[:, 1]), ("z", real, xyz[:, 2])]
    if colours:
        cols += [(c, "uchar", np.arange(xyz.shape[0]) % 251) for c in ("red", "green", "blue")]
    if normals is not None:
        cols += [(n, real, normals[:, j]) for j, n in enumerate(("nx", "ny", "nz"))]
    cols = [c for c in cols if c[0] not in leave_out]
    head = ["ply", f"format {fmt} 1.0", "comment a point file", f"element vertex {xyz.shape[0]}"] + [f"property {t} {n}" for n, t, _ in cols]
    if faces:
        head += ["element face 2", "property list uchar int vertex_indices"]
    head.append("end_header")
    np_type = {"float": "f4", "double": "f8", "uchar": "u1"}
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for r in range(xyz.shape[0]):
                f.write((" ".join(repr(float(v[r])) if t != "uchar" else str(int(v[r])) for _, t, v in cols) + "\n").encode("ascii"))
            if faces:
                f.write(b"3 0 1 2\n3 0 2 3\n")
            return
        bo = "<" if fmt == "binary_little_endian" else ">"
        table = np.zeros(xyz.shape[0], np.dtype([(n, bo + np_type[t]) for n, t, _ in cols]))
        for n, _, v in cols:
            table[n] = v
        f.write(table.tobytes())
        if faces:
            for tri in ((0, 1, 2), (0, 2, 3)):
                f.write(np.array([3], "u1").tobytes() + np.array(tri, bo + "i4").tobytes())
