"""Numpy restatement of the tightest-box kernel (meshanything_amd/csrc/pc_align.hpp, C ABI ma_op_pc_align_extents, meshanything_amd/pc_align.py)
that the pc_align tests compare against, and the clouds they share.

* `extents_ref`: the rule in float32, every product and sum a numpy operation of its own (numpy rounds each and fuses none):
  q = p - c, u_a = ((r_a0*qx + r_a1*qy) + r_a2*qz) + 0.0f, lo = min over the rows, hi = max; a hypothesis is bad iff one of its nine
  entries or one u is not finite: six NaN extents, volume +inf, never best.  volume = ((double)hi0 - (double)lo0) * ((double)hi1 -
  (double)lo1), then * ((double)hi2 - (double)lo2).  best: the least volume among those not bad, the first among equals, -1 if none.  The
  kernel must give EQUAL bits.
* `score_of`: the `score` callable of `pc_align.search` over it.
* `box_surface`, `ball`, `turn`: the clouds of the search tests; `angle_to_cube`: how far a rotation is from the nearest of the cube's 24.
"""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ROWS_PER_GROUP = 8192                                              # pca::ROWS: the rows of one workgroup of extent_kernel
HYP_TILE = 8                                                       # pca::TILE: the hypotheses of one workgroup


def extents_ref(xyz, rot, centre, chunk=64):
    """xyz (N, >= 3), rot (H, 9) or (H, 3, 3), centre (3) -> (extents (H, 6) float32, volumes (H) float64, best int)"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], F32)
    r = np.ascontiguousarray(np.asarray(rot, F32).reshape(-1, 9))
    c = np.asarray(centre, F32)
    H = r.shape[0]
    ext = np.empty((H, 6), F32)
    bad = ~np.isfinite(r).all(1)
    zero = F32(0)
    with np.errstate(all="ignore"):
        qx, qy, qz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        assert qx.dtype == np.float32
        for h0 in range(0, H, chunk):
            m = r[h0:h0 + chunk]
            for a in range(3):
                t0 = m[:, None, 3 * a] * qx[None, :]
                t1 = m[:, None, 3 * a + 1] * qy[None, :]
                t2 = m[:, None, 3 * a + 2] * qz[None, :]
                s = t0 + t1
                s = s + t2
                u = s + zero
                assert u.dtype == np.float32
                bad[h0:h0 + chunk] |= ~np.isfinite(u).all(1)
                ext[h0:h0 + chunk, a] = np.fmin.reduce(u, axis=1)    # a NaN u makes the hypothesis bad: what fmin does with it is never read
                ext[h0:h0 + chunk, 3 + a] = np.fmax.reduce(u, axis=1)
        e = ext.astype(np.float64)
        vol = (e[:, 3] - e[:, 0]) * (e[:, 4] - e[:, 1])
        vol = vol * (e[:, 5] - e[:, 2])
    ext[bad] = np.nan
    vol[bad] = np.inf
    return ext, vol, (int(np.argmin(vol)) if not bad.all() else -1)  # argmin: the first of the least; a volume that is not bad is finite


def score_of(xyz, centre=None):
    """The `score` of pc_align.search over the restatement; centre: the float32 bounding-box mid-point unless given"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], F32)
    c = (p.min(0) + p.max(0)) / F32(2) if centre is None else np.asarray(centre, F32)

    def score(rot32):
        assert rot32.dtype == np.float32 and rot32.ndim == 2 and rot32.shape[1] == 9
        _, vol, best = extents_ref(p, rot32, c)
        return vol, best
    return score


def brute64(xyz, rot, centre):
    """the extents in float64, of the float32 inputs: the geometry the rule approximates"""
    q = np.asarray(xyz)[:, :3].astype(F32).astype(np.float64) - np.asarray(centre, F32).astype(np.float64)[None, :]
    u = np.einsum("hak,nk->han", np.asarray(rot, F32).astype(np.float64).reshape(-1, 3, 3), q)
    return np.concatenate([u.min(2), u.max(2)], 1)


# ---- clouds -----------------------------------------------------------------------------------------------------------------------------
BOX = (1.0, 0.6, 0.3)
BOX_VOLUME = 0.18


def rotation(axis, degrees):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


R_25 = rotation((1, 2, 3), 25.0)                                   # the turn of the box tests: 25 degrees about (1, 2, 3) / sqrt(14)
R_10Z = rotation((0, 0, 1), 10.0)


def box_surface(n, seed):
    """-> (xyz (n, 3), normals (n, 3)) float64: n rows uniform on the surface of the box of edges BOX about the origin, by face area"""
    g = np.random.default_rng([seed, 20])
    half = np.array(BOX) / 2
    area = np.array([BOX[1] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[1]])
    axis = g.choice(3, n, p=area / area.sum())
    side = g.choice([-1.0, 1.0], n)
    xyz = g.uniform(-1, 1, (n, 3)) * half[None, :]
    xyz[np.arange(n), axis] = side * half[axis]
    normals = np.zeros((n, 3))
    normals[np.arange(n), axis] = side
    return xyz, normals


def turn(xyz, R, shift=(0.0, 0.0, 0.0)):
    return xyz @ np.asarray(R).T + np.asarray(shift)


def ball(n, seed):
    """n rows uniform on the unit sphere, the ball's skin.  Rows uniform INSIDE the ball are too sparse near its boundary for the default
    min_gain: 6 000 of them leave the search a gain of 3.1 %, these 0.3 %."""
    g = np.random.default_rng([seed, 21])
    d = g.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def angle_between(A, B):
    """the angle of A BT in radians"""
    return float(np.arccos(np.clip((np.trace(np.asarray(A) @ np.asarray(B).T) - 1) / 2, -1, 1)))


def angle_to_cube(M, cube):
    """the least angle between M and one of `cube` (24, 3, 3)"""
    return min(angle_between(M, C) for C in cube)


# ---- the kernel's cases -------------------------------------------------------------------------------------------------------------------
def uniform_cloud(N, ld, seed=0):
    return np.random.default_rng([seed, N, ld, 20]).uniform(-1, 1, (N, ld)).astype(F32)


def uniform_rotations(H, seed=0):
    """(H, 9) float32: H - 1 random rotations scaled a little off orthonormal, after the identity"""
    g = np.random.default_rng([seed, H, 22])
    q, _ = np.linalg.qr(g.standard_normal((H, 3, 3)))
    out = (q * g.uniform(0.9, 1.1, (H, 1, 1))).reshape(H, 9).astype(F32)
    out[0] = np.eye(3, dtype=F32).reshape(9)
    return out


SHAPES = tuple([(1, 3, 1), (1, 6, 9)] + [(257, ld, H) for ld in (3, 6) for H in (1, 3, 65)] +
               [(ROWS_PER_GROUP * k + d, 3, 5) for k in (1, 2) for d in (-1, 0, 1)] +
               [(300, 3, HYP_TILE - 1), (300, 6, HYP_TILE), (300, 3, HYP_TILE + 1)])   # (N, ld, H)
CENTRE = np.array([0.125, -0.25, 0.0625], F32)


@functools.lru_cache(maxsize=None)
def uniform_case(N, ld, H):
    """-> (cloud (N, ld), rot (H, 9), centre, (extents, volumes, best)); nobody writes to it"""
    cloud, rot = uniform_cloud(N, ld), uniform_rotations(H)
    return cloud, rot, CENTRE, extents_ref(cloud, rot, CENTRE)


@functools.lru_cache(maxsize=None)
def content_cases():
    """name -> (cloud, rot, centre, (extents, volumes, best))"""
    out = {}
    rot = uniform_rotations(11, seed=1)
    # every row equal to the centre: q = 0, every product a zero of some sign, every extent +0
    cloud = np.tile(CENTRE, (70, 1))
    out["at_centre"] = (cloud, rot, CENTRE)
    # products that are -0: rows on the axes against entries of both signs and zeros
    cloud = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, -0.0], [-0.0, -0.0, -0.0]], F32)
    signs = np.array([[1, 0, 0, 0, -1, 0, 0, 0, 1], [-1, 0, 0, 0, 1, 0, 0, 0, -1], [0, -1, 0, -0.0, 0, 1, 0, 0, 0], [-0.0] * 9, [0, 0, -1, 0, 0, -1, 0, 0, -1]], F32)
    out["minus_zero"] = (cloud, signs, np.zeros(3, F32))
    # two identical hypotheses that share the least volume: the lower index wins
    cloud = (box_surface(600, 3)[0] @ R_10Z.T).astype(F32)
    twin = uniform_rotations(20, seed=2)
    twin[13] = twin[4] = R_10Z.T.astype(F32).reshape(9)
    out["twin"] = (cloud, twin, np.zeros(3, F32))
    # bad hypotheses: a NaN entry, an infinite entry; finite rows of 3e38 whose sums overflow make every hypothesis with two entries on a row bad
    cloud = uniform_cloud(257, 6, seed=5)
    nan_rot = uniform_rotations(9, seed=3)
    nan_rot[2, 4] = np.nan
    nan_rot[5, 0] = np.inf
    out["nan_entry"] = (cloud, nan_rot, CENTRE)
    big = uniform_cloud(300, 3, seed=6)
    big[17] = (3e38, 3e38, 0)
    big[200] = (-3e38, 1, 3e38)
    over = uniform_rotations(9, seed=4)
    over[1] = np.eye(3, dtype=F32).reshape(9)                        # the identity keeps every u finite: not bad
    over[6] = (F32(0.5) * np.eye(3, dtype=F32)).reshape(9)
    over[3] = (2, -2, 0, 0, 0.1, 0, 0, 0, 0.1)                       # row 17: inf + -inf = NaN on axis 0, which no min or max shows
    out["overflow"] = (big, over, np.zeros(3, F32))
    sums = np.array([[1, 1, 0, 1, -1, 0, 0, 0, 1], over[3]], F32)     # row 17: 3e38 + 3e38 = inf on axis 0, finite on axis 1: bad all the same
    out["all_bad"] = (big, np.concatenate([sums, nan_rot[2:3]]), np.zeros(3, F32))
    return {k: (c, r, ce, extents_ref(c, r, ce)) for k, (c, r, ce) in out.items()}
