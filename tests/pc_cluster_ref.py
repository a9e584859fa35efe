"""Numpy restatement of Euclidean clustering (meshanything_amd/csrc/pc_cluster.hpp, C ABI ma_op_pc_cluster, meshanything_amd/pc_cluster.py)
that the pc_cluster tests compare against, and the clouds they share.

* `edges_ref`: chunked brute force with the float32 key of `pc_fps_ref.key_to`'s form, (dx*dx + dy*dy) + dz*dz (numpy rounds every
  operation and fuses none): the pairs (i, j), j < i, with d <= r2, r2 = fl32(fl32(radius) * fl32(radius)).
* `cluster_ref`: a sequential union-find over those edges that hooks the larger root to the smaller: labels[i] = the smallest row of
  i's component, int32.  The kernels must give EQUAL labels.
* `walk_ref`: the hook kernel's walk over a grid (the faces and the cell rule of `pc_outliers_ref`, the block that grows by one ring per
  round, the stop rule fl32(b * b) > r2 on every side that is not a grid border): per query the number of points in its final block,
  which is what it evaluates keys against, and whether every linked point lies in that block.  `bound_ref`: the pair bound.
* `scene`: two spheres, a clump and strays: what `--cluster_radius` is for.
"""
import functools

import numpy as np

import pc_fps_ref as F
import pc_normals_ref as PN
import pc_outliers_ref as R

REPO = PN.REPO


def r2_of(radius):
    r = np.float32(radius)
    r2 = r * r
    assert r2.dtype == np.float32
    return r2


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def edges_ref(xyz, radius, chunk=512):
    """-> (E, 2) int64 rows (i, j), j < i, of the linked pairs"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    r2 = r2_of(radius)
    out = []
    for i0 in range(0, p.shape[0], chunk):
        q = p[i0:i0 + chunk]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        i, j = np.nonzero(d <= r2)                                   # a NaN key links nothing
        i += i0
        keep = j < i
        out.append(np.stack([i[keep], j[keep]], 1))
    return np.concatenate(out, 0).astype(np.int64)


def labels_of_edges(N, edges):
    """sequential union-find, the larger root hooked to the smaller -> (N) int32, the smallest row of every component"""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in edges.tolist():
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(N)], np.int32)


def cluster_ref(xyz, radius):
    """xyz (N, >= 3) float32 -> labels (N) int32.  Not cached (arrays do not hash): `reference(name)` is."""
    return labels_of_edges(np.asarray(xyz).shape[0], edges_ref(xyz, radius))


def sizes_ref(labels):
    """(N) int32: the number of rows of a component at its root, 0 elsewhere"""
    return np.bincount(labels, minlength=labels.shape[0]).astype(np.int32)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed=0):
    """-> (xyz (15190, 3) float32, normals (15190, 3) float64, kind (15190) int8: 0 = the large sphere, 1 = the small one, 2 = the clump, 3 = a
    stray): 9 000 points on a sphere of radius 0.5 at (-0.7, 0, 0), 6 000 on one of radius 0.3 at (0.6, 0, 0), a 150-point clump within
    0.03 of (0, 0.9, 0.9), 40 strays uniform in [-1.5, 1.5]^3, the rows shuffled.  Built once; nobody writes to it."""
    a, na = PN.sphere(9000, seed=seed, radius=0.5, center=(-0.7, 0.0, 0.0))
    b, nb = PN.sphere(6000, seed=seed + 1, radius=0.3, center=(0.6, 0.0, 0.0))
    g = np.random.default_rng(seed + 5)                              # the clump, the strays and the shuffle; the spheres: seed and seed + 1
    d = g.normal(size=(150, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    clump = (np.array([0.0, 0.9, 0.9]) + d * (0.03 * g.uniform(0, 1, (150, 1)) ** (1 / 3))).astype(np.float32)
    strays = g.uniform(-1.5, 1.5, (40, 3)).astype(np.float32)
    xyz = np.concatenate([a, b, clump, strays], 0)
    up = np.tile([0.0, 0.0, 1.0], (190, 1))
    normals = np.concatenate([na, nb, up], 0)
    kind = np.concatenate([np.zeros(9000), np.ones(6000), np.full(150, 2), np.full(40, 3)]).astype(np.int8)
    perm = g.permutation(xyz.shape[0])
    return xyz[perm].copy(), normals[perm].copy(), kind[perm].copy()


SCENE_RADIUS = 0.06
UNIFORM_N = (1, 2, 255, 256, 257, 1025, 2500)                        # around the 256-query workgroup
KINDS = ("singletons", "mix", "one")


def _bottleneck(key):
    """the largest edge of the minimum spanning tree of the complete graph with float32 keys `key` (N, N): Prim, O(N^2)"""
    N = key.shape[0]
    best = key[0].copy()
    done = np.zeros(N, bool)
    done[0] = True
    worst = np.float32(0)
    for _ in range(N - 1):
        cand = np.where(done, np.float32(np.inf), best)
        j = int(np.argmin(cand))
        worst = max(worst, cand[j])
        done[j] = True
        best = np.minimum(best, key[j])
    return worst


@functools.lru_cache(maxsize=None)
def uniform_radii(N, ld):
    """-> {kind: radius} for F.uniform_cloud(N, ld), found on the CPU: below the closest pair (all singletons), above the longest edge of
    the minimum spanning tree (one component), and between them a radius whose clustering has, from N = 1025 on, at least one singleton
    and at least one component of more than 256 rows."""
    p = np.ascontiguousarray(F.uniform_cloud(N, ld)[:, :3])
    if N == 1:
        return {"singletons": 0.01, "mix": 0.1, "one": 1.0}
    key = np.stack([F.key_to(p, q) for q in p], 0)
    np.fill_diagonal(key, np.inf)
    closest, longest = float(np.sqrt(key.min())), float(np.sqrt(_bottleneck(key)))
    radii = {"singletons": 0.5 * closest, "one": 1.01 * longest}
    for share in (0.5, 0.6, 0.7, 0.8, 0.9, 0.95):
        radii["mix"] = closest + share * (longest - closest)
        counts = np.bincount(cluster_ref(p, radii["mix"]))
        if N < 1025 or ((counts == 1).any() and counts.max() > 256):
            break
    return radii


@functools.lru_cache(maxsize=None)
def uniform_cases():
    """name -> (cloud (N, 3 | 6) float32, radius).  Built once: every call returns the same arrays, which nobody writes to."""
    cases = {}
    for N in UNIFORM_N:
        for ld in (3, 6):
            cloud = F.uniform_cloud(N, ld)
            for kind, radius in uniform_radii(N, ld).items():
                cases[f"n{N}_ld{ld}_{kind}"] = (cloud, radius)
    return cases


def tie_cases():
    """name -> (cloud, radius): exact ties.  The lattice of spacing 1/8 at radius 1/8 (every edge has d == r2 exactly) and one float32 below
    it; every point three times at a radius whose square underflows to 0 (only d == 0 links); one position repeated 40 times."""
    below = float(np.nextafter(np.float32(0.125), np.float32(0)))
    return {"lattice_at": (PN.lattice(10), 0.125), "lattice_below": (PN.lattice(10), below), "tripled": (PN.tripled(400, seed=4), 1e-30),
            "repeated": (R.repeated_point(), 0.05)}


def all_cases():
    return dict(uniform_cases(), **tie_cases(), scene=(scene(0)[0], SCENE_RADIUS))


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> labels (N) int32 of the case, computed once; nobody writes to it.  Asserts what the case is there for."""
    cloud, radius = all_cases()[name]
    labels = cluster_ref(cloud, radius)
    counts = np.bincount(labels)
    N = cloud.shape[0]
    if name.endswith("_singletons"):
        assert (counts == 1).all()
    if name.endswith("_one"):
        assert counts[0] == N
    if name.endswith("_mix") and N >= 1025:
        assert (counts == 1).any() and counts.max() > 256, name
    return labels


def uniform_grids(radius):
    """name -> (origin, cell, dims) or None: the grids every uniform cloud of [-1, 1)^3 is clustered over.  `fine` has cell < radius, so a
    search needs several rings; the box of `octant` is smaller than the cloud, most points fall in its border cells.  ma_op_pc_cluster
    takes radius / cell <= 8: a fixed grid too fine for the radius is left out (`grids_for`)."""
    cell = np.float32(radius / 2.5)
    n = int(min(max(np.ceil(2.0 / float(cell)), 1), 128))
    return {"auto": None, "1x1x1": ((-1.0, -1.0, -1.0), 2.0, (1, 1, 1)), "8x8x8": ((-1.0, -1.0, -1.0), 0.25, (8, 8, 8)),
            "fine": ((-1.0, -1.0, -1.0), float(cell), (n, n, n)), "octant": ((0.0, 0.0, 0.0), 0.125, (8, 8, 8))}


def grids_for(radius):
    return {k: g for k, g in uniform_grids(radius).items() if g is None or radius / g[1] <= 8}


# ---- the walk and the pair bound -------------------------------------------------------------------------------------------------------
def _cells(p, origin, cell, dims):
    fc = [R.faces(origin[a], cell, int(dims[a])) for a in range(3)]
    return fc, np.stack([R.cells_ref(p[:, a], fc[a]) for a in range(3)], 1)


def walk_ref(xyz, radius, origin, cell, dims):
    """-> (evaluated (N) int64: the points in every query's final block, rounds (N) int64, complete: every linked pair lies inside the
    final block of its larger row)"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    N, r2 = p.shape[0], r2_of(radius)
    dims = np.asarray([int(d) for d in dims])
    fc, pc = _cells(p, origin, cell, dims)
    evaluated, rounds = np.zeros(N, np.int64), np.zeros(N, np.int64)
    final_lo, final_hi = np.zeros((N, 3), np.int64), np.zeros((N, 3), np.int64)
    active, ring = np.arange(N), 0
    while active.size:
        qc = pc[active]
        lo, hi = np.maximum(qc - ring, 0), np.minimum(qc + ring, dims - 1)
        stop = np.ones(active.size, bool)
        for a in range(3):
            q = p[active, a]
            b = q - fc[a][lo[:, a]]
            stop &= (lo[:, a] == 0) | (b * b > r2)
            b = q - fc[a][hi[:, a] + 1]
            stop &= (hi[:, a] == dims[a] - 1) | (b * b > r2)
        final_lo[active[stop]], final_hi[active[stop]], rounds[active[stop]] = lo[stop], hi[stop], ring + 1
        active = active[~stop]
        ring += 1
    for q0 in range(0, N, 512):
        inside = np.ones((min(512, N - q0), N), bool)
        for a in range(3):
            inside &= (pc[None, :, a] >= final_lo[q0:q0 + 512, a, None]) & (pc[None, :, a] <= final_hi[q0:q0 + 512, a, None])
        evaluated[q0:q0 + 512] = inside.sum(1)
    e = edges_ref(p, radius)
    complete = bool(((pc[e[:, 1]] >= final_lo[e[:, 0]]) & (pc[e[:, 1]] <= final_hi[e[:, 0]])).all())
    return evaluated, rounds, complete


def bound_ref(xyz, radius, origin, cell, dims):
    """the pair bound of ma_op_pc_cluster: sum over the cells c of n_c * (the points in the block of R = floor(radius / cell) + 2 rings around c)"""
    p = np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float32)
    dims = [int(d) for d in dims]
    _, pc = _cells(p, origin, cell, dims)
    R_ = int(np.floor(float(np.float32(radius)) / float(np.float32(cell)))) + 2
    n = np.zeros(dims, np.int64)
    np.add.at(n, (pc[:, 0], pc[:, 1], pc[:, 2]), 1)
    s = np.zeros([d + 1 for d in dims], np.int64)                   # summed-area table
    s[1:, 1:, 1:] = n.cumsum(0).cumsum(1).cumsum(2)
    total = 0
    for x, y, z in np.argwhere(n > 0).tolist():
        l = [max(c - R_, 0) for c in (x, y, z)]
        h = [min(c + R_, d - 1) + 1 for c, d in zip((x, y, z), dims)]
        block = (s[h[0], h[1], h[2]] - s[l[0], h[1], h[2]] - s[h[0], l[1], h[2]] - s[h[0], h[1], l[2]] + s[l[0], l[1], h[2]] + s[l[0], h[1], l[2]]
                 + s[h[0], l[1], l[2]] - s[l[0], l[1], l[2]])
        total += int(n[x, y, z]) * int(block)
    return total
