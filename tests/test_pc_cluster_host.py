"""Euclidean clustering (`--cluster_radius`, meshanything_amd/pc_cluster.py) without a GPU: the numpy restatement (tests/pc_cluster_ref.py)
against two independent routes to the components; the exact ties; the scene the GPU tests rest on; the restated walk, which checks the
stop rule and the pair bound before any kernel runs; the host helpers; every refusal that comes before the first device call; the
command line's new flags; `pc_frame`, `merge_meshes` and `shard_grouped`."""
import ctypes as C
import sys
from collections import deque

import numpy as np
import pytest
import torch

import pc_cluster_ref as CR
import pc_normals_ref as PN

REPO = CR.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, dp, mesh_export, pc_cluster, pc_common, pc_outliers   # noqa: E402
from meshanything_amd.data import Dataset, normalize_pc, pc_frame                      # noqa: E402


# ---- the restatement against independent routes -------------------------------------------------------------------------------------------
def _bfs_labels(N, edges):
    nbrs = [[] for _ in range(N)]
    for i, j in edges.tolist():
        nbrs[i].append(j)
        nbrs[j].append(i)
    labels = np.full(N, -1, np.int32)
    for s in range(N):                                               # ascending: the first row of a component is its smallest
        if labels[s] >= 0:
            continue
        labels[s] = s
        queue = deque([s])
        while queue:
            for v in nbrs[queue.popleft()]:
                if labels[v] < 0:
                    labels[v] = s
                    queue.append(v)
    return labels


@pytest.mark.parametrize("name", ["lattice_at", "tripled", "repeated", "scene"])
def test_restatement_equals_a_breadth_first_search_and_scipy(name):
    cloud, radius = CR.all_cases()[name]
    labels = CR.reference(name)
    N = cloud.shape[0]
    edges = CR.edges_ref(cloud, radius)
    assert labels.dtype == np.int32 and labels.shape == (N,)
    assert np.array_equal(labels, _bfs_labels(N, edges))
    assert (labels <= np.arange(N)).all() and np.array_equal(labels[labels], labels)
    try:                                                             # scipy's components too, where it imports
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return
    n, comp = connected_components(coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(N, N)), directed=False)
    first = np.full(n, N, np.int64)
    np.minimum.at(first, comp, np.arange(N))
    assert n == np.unique(labels).shape[0] and np.array_equal(first[comp].astype(np.int32), labels)


def test_exact_ties():
    lat = PN.lattice(10)
    assert CR.edges_ref(lat, 0.125).shape[0] == 2700 and (CR.reference("lattice_at") == 0).all()   # every edge has d == r2: equality links
    assert np.array_equal(CR.reference("lattice_below"), np.arange(1000, dtype=np.int32))
    assert CR.r2_of(1e-30) == 0
    labels = CR.reference("tripled")
    assert np.unique(labels).shape[0] == 400 and np.array_equal(labels, np.tile(np.arange(400, dtype=np.int32), 3))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_scene_is_two_spheres_a_clump_and_strays(seed):
    xyz, normals, kind = CR.scene(seed)
    assert xyz.shape == (15190, 3) and xyz.dtype == np.float32 and normals.shape == (15190, 3)
    assert np.abs(np.linalg.norm(normals, axis=1) - 1).max() < 1e-12
    for radius in (0.06, 0.04):
        labels = CR.reference("scene") if (seed, radius) == (0, CR.SCENE_RADIUS) else CR.cluster_ref(xyz, radius)
        roots, counts = pc_cluster.components(labels)
        assert counts.tolist() == [9000, 6000, 150] + [1] * 40
        assert (kind[labels == roots[0]] == 0).all() and (kind[labels == roots[1]] == 1).all()      # exactly the two spheres
        assert int((counts >= 4096).sum()) == 2 and int(counts[counts < 4096].sum()) == 190


def test_uniform_radii_give_singletons_a_mix_and_one_component():
    for name in CR.uniform_cases():
        CR.reference(name)                                           # asserts the kind of every case
    for N in (1025, 2500):
        for ld in (3, 6):
            counts = np.bincount(CR.reference(f"n{N}_ld{ld}_mix"))
            assert (counts == 1).any() and counts.max() > 256
    assert {len(CR.grids_for(r)) for c, r in CR.uniform_cases().values() if c.shape[0] != 2} == {5}
    fine = CR.uniform_grids(0.2)["fine"]
    assert fine[1] < 0.2 and CR.uniform_grids(0.2)["octant"][0] == (0.0, 0.0, 0.0)


# ---- the walk: the stop rule is exact, the pair bound is one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n257_ld3_mix", "n1025_ld6_one", "n1025_ld3_singletons", "lattice_at", "lattice_below", "tripled"])
def test_walk_reaches_every_linked_point_and_stays_within_the_bound(name):
    cloud, radius = CR.all_cases()[name]
    grids = dict(CR.grids_for(radius), cell8=((0.0, 0.0, 0.0), 1 / 8, (10, 10, 10)), cell16=((0.0, 0.0, 0.0), 1 / 16, (20, 20, 20)))
    grids["auto"] = pc_cluster.choose_cluster_grid(cloud, radius)
    for gname, (origin, cell, dims) in grids.items():
        if radius / cell > 8:
            continue
        evaluated, rounds, complete = CR.walk_ref(cloud, radius, origin, cell, dims)
        assert complete, (name, gname)
        assert rounds.max() <= int(np.floor(np.float32(radius) / np.float32(cell))) + 3        # stopped after round R at the latest
        assert CR.bound_ref(cloud, radius, origin, cell, dims) >= int(evaluated.sum()), (name, gname)


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------------
def test_components_orders_by_count_then_root():
    roots, counts = pc_cluster.components(np.array([0, 1, 1, 3, 4, 4, 1, 4, 8], np.int32))
    assert roots.tolist() == [1, 4, 0, 3, 8] and counts.tolist() == [3, 3, 1, 1, 1] and roots.dtype == np.int64
    for bad in (np.zeros((2, 2), np.int32), np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            pc_cluster.components(bad)


def test_choose_cluster_grid():
    g = np.random.default_rng(0)
    scene = CR.scene(0)[0]
    clouds = [scene, PN.lattice(10), np.zeros((100, 3), np.float32), g.uniform(-1, 1, (3, 3)).astype(np.float32),
              (g.uniform(-1, 1, (200000, 3)) * [5.0, 0.01, 1.0]).astype(np.float32), g.uniform(1e6, 1e6 + 1, (5000, 6))]
    for xyz in clouds:
        for radius in (1e-4, 0.004, 0.06, 0.5, 3.0, 1e3):
            origin, cell, dims = pc_cluster.choose_cluster_grid(xyz, radius)
            again = pc_cluster.choose_cluster_grid(xyz.copy(), radius)
            assert origin.dtype == np.float32 and origin.shape == (3,) and dims.dtype == np.int32 and dims.shape == (3,) and isinstance(cell, np.float32)
            assert origin.tobytes() == again[0].tobytes() and cell == again[1] and dims.tobytes() == again[2].tobytes()
            pc_common.check_grid((origin, cell, dims))            # within the limits always
            assert float(cell) >= radius, (radius, cell)             # 128 cells an axis always allow it (docstring)
    origin, cell, dims = pc_cluster.choose_cluster_grid(scene, 0.06)
    assert 0.06 <= float(cell) < 0.07 and int(dims.max()) >= 30     # as fine as cell >= radius allows
    assert int(pc_cluster.choose_cluster_grid(scene, 1e-4)[2].max()) == 128
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    pc_cluster.choose_cluster_grid(scene, 0.06)
    assert np.array_equal(np.random.get_state()[1], before)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", True, 1e-50):
        with pytest.raises(ValueError):
            pc_cluster.choose_cluster_grid(scene, bad)


# ---- refusals before the first device call ----------------------------------------------------------------------------------------------------
def test_euclidean_clusters_refusals_come_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    for bad, radius, kw in [(pts.double(), 0.1, {}), (torch.zeros((100, 4)), 0.1, {}), (torch.zeros(100), 0.1, {}), (np.zeros((100, 3), np.float32), 0.1, {}),
                            (pts[:0], 0.1, {}), (pts, 0.0, {}), (pts, -0.1, {}), (pts, float("nan"), {}), (pts, float("inf"), {}), (pts, "0.1", {}),
                            (pts, True, {}), (pts, 0.1, {"want": ()}), (pts, 0.1, {"want": ("labels", "idx")}), (pts, 0.1, {"max_pairs": 0}),
                            (pts, 0.1, {"max_pairs": 1.5}), (pts, 0.1, {"max_pairs": 1 << 64}), (pts, 0.1, {"grid": (np.zeros(3), 0.0, (1, 1, 1))}),
                            (pts, 0.1, {"grid": (np.zeros(3), 1.0, (129, 1, 1))}), (pts, 0.1, {"grid": 7}),
                            (pts, 2.01, {"grid": (np.zeros(3), 0.25, (8, 8, 8))})]:             # radius / cell > 8
        with pytest.raises(ValueError):
            pc_cluster.euclidean_clusters(bad, radius, **kw)
    grid = (np.zeros(3, np.float32), np.float32(1.0), np.ones(3, np.int32))
    for kw in ({}, {"grid": grid}, {"want": "sizes"}, {"max_pairs": 1000}):
        with pytest.raises(ValueError, match="CUDA tensor"):         # a valid call stops at the device check: no CPU fallback
            pc_cluster.euclidean_clusters(pts, 0.1, **kw)


def test_split_rows_checks_its_arguments_first():
    good = np.zeros((5000, 3), np.float32)
    nan = good.copy()
    nan[17, 1] = np.nan
    for bad, kw in [(np.zeros((5000, 2), np.float32), {}), (np.zeros(5000, np.float32), {}), (np.zeros((5000, 3), np.int32), {}), (nan, {}),
                    (good[:0], {}), (good, {"radius": 0.0}), (good, {"radius": float("nan")}), (good, {"min_points": 0}), (good, {"min_points": 2.5}),
                    (good, {"mode": "all"}), (np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 22) + 1, 3), (0, 4)), {})]:
        args = dict(radius=0.1, min_points=4096, mode="largest", uid="x")
        args.update(kw)
        with pytest.raises(ValueError):
            pc_cluster.split_rows(bad, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_cluster.split_rows(good, 0.1, 4096, "split", "x", device="cpu")


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    a256 = lambda n: (n + 255) // 256 * 256                          # noqa: E731
    size = lib.ma_pc_cluster_workspace_bytes
    assert size(4096, 4, 5, 6) == lib.ma_pc_knn_grid_workspace_bytes(4096, 16, 4, 5, 6) + a256(4096 * 4) + 256   # the grid's layout, parent, the total
    assert size(1, 1, 1, 1) > 0 and size(1 << 22, 128, 128, 128) < 120 << 20
    for N, nx, ny, nz in [(0, 1, 1, 1), ((1 << 22) + 1, 1, 1, 1), (100, 0, 1, 1), (100, 1, 129, 1), (100, 128, 128, 129), (100, 1, 1, -1)]:
        assert size(N, nx, ny, nz) == 0, (N, nx, ny, nz)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    origin, dims, big = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4), 1 << 40
    bound = C.c_uint64(7)

    def bad(word, *args):
        assert lib.ma_op_pc_cluster(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_cluster:") and word in msg, msg
        assert bound.value == 7                                      # no bound was computed

    bad("null", None, 100, 3, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, None, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, origin, 1.0, None, 0, p, p, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, origin, 1.0, dims, 0, None, p, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), None, big, None)
    bad("1 <= N", p, 0, 3, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("2^22", p, (1 << 22) + 1, 3, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("dim", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(4, 129, 4), 0, p, p, C.byref(bound), p, big, None)
    bad("dim", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(4, 0, 4), 0, p, p, C.byref(bound), p, big, None)
    bad("cells", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(128, 128, 129), 0, p, p, C.byref(bound), p, big, None)
    bad("ref_ld", p, 100, 4, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        bad("radius", p, 100, 3, radius, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("origin", p, 100, 3, 0.5, (C.c_float * 3)(0, float("nan"), 0), 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("cell", p, 100, 3, 0.5, origin, 0.0, dims, 0, p, p, C.byref(bound), p, big, None)
    bad("cell", p, 100, 3, 0.5, origin, float("inf"), dims, 0, p, p, C.byref(bound), p, big, None)
    bad("radius / cell", p, 100, 3, 8.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, big, None)
    # faces that coincide in float32 (an origin huge against the cell): the pair bound would not hold, refused on the host
    bad("faces", p, 100, 3, 1e-3, (C.c_float * 3)(1e6, 0, 0), 1e-3, (C.c_int32 * 3)(64, 4, 4), 0, p, p, C.byref(bound), p, big, None)
    bad("workspace", p, 100, 3, 0.5, origin, 1.0, dims, 0, p, p, C.byref(bound), p, size(100, 4, 4, 4) - 1, None)


# ---- the input side and the command line ------------------------------------------------------------------------------------------------------
def _sphere_file(tmp_path):
    p, n = PN.sphere(5000, seed=2)
    path = str(tmp_path / "sphere.npy")
    np.save(path, np.concatenate([p, n.astype(np.float32)], 1))
    return path


def test_dataset_with_clustering_off_consumes_the_rng_as_before(tmp_path):
    path = _sphere_file(tmp_path)
    np.random.seed(11)
    plain = Dataset("pc_normal", [path])
    state_plain = np.random.get_state()
    np.random.seed(11)
    off = Dataset("pc_normal", [path], cluster_radius=0.0, cluster_mode="split", cluster_min_points=9999)
    state_off = np.random.get_state()
    assert plain.data[0]["pc_normal"].tobytes() == off.data[0]["pc_normal"].tobytes()
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    assert sorted(off.data[0]) == ["pc_normal", "uid"] and sorted(off[0]) == ["pc_normal", "uid"] and off.groups() == [0]


def test_dataset_refusals(tmp_path):
    path = _sphere_file(tmp_path)
    with pytest.raises(ValueError, match="mesh"):
        Dataset("mesh", [], cluster_radius=0.1)
    for kind in ("pc_normal", "pc_xyz"):
        for kw in ({"cluster_radius": -0.1}, {"cluster_radius": float("nan")}, {"cluster_radius": float("inf")}, {"cluster_radius": 0.1, "cluster_mode": "both"},
                   {"cluster_radius": 0.1, "cluster_min_points": 4095}, {"cluster_radius": 0.1, "cluster_min_points": 0}):
            with pytest.raises(ValueError):
                Dataset(kind, [path], **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            Dataset(kind, [path], cluster_radius=0.1, sample_device="cpu")


def test_command_line_flags(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert a.cluster_radius == 0.0 and a.cluster_mode == "largest" and a.cluster_min_points == 4096
    a = main.get_args(base + ["--input_type", "pc_normal", "--cluster_radius", "0.06", "--cluster_mode", "split", "--cluster_min_points", "5000"])
    assert a.cluster_radius == 0.06 and a.cluster_mode == "split" and a.cluster_min_points == 5000
    assert main.get_args(base + ["--input_type", "pc_xyz", "--cluster_radius", "2"]).cluster_mode == "largest"
    assert main.get_args(base + ["--input_type", "mesh", "--cluster_radius", "0"]).cluster_radius == 0.0
    for bad, word in [(["--input_type", "pc_xyz", "--cluster_radius", "-1"], "--cluster_radius"), (["--input_type", "pc_xyz", "--cluster_radius", "nan"], "--cluster_radius"),
                      (["--input_type", "pc_xyz", "--cluster_radius", "inf"], "--cluster_radius"),
                      (["--input_type", "pc_xyz", "--cluster_radius", "0.1", "--cluster_min_points", "4095"], "--cluster_min_points"),
                      (["--input_type", "pc_xyz", "--cluster_mode", "split"], "need --cluster_radius"),
                      (["--input_type", "pc_xyz", "--cluster_min_points", "5000"], "need --cluster_radius"),
                      (["--input_type", "pc_xyz", "--cluster_radius", "0.1", "--cluster_mode", "both"], "--cluster_mode"),
                      (["--input_type", "mesh", "--cluster_radius", "0.1"], "mesh"), (["--input_type", "mesh", "--cluster_mode", "largest"], "mesh"),
                      (["--input_type", "mesh", "--cluster_min_points", "4096"], "mesh")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err


# ---- the output frame -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pc_frame_inverts_normalize_pc(dtype):
    g = np.random.default_rng(3)
    p, n = PN.sphere(4096, seed=5)
    x = (p.astype(np.float64) * [3.0, 0.5, 1.25] + [10.0, -4.0, 0.25] + g.normal(size=(4096, 3)) * 1e-3).astype(dtype)
    rows = np.concatenate([x, n.astype(dtype)], 1)
    centre, scale = pc_frame(rows)
    assert centre.dtype == np.float64 and centre.shape == (3,) and isinstance(scale, float)
    back = centre[None, :] + scale * normalize_pc(rows)[:, :3].astype(np.float64)
    # the normalised coordinates lie in [-1, 1], where fp16's half-ulp is 2^-12; a float32 input is normalised in float32, whose
    # centring, division and scaling each round once more, relative to the coordinates' magnitude
    own = 0.0 if dtype == np.float64 else 4 * np.finfo(np.float32).eps * float(np.abs(x).max())
    assert np.abs(back - x.astype(np.float64)).max() <= scale * 2.0 ** -12 + own
    assert abs(scale - 3.0 / 0.9995) < 0.02 and np.abs(centre - [10.0, -4.0, 0.25]).max() < 0.01


def test_merge_meshes_offsets_the_faces_and_keeps_the_order():
    a = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]]))
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    b = (np.array([[5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]], np.float64), np.array([[0, 2, 1], [3, 1, 0]]))
    v, f = mesh_export.merge_meshes([a, empty, b])
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(v, np.concatenate([a[0], b[0]], 0)) and f.tolist() == [[0, 1, 2], [3, 5, 4], [6, 4, 3]]   # the winding kept
    v, f = mesh_export.merge_meshes([empty, a])
    assert np.array_equal(v, a[0]) and f.tolist() == [[0, 1, 2]]
    v, f = mesh_export.merge_meshes([])
    assert v.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh_export.merge_meshes([(a[0], np.array([[0, 1, 3]]))])


def test_shard_grouped():
    for world in (1, 2, 3, 8):
        for n in (0, 1, 5, 17):
            for rank in range(world):
                assert dp.shard_grouped(list(range(n)), rank, world) == dp.shard_indices(n, rank, world)
        groups = [0, 0, 1, 2, 2, 2, 3, 4, 4, 5]
        owned = [dp.shard_grouped(groups, r, world) for r in range(world)]
        assert sorted(i for o in owned for i in o) == list(range(len(groups)))                      # every item once
        for o in owned:
            assert o == sorted(o)
            mine = {groups[i] for i in o}
            assert all((groups[i] in mine) == (i in o) for i in range(len(groups)))                # a group is never split
    with pytest.raises(ValueError):
        dp.shard_grouped([0, 1], 2, 2)
    ds = Dataset.from_clouds([np.zeros((1, 6))] * 5, list("abcde"))
    ds.data[1].update(group="f", part=0)
    ds.data[2].update(group="f", part=1)
    ds.data[3].update(group="g", part=0)
    assert ds.groups() == [0, 1, 1, 2, 3]
