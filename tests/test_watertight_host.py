"""Watertight remeshing (`--mc`, meshanything_amd/watertight.py), host side: the marching-cubes table the kernel reads (through the
library's host-only ma_mc_table) and the numpy restatement of both kernels (tests/watertight_ref.py) on fields and meshes whose answer
is known; Dataset.from_clouds; the input checks that run before any launch.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import watertight_ref as W
from meshanything_amd import _lib
from meshanything_amd.data import Dataset, uid_of
from meshanything_amd.mesh_input import load_mesh, mesh_to_pc_normal
from meshanything_amd import watertight

REPO = W.REPO


def test_committed_table_is_the_generators_output():
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_mc_table.py"), "--check"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tris, edges, ntris = W.mc_table()
    assert tris.shape == (256, 15) and ntris[0] == 0 and ntris[255] == 0
    assert ntris.max() <= 5 and (ntris[1:255] > 0).all()
    # the 12 edges: every (corner, axis) whose corner is the lower end along that axis; no triangle repeats an edge
    assert sorted(map(tuple, edges.tolist())) == sorted({(c & 1, c >> 1 & 1, c >> 2 & 1, a) for a in range(3) for c in range(8) if not c >> a & 1})
    for c in range(256):
        fwd = {tuple(t) for t in tris[c, :3 * ntris[c]].reshape(-1, 3).tolist()}
        for a, b, e in fwd:
            assert len({a, b, e}) == 3


def test_random_fields_reach_every_case_and_stay_closed():
    rng = np.random.default_rng(0)
    seen = set()
    level = 0.5
    for _ in range(4):
        n = 22
        f = rng.random((n, n, n)).astype(np.float32)
        f[[0, -1], :, :] = f[:, [0, -1], :] = f[:, :, [0, -1]] = 1.0       # the border is above the level: the surface must close
        up = (f >= level).astype(np.int64)
        ci = sum(up[c & 1:n - 1 + (c & 1), c >> 1 & 1:n - 1 + (c >> 1 & 1), c >> 2 & 1:n - 1 + (c >> 2 & 1)] << c for c in range(8))
        seen |= set(np.unique(ci).tolist())
        v, t = W.marching_cubes(f, level)
        assert t.shape[0] > 0 and t.max() < v.shape[0]
        undirected_twice, directed_once = W.closed_and_oriented(t)
        assert undirected_twice and directed_once
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        # every vertex lies on a crossing grid edge, between its two ends
        frac = v - np.floor(v)
        assert ((frac > 0).sum(1) <= 1).all()
    assert seen == set(range(256))


def test_sphere_gives_two_closed_oriented_shells():
    n = 64
    dx = 2 / n
    g = W.grid_points(np.arange(n), n).astype(np.float64)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    R = 0.55
    v, t = W.marching_cubes(np.abs(np.linalg.norm(x, axis=-1) - R).astype(np.float32), dx)
    assert W.closed_and_oriented(t) == (True, True)
    lab = W.components(t)
    assert lab.max() == 1                                          # two shells
    radii = []
    for L in (0, 1):
        tl = t[lab == L]
        assert W.euler(tl) == 2                                    # each a sphere
        c = v[tl].mean(1) * 2 / n - 1
        r = np.linalg.norm(c, axis=1)
        radii.append(r.mean())
        nrm = W.face_normals(v, tl)
        s = np.sign((nrm * c).sum(1))
        want = 1 if r.mean() > R else -1                           # outer shell outward, inner shell inward (toward larger |r - R|)
        assert (s == want).mean() > 0.999, (s == want).mean()
        assert np.abs(np.abs(r - R) - dx).max() < 0.5 * dx
    assert min(radii) < R < max(radii)


@pytest.mark.parametrize("name", ["open_box", "sliver_soup", "collinear", "degenerate"])
def test_band_udf_is_exact_where_it_matters(name):
    if name == "degenerate":                                       # a segment, a point, a collinear triple and one regular triangle
        v = np.array([[-0.5, -0.5, -0.5], [0.5, 0.2, -0.1], [0.0, 0.6, 0.3], [0.1, -0.2, 0.4], [-0.3, -0.3, 0.1], [0.0, -0.3, 0.1],
                      [0.6, -0.3, 0.1], [0.2, 0.3, -0.6], [0.7, 0.4, -0.6], [0.3, 0.8, -0.5]])
        f = np.array([[0, 1, 1], [3, 3, 3], [4, 5, 6], [7, 8, 9], [2, 2, 0]])
    else:
        v, f = W.MESHES[name]()
    n = 32
    dx = 2 / n
    v32 = W.normalized32(v)
    band = W.band_udf(v32, f, n)
    brute = W.brute_udf(v32, f, n)
    flat = dx * W.FLAT_CELLS
    near = brute < 2 * dx
    assert near.sum() > 100
    # exact wherever the level set can be reached: to rounding, or within its inradius (<= flat) for a face taken as its edges
    assert np.abs(band[near] - brute[near]).max() <= flat
    fin = np.isfinite(band)
    assert (band[fin] >= brute[fin] - 1e-12).all()                 # elsewhere in the band: a min over fewer triangles
    assert (brute[~fin] >= 2 * dx).all()                           # +inf only where the true distance is >= 2 dx
    # the finite points are exactly the union of the widened boxes
    lo, hi = W.band_boxes(v32, f, n)
    cover = np.zeros((n, n, n), bool)
    for a, b in zip(lo, hi):
        cover[a[0]:b[0] + 1, a[1]:b[1] + 1, a[2]:b[2] + 1] = True
    assert np.array_equal(cover, fin)


@pytest.mark.parametrize("name", ["sliver_soup", "collinear", "spanning"])
def test_band_udf_in_fp32_arithmetic_stays_exact(name):
    """The kernel's arithmetic restated in float32 against the true distance: zero-area faces in general position (collinear in real
    numbers, not in fp32) and thin slivers must not pick a plane fp32 cannot resolve."""
    v, f = W.MESHES[name]()
    n = 64
    v32 = W.normalized32(v)
    band = W.band_udf(v32, f, n, dtype=np.float32)
    brute = W.brute_udf(v32, f, n)
    near = brute < 2 * (2 / n)
    assert np.array_equal(np.isfinite(band), np.isfinite(W.band_udf(v32, f, n)))
    assert np.abs(band[near] - brute[near]).max() <= 2e-6


def test_dataset_from_clouds_matches_the_constructor(tmp_path):
    paths = []
    for name in ("icosphere", "torus"):
        v, f = W.MESHES[name]()
        p = tmp_path / f"{name}.shape.obj"
        W.write_obj(p, v, f)
        paths.append(str(p))
    np.random.seed(7)
    ds = Dataset("mesh", paths)
    np.random.seed(7)
    clouds = [mesh_to_pc_normal(*load_mesh(p), 4096) for p in paths]
    ds2 = Dataset.from_clouds(clouds, [uid_of(p) for p in paths])
    assert len(ds2) == len(ds) == 2
    for i in range(2):
        assert ds2[i]["uid"] == ds[i]["uid"] == ("icosphere", "torus")[i]
        assert ds2[i]["pc_normal"].dtype == np.float16
        assert np.array_equal(ds2[i]["pc_normal"].view(np.uint16), ds[i]["pc_normal"].view(np.uint16))
    with pytest.raises(ValueError):
        Dataset.from_clouds(clouds, ["one"])


def test_input_checks_run_before_any_launch():
    v, f = W.open_box()
    bad_vertex = v.copy()
    bad_vertex[3, 1] = np.nan
    cases = [(np.zeros((0, 3)), np.zeros((0, 3), np.int64)),        # empty
             (v, np.zeros((0, 3), np.int64)),                       # no faces
             (bad_vertex, f),                                       # non-finite vertex
             (v, np.vstack([f, [[0, 1, 8]]])),                      # face index out of range
             (v, np.vstack([f, [[0, -1, 2]]])),
             (np.ones((3, 3)), np.array([[0, 1, 2]]))]              # no extent
    for vv, ff in cases:
        with pytest.raises(ValueError):
            watertight.export_to_watertight(vv, ff)
        # the bad mesh comes second: the good one must not have been launched first (on a host without a GPU that would not raise ValueError)
        with pytest.raises(ValueError):
            watertight.process_mesh_to_pc([(v, f), (vv, ff)], marching_cubes=True)
    # Dataset itself stays host-only and keeps refusing --mc, now pointing to the GPU path
    with pytest.raises(NotImplementedError, match="process_mesh_to_pc"):
        Dataset("mesh", ["a.obj"], mc=True)


def test_abi_refuses_bad_arguments_on_the_host():
    W.mc_table()                                                   # builds the library if needed
    lib = _lib.load()
    counts = (C.c_int64 * 2)(-1, -1)
    assert lib.ma_op_marching_cubes(None, 8, 8, 8, 0.5, None, 0, None, 0, counts, None, 0, None) == -1
    assert b"null" in lib.ma_last_error(None)
    assert lib.ma_op_marching_cubes(C.c_void_p(16), 1, 8, 8, 0.5, None, 0, None, 0, counts, C.c_void_p(16), 1 << 30, None) == -1
    assert lib.ma_op_mesh_udf(C.c_void_p(16), 3, C.c_void_p(16), 1, 1, C.c_void_p(16), C.c_void_p(16), 1 << 20, None) == -1
    assert lib.ma_op_mesh_udf(C.c_void_p(16), 3, C.c_void_p(16), 1, 32, C.c_void_p(16), C.c_void_p(16), 1, None) == -1
    assert b"workspace" in lib.ma_last_error(None)
    assert lib.ma_marching_cubes_workspace_bytes(128, 128, 128) > 2 * 8 * 128 ** 3
    assert lib.ma_marching_cubes_workspace_bytes(1, 8, 8) == 0
    assert lib.ma_mesh_udf_workspace_bytes(1000) > 1000 * (24 + 8)
    assert lib.ma_mesh_udf_workspace_bytes(0) == 0
    assert lib.ma_mesh_udf_workspace_bytes((1 << 28) + 1) == 0                      # MA_MESH_UDF_MAX_FACES
    assert lib.ma_op_mesh_udf(C.c_void_p(16), 3, C.c_void_p(16), 2 ** 31 - 1, 32, C.c_void_p(16), C.c_void_p(16), 1 << 40, None) == -1
    assert _lib.ERR_NAMES[_lib.MA_ERR_CAPACITY] == "MA_ERR_CAPACITY"
