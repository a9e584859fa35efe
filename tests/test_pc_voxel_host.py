"""Voxel thinning (`--voxel_size`, meshanything_amd/pc_voxel.py) and .ply point files without a GPU: the numpy restatement
(tests/pc_voxel_ref.py) against a mask listed by hand and against exact arithmetic on the face lattice; every refusal that comes before
the first device call, in Python and in the C ABI; the stage's place in `cloud_prep.STAGES` through `Dataset` with stand-ins for the GPU
functions; that `voxel_size=0` leaves the numpy RNG and the imported modules as they were; the pc_xyz row cap; the command line; and
the .ply reader over every format."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pc_voxel_ref as R

REPO = R.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, mesh_input, pc_cluster, pc_fps, pc_normals, pc_outliers, pc_upsample, pc_voxel   # noqa: E402
from meshanything_amd import cloud_prep                           # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_hand_listed_mask():
    cloud, leaf, want = R.hand_cloud()
    assert cloud.shape == (12, 3) and cloud.dtype == np.float32
    keep, voxels, beyond = R.voxel_ref(cloud, leaf)
    assert keep.dtype == np.bool_ and keep.tolist() == want.tolist() and voxels == 7 and not beyond
    keep_rev, _, _ = R.voxel_ref(cloud[::-1], leaf)                  # the same rows in reverse: ties now go to what was the higher index
    assert keep_rev[::-1].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1]
    wide = np.concatenate([cloud, np.full((12, 3), np.nan, np.float32)], 1)
    assert R.voxel_ref(wide, leaf)[0].tolist() == want.tolist()      # columns after the third are not read


def test_restatement_on_the_shared_clouds():
    assert R.reference("one_voxel") == (R.reference("one_voxel")[0], 1) and int(R.reference("one_voxel")[0].sum()) == 1
    keep, voxels = R.reference("one_per_row_257")
    assert keep.all() and voxels == 257 and keep.shape == (257,)
    assert R.reference("one_row")[0].tolist() == [True]
    assert R.reference("load_limit")[1] == 8
    for name in ("sphere_ld3", "sphere_ld6", "shifted"):
        keep, voxels = R.reference(name)
        assert keep.shape == (20000,) and 2000 <= voxels <= 8000 and int(keep.sum()) == voxels, (name, voxels)
    assert _same(R.reference("sphere_ld3")[0], R.reference("sphere_ld6")[0])
    # ties: every voxel's survivor is the lowest index among the rows of the least d
    cloud, leaf = R.cases()["ties"]
    keep, voxels = R.reference("ties")
    cell = np.floor(cloud).astype(np.int64)
    d = ((cloud - (cell + 0.5)) ** 2).sum(1)                         # exact: multiples of 1 / 64
    for row in np.flatnonzero(keep):
        mates = np.flatnonzero((cell == cell[row]).all(1))
        assert row == mates[d[mates] == d[mates].min()].min()
    assert voxels == np.unique(cell, axis=0).shape[0]


def test_face_lattice_floors_equal_exact_arithmetic():
    cloud, leaf = R.cases()["face_lattice"]
    assert leaf == 1 / 8 and cloud.shape == (3 * 729, 3) and (cloud.min(0) == 0).all()
    exact = np.floor(cloud.astype(np.float64) * 8).astype(np.int64)  # k / 8 and its neighbours times 8: exact in float64, and in float32
    lat = exact[:729]
    assert (exact[729:1458] == np.maximum(lat - 1, 0)).all() and (exact[1458:] == lat).all()   # one ulp below a face: the voxel before it
    keep, voxels = R.reference("face_lattice")
    assert voxels == np.unique(exact, axis=0).shape[0] == 729
    got = np.floor((cloud - cloud.min(0)) / np.float32(leaf)).astype(np.int64)
    assert (got == exact).all()


def test_out_of_range_and_skipped_rows():
    cloud = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [0, np.inf, 0], [3e6, 0, 0], [-1, 0, 0]], np.float32)
    keep, voxels, beyond = R.voxel_ref(cloud, 1.0, origin=(0, 0, 0))
    assert keep.tolist() == [True, True, False, False, False, False] and voxels == 2 and beyond
    assert not R.voxel_ref(cloud[:4], 1.0, origin=(0, 0, 0))[2]


# ---- refusals before the first device call --------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_the_device():
    good = np.random.default_rng(0).uniform(0, 1, (500, 3)).astype(np.float32)
    nan = good.copy()
    nan[7, 2] = np.nan
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "0.1", True, None, 1e-50, 1e39):
        with pytest.raises(ValueError, match="voxel_size"):
            pc_voxel.check_voxel_args(bad)
    assert pc_voxel.check_voxel_args(0.25) == 0.25 and pc_voxel.check_voxel_args(np.float32(2)) == 2.0 and pc_voxel.check_voxel_args(3) == 3.0
    for bad, kw in [(good[:, :2], {}), (good[:, 0], {}), (good.astype(np.int32), {}), (good[:0], {}), (nan, {}),
                    (np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 28) + 1, 3), (0, 4)), {}),
                    (good, {"leaf": 0.0}), (good, {"leaf": float("nan")}), (good, {"chunk_rows": 0}), (good, {"chunk_rows": (1 << 22) + 1}),
                    (good, {"chunk_rows": 2.5}), (good, {"max_voxels": 0}), (good, {"max_voxels": (1 << 22) + 1}), (good, {"capacity": 1}),
                    (good, {"capacity": 24}), (good, {"capacity": 1 << 24}), (good, {"capacity": 16.0}), (good, {"leaf": 1e-7})]:
        kw = {"leaf": 0.1, **kw}
        with pytest.raises(ValueError):
            pc_voxel.voxel_keep(bad, **kw)
    with pytest.raises(ValueError, match="too small"):               # extent / leaf reaches 2^21 - 1: refused on the host
        pc_voxel.voxel_keep(np.array([[0, 0, 0], [1, 0, 0]], np.float32), 1.0 / (1 << 21))
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_voxel.voxel_keep(good, 0.1, device="cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_voxel.thin_rows(good, 0.1, 10, "x", device="cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_voxel.new_table(16, "cpu")
    with pytest.raises(ValueError, match="CUDA tensor"):
        pc_voxel.insert(None, 16, torch.zeros((10, 3)), 0, (0, 0, 0), 1.0)
    for pts, row0 in [(torch.zeros((10, 4)), 0), (torch.zeros((10, 3), dtype=torch.float64), 0), (torch.zeros((0, 3)), 0), (torch.zeros((10, 3)), -1),
                      (torch.zeros((10, 3)), (1 << 28) - 9), (np.zeros((10, 3), np.float32), 0)]:
        with pytest.raises(ValueError):
            pc_voxel.insert(None, 16, pts, row0, (0, 0, 0), 1.0)
    # what check_keep_args hands on
    xyz, origin, leaf, chunk, mv, cap = pc_voxel.check_keep_args(good.astype(np.float64) - 5.0, 0.1)
    assert origin.dtype == np.float32 and _same(origin, (good.astype(np.float64) - 5.0).astype(np.float32).min(0)) and (chunk, mv, cap) == (1 << 22, 1 << 22, 1024)
    assert [pc_voxel.default_capacity(n) for n in (1, 2, 3, 8, 9, 1 << 22, 1 << 28)] == [2, 4, 8, 16, 32, 1 << 23, 1 << 23]
    assert pc_voxel.default_capacity(100, 8) == 16


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    size = lib.ma_pc_voxel_table_bytes
    assert size(16) == 16 * 16 + 256 and size(2) == 2 * 16 + 256 and size(1 << 23) == (128 << 20) + 256
    for capacity in (0, 1, 3, 24, (1 << 23) + 1, 1 << 24, 1 << 40):
        assert size(capacity) == 0, capacity
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    origin, state = (C.c_float * 3)(0, 0, 0), (C.c_uint32 * 4)()

    def bad(fn, word, *args):
        assert getattr(lib, fn)(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    bad("ma_op_pc_voxel_reset", "null", None, 16, None)
    bad("ma_op_pc_voxel_reset", "capacity", p, 24, None)
    bad("ma_op_pc_voxel_reset", "capacity", p, 1, None)
    bad("ma_op_pc_voxel_reset", "capacity", p, 1 << 24, None)
    ins = "ma_op_pc_voxel_insert"
    bad(ins, "null", None, 100, 3, 0, origin, 1.0, p, 16, None)
    bad(ins, "null", p, 100, 3, 0, None, 1.0, p, 16, None)
    bad(ins, "null", p, 100, 3, 0, origin, 1.0, None, 16, None)
    bad(ins, "n <=", p, 0, 3, 0, origin, 1.0, p, 16, None)
    bad(ins, "n <=", p, (1 << 22) + 1, 3, 0, origin, 1.0, p, 16, None)
    bad(ins, "row0", p, 100, 3, -1, origin, 1.0, p, 16, None)
    bad(ins, "row0", p, 100, 3, (1 << 28) - 99, origin, 1.0, p, 16, None)
    bad(ins, "ref_ld", p, 100, 4, 0, origin, 1.0, p, 16, None)
    bad(ins, "origin", p, 100, 3, 0, (C.c_float * 3)(0, float("nan"), 0), 1.0, p, 16, None)
    bad(ins, "origin", p, 100, 3, 0, (C.c_float * 3)(0, 0, float("inf")), 1.0, p, 16, None)
    bad(ins, "leaf", p, 100, 3, 0, origin, 0.0, p, 16, None)
    bad(ins, "leaf", p, 100, 3, 0, origin, -1.0, p, 16, None)
    bad(ins, "leaf", p, 100, 3, 0, origin, float("inf"), p, 16, None)
    bad(ins, "leaf", p, 100, 3, 0, origin, float("nan"), p, 16, None)
    bad(ins, "capacity", p, 100, 3, 0, origin, 1.0, p, 48, None)
    bad(ins, "capacity", p, 100, 3, 0, origin, 1.0, p, 0, None)
    mk = "ma_op_pc_voxel_mark"
    bad(mk, "null", None, 16, p, 100, state, None)
    bad(mk, "null", p, 16, None, 100, state, None)
    bad(mk, "null", p, 16, p, 100, None, None)
    bad(mk, "capacity", p, 17, p, 100, state, None)
    bad(mk, "N <=", p, 16, p, 0, state, None)
    bad(mk, "N <=", p, 16, p, (1 << 28) + 1, state, None)


# ---- the stage's place ----------------------------------------------------------------------------------------------------------------------
N_POINTS, MIN_ROWS = 4096, 64
DROP_VOXEL, DROP_OUTLIERS, DROP_CLUSTER = 200, 10, 50


def origin_of(rows):
    return int(rows[0, 1]), int(rows[0, 0])


@pytest.fixture
def calls(monkeypatch):
    log = []

    def thin_rows(rows, voxel_size, floor, uid, device="cuda"):
        log.append(("voxel", uid, origin_of(rows), rows.shape[0], floor, device, voxel_size))
        return rows[:-DROP_VOXEL]

    def filter_rows(xyz, k, std_ratio, n_points, uid, device="cuda"):
        log.append(("outliers", uid, origin_of(xyz), xyz.shape[0], n_points, device))
        return xyz[:-DROP_OUTLIERS]

    def split_rows(xyz, radius, min_points, mode, uid, device="cuda"):
        log.append(("cluster", uid, origin_of(xyz), xyz.shape[0], None, device))
        half = xyz.shape[0] // 2
        return [np.arange(half), np.arange(half, xyz.shape[0] - DROP_CLUSTER)][:2 if mode == "split" else 1]

    def upsample_rows(rows, radius, target, uid, device="cuda"):
        log.append(("upsample", uid, origin_of(rows), rows.shape[0], target, device))
        return rows if rows.shape[0] >= target else np.concatenate([rows, rows[np.arange(target - rows.shape[0]) % rows.shape[0]]])

    def fps_rows(xyz, n_points, device="cuda"):
        log.append(("pick", None, origin_of(xyz), xyz.shape[0], n_points, device))
        return np.arange(n_points) % xyz.shape[0]

    def xyz_to_pc_normal(xyz, n_points=4096, k=16, device="cuda", sampling="random"):
        log.append(("pick", None, origin_of(xyz), xyz.shape[0], n_points, device))
        return np.concatenate([xyz[np.arange(n_points) % xyz.shape[0], :3], np.tile(np.float32([0, 0, 1]), (n_points, 1))], axis=1)

    for module, fn in ((pc_voxel, thin_rows), (pc_outliers, filter_rows), (pc_cluster, split_rows), (pc_upsample, upsample_rows), (pc_fps, fps_rows),
                       (pc_normals, xyz_to_pc_normal)):
        monkeypatch.setattr(module, fn.__name__, fn)
    return log


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two files of 20 000 and 18 000 rows: column 0 = the row, column 1 = the file, unit normals"""
    d = tmp_path_factory.mktemp("voxel_prep")
    paths = []
    for f, (name, n) in enumerate((("first", 20000), ("second", 18000))):
        rows = np.zeros((n, 6), np.float32)
        rows[:, 0], rows[:, 1], rows[:, 5] = np.arange(n), f, 1.0
        paths.append(str(d / f"{name}.npy"))
        np.save(paths[-1], rows)
    return paths


def test_voxel_is_the_first_stage():
    assert cloud_prep.STAGES[0].switch == "voxel_size" and cloud_prep.STAGES[0].module == "pc_voxel"
    assert [s.switch for s in cloud_prep.STAGES[1:]] == ["outlier_k", "plane_threshold", "cluster_radius", "smooth_radius", "upsample_radius"]
    assert cloud_prep.CloudPrep().voxel_size == 0.0 and [s.switch for s, _ in cloud_prep.CloudPrep(voxel_size=0.5).on()] == ["voxel_size"]


@pytest.mark.parametrize("mode", ["largest", "split"])
@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_voxel_runs_first_once_per_file_with_the_floor_and_the_device(kind, mode, calls, files):
    for upsample, device in ((False, None), (True, "cuda:3")):
        del calls[:]
        kw = dict(upsample_radius=0.1, cluster_min_points=MIN_ROWS) if upsample else {}
        ds = Dataset(kind, files, sample_device=device, point_sampling="fps", voxel_size=0.25, outlier_k=16, cluster_radius=0.1, cluster_mode=mode, **kw)
        floor, dev = (MIN_ROWS if upsample else N_POINTS), device or "cuda"
        want = []
        for f, (uid, n) in enumerate((("first", 20000), ("second", 18000))):
            want.append(("voxel", uid, (f, 0), n, floor, dev, 0.25))       # the whole file, before anything else, once
            n -= DROP_VOXEL
            want.append(("outliers", uid, (f, 0), n, floor, dev))
            n -= DROP_OUTLIERS
            want.append(("cluster", uid, (f, 0), n, None, dev))
            half = n // 2
            parts = [(uid, 0, half)] if mode == "largest" else [(f"{uid}_part0", 0, half), (f"{uid}_part1", half, n - DROP_CLUSTER - half)]
            if upsample:
                want += [("upsample", part, (f, start), m, 4 * N_POINTS, dev) for part, start, m in parts]
                parts = [(part, start, max(m, 4 * N_POINTS)) for part, start, m in parts]
            want += [("pick", None, (f, start), m, N_POINTS, dev) for _, start, m in parts]
        assert calls == want, (upsample, device)
        assert len(ds) == (2 if mode == "largest" else 4) and all(d["pc_normal"].shape == (N_POINTS, 6) for d in ds.data)


def test_voxel_alone_and_its_refusals(calls, files):
    ds = Dataset("pc_normal", files[:1], point_sampling="fps", voxel_size=2)
    assert [c[0] for c in calls] == ["voxel", "pick"] and calls[0][3:] == (20000, N_POINTS, "cuda", 2) and calls[1][3] == 20000 - DROP_VOXEL and len(ds) == 1
    with pytest.raises(ValueError, match="mesh"):
        Dataset("mesh", [], voxel_size=0.1)
    for kind in ("pc_normal", "pc_xyz"):
        for bad in (-1.0, float("nan"), float("inf"), "1"):
            with pytest.raises(ValueError, match="voxel_size"):
                Dataset(kind, files[:1], voxel_size=bad)


def test_thin_rows_prints_its_line_and_enforces_the_floor(monkeypatch, capsys):
    rows = np.arange(60, dtype=np.float32).reshape(10, 6)
    keep = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0, 0], bool)
    seen = []
    monkeypatch.setattr(pc_voxel, "voxel_keep", lambda xyz, leaf, device="cuda": (seen.append((xyz.shape, leaf, device)), (keep, 4))[1])
    out = pc_voxel.thin_rows(rows, 0.5, 4, "scan", device="cuda:1")
    assert _same(out, rows[keep]) and seen == [((10, 6), 0.5, "cuda:1")]
    assert capsys.readouterr().out == "scan: voxel grid kept 4 of 10 points (voxel_size 0.5)\n"
    with pytest.raises(ValueError, match="scan: only 4 of 10 points survive the voxel grid, fewer than the 5 the encoder takes"):
        pc_voxel.thin_rows(rows, 0.5, 5, "scan")


# ---- off ------------------------------------------------------------------------------------------------------------------------------------
def test_off_leaves_the_rng_and_the_imports_as_before(files):
    np.random.seed(11)
    plain = Dataset("pc_normal", files[:1])
    state_plain = np.random.get_state()
    np.random.seed(11)
    off = Dataset("pc_normal", files[:1], voxel_size=0.0)
    state_off = np.random.get_state()
    assert _same(plain.data[0]["pc_normal"], off.data[0]["pc_normal"])
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "import meshanything_amd.data as data\n"
            "assert len(data.Dataset('pc_normal', [sys.argv[2]], voxel_size=0.0)) == 1\n"
            "loaded = sorted(m for m in sys.modules if m.startswith('meshanything_amd.pc_'))\n"
            "assert not loaded and 'torch' not in sys.modules, loaded\n")
    r = subprocess.run([sys.executable, "-c", code, REPO, files[0]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ---- the pc_xyz row cap -----------------------------------------------------------------------------------------------------------------------
def test_pc_xyz_takes_more_than_2_22_rows_only_with_voxel_size(tmp_path, calls):
    n = (1 << 22) + 1
    rows = np.zeros((n, 3), np.float32)                              # 50 MB
    rows[:, 0] = np.arange(n)
    path = str(tmp_path / "dense.npy")
    np.save(path, rows)
    with pytest.raises(ValueError, match=r"a pc_xyz input may have at most 2\^22 points, got 4194305"):
        Dataset("pc_xyz", [path])
    ds = Dataset("pc_xyz", [path], voxel_size=0.5, point_sampling="fps")
    assert [c[0] for c in calls] == ["voxel", "pick"] and calls[0][3] == n and calls[1][3] == n - DROP_VOXEL and len(ds) == 1
    with pytest.raises(ValueError, match="at most 268435456 points with voxel thinning"):
        pc_normals.check_xyz(np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 28) + 1, 3), (0, 4)), 4096, 16, max_points=pc_voxel.MAX_POINTS)
    small = np.zeros((5000, 3), np.float32)
    assert pc_normals.check_xyz(small, 4096, 16) is small and pc_normals.check_xyz(small, 4096, 16, max_points=1 << 28) is small


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_command_line_flag(capsys):
    import main
    base = ["--input_path", "x.ply"]
    assert main.get_args(base + ["--input_type", "pc_xyz"]).voxel_size == 0.0
    assert main.get_args(base + ["--input_type", "pc_normal", "--voxel_size", "0.02"]).voxel_size == 0.02
    assert main.get_args(base + ["--input_type", "mesh", "--voxel_size", "0"]).voxel_size == 0.0
    a = main.get_args(base + ["--input_type", "pc_xyz", "--voxel_size", "0.5", "--outlier_k", "16"])
    assert cloud_prep.CloudPrep.from_args(a).voxel_size == 0.5 and cloud_prep.CloudPrep.from_args(a).outlier_k == 16
    for bad, word in [(["--input_type", "pc_xyz", "--voxel_size", "-0.1"], "--voxel_size must be finite and >= 0"),
                      (["--input_type", "pc_xyz", "--voxel_size", "nan"], "--voxel_size must be finite and >= 0"),
                      (["--input_type", "pc_normal", "--voxel_size", "inf"], "--voxel_size must be finite and >= 0"),
                      (["--input_type", "mesh", "--voxel_size", "0.1"], "--voxel_size applies to --input_type pc_normal and pc_xyz, not to mesh inputs")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    assert "--voxel_size" in capsys.readouterr().out and "--voxel_size" in main.__doc__ and ".ply" in main.__doc__


# ---- .ply point files ---------------------------------------------------------------------------------------------------------------------------
FORMATS = ("ascii", "binary_little_endian", "binary_big_endian")


@pytest.mark.parametrize("real", ["float", "double"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_ply_point_files(tmp_path, fmt, real):
    g = np.random.default_rng(1)
    xyz = g.uniform(-3, 3, (300, 3)).astype(np.float32 if real == "float" else np.float64)
    nrm = g.normal(size=(300, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(xyz.dtype)
    both = np.concatenate([xyz, nrm], 1)
    path = str(tmp_path / "scan.ply")
    for colours, faces in ((False, False), (True, True)):
        R.write_ply(path, fmt, xyz, nrm, real, colours=colours, faces=faces)
        assert _same(mesh_input.load_ply_points(path), xyz)          # the dtype the file declares, the bits it holds
        assert _same(mesh_input.load_ply_points(path, normals=True), both)
        if faces:                                                    # the mesh reader still reads the same file, through the shared header parse
            verts, tris = mesh_input.load_mesh(path)
            assert _same(verts, xyz.astype(np.float64)) and tris.tolist() == [[0, 1, 2], [0, 2, 3]]
    R.write_ply(path, fmt, xyz, None, real, faces=True)              # without normals
    assert _same(mesh_input.load_ply_points(path), xyz)
    with pytest.raises(ValueError, match="'nx'"):
        mesh_input.load_ply_points(path, normals=True)
    R.write_ply(path, fmt, xyz, nrm, real, leave_out=("y",))
    with pytest.raises(ValueError, match="'y'"):
        mesh_input.load_ply_points(path)
    R.write_ply(path, fmt, xyz, nrm, real, leave_out=("nz",))
    with pytest.raises(ValueError, match="'nz'"):
        mesh_input.load_ply_points(path, normals=True)
    assert _same(mesh_input.load_ply_points(path), xyz)


def test_ply_refusals_and_dataset(tmp_path, calls):
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"plx\nend_header\n")
    with pytest.raises(ValueError, match="not a PLY"):
        mesh_input.load_ply_points(str(bad))
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with pytest.raises(ValueError, match="no vertex element"):
        mesh_input.load_ply_points(str(bad))
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nend_header\n" + b"\0" * 59)
    with pytest.raises(ValueError, match="ends before"):
        mesh_input.load_ply_points(str(bad))
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty int x\nproperty int y\nproperty int z\nend_header\n1 2 3\n")
    with pytest.raises(ValueError, match="float or double"):
        mesh_input.load_ply_points(str(bad))
    # through Dataset: both cloud types read a .ply, and the voxel stage sees the file's rows
    n = 6000
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0], rows[:, 5] = np.arange(n), 1.0
    path = str(tmp_path / "scan.ply")
    R.write_ply(path, "binary_little_endian", rows[:, :3], rows[:, 3:], colours=True, faces=True)
    np.random.seed(4)
    got = Dataset("pc_normal", [path]).data[0]["pc_normal"]
    np.random.seed(4)
    assert _same(got, rows[np.random.choice(n, N_POINTS, replace=False)])
    for kind in ("pc_normal", "pc_xyz"):
        del calls[:]
        ds = Dataset(kind, [path], voxel_size=0.5, point_sampling="fps")
        assert [c[:4] for c in calls] == [("voxel", "scan", (0, 0), n), ("pick", None, (0, 0), n - DROP_VOXEL)] and ds.data[0]["uid"] == "scan"
    assert calls[0][3] == n
