"""Statistical outlier removal (`--outlier_k`, meshanything_amd/pc_outliers.py) without a GPU: the numpy restatement of the cell-grid
search (tests/pc_outliers_ref.py) against the brute force over the adversarial cases of the GPU tests, which checks the strict stop
rule before any kernel runs; what the filter removes from surfaces with strays; `choose_grid`; every refusal that comes before the
first device call; the command line's new flags; and that `outlier_k=0` leaves the numpy RNG as it was."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import pc_normals_ref as PN
import pc_outliers_ref as R

REPO = R.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, pc_common, pc_outliers             # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the grid search's restatement against the brute force ----------------------------------------------------------------------------
def _agrees(ref, k, origin, cell, dims):
    want = PN.knn_ref(ref, None, k)
    got = R.grid_knn_ref(ref, k, origin, cell, dims, return_rounds=True)
    assert np.array_equal(got[0], want[0]) and _same(got[1], want[1])
    return got[2]


@pytest.mark.parametrize("case", ["k3_n3_ld3_all", "k3_n4_ld6_all", "k8_n255_ld3_all", "k32_n257_ld6_all", "k16_n1025_ld3_all", "k8_n1025_ld6_all",
                                  "k32_n32_ld3_all", "k16_n17_ld6_all"])
def test_grid_search_equals_brute_force_on_every_grid(case):
    ref, _, k = PN.knn_cases()[case]
    grids = dict(R.uniform_grid_cases(ref), auto=pc_outliers.choose_grid(ref, k))
    early = 0
    for name, (origin, cell, dims) in grids.items():
        rounds = _agrees(ref, k, origin, cell, dims)
        early += int(name == "16x16x16" and ref.shape[0] >= 255 and rounds.max() < 16)
        assert rounds.min() >= 1 and rounds.max() <= max(dims)
    if ref.shape[0] >= 255:
        assert early == 1                                            # the stop rule did end searches before the block was the whole grid


@pytest.mark.parametrize("cell", [1 / 8, 1 / 16])
@pytest.mark.parametrize("k", [8, 32])
def test_points_exactly_on_faces(cell, k):
    lat = PN.lattice(10)
    dims = (10, 10, 10) if cell == 1 / 8 else (20, 20, 20)
    f = R.faces(0.0, cell, dims[0])
    assert np.isin(lat[:, 0], f).all()                               # every coordinate is a face
    rounds = _agrees(lat, k, (0.0, 0.0, 0.0), cell, dims)
    assert rounds.max() < dims[0]


def test_duplicates_where_only_the_index_decides():
    _agrees(PN.tripled(400, seed=4), 8, (-1.0, -1.0, -1.0), 0.25, (8, 8, 8))
    p = R.repeated_point()
    for grid in (((-1.0, -1.0, -1.0), 0.25, (8, 8, 8)), pc_outliers.choose_grid(p, 32)):
        _agrees(p, 32, *grid)
    idx, d2 = PN.knn_ref(p, None, 32)
    copies = np.flatnonzero(d2[:, 31] == 0)
    assert copies.shape[0] == 40 and np.array_equal(idx[copies[0]], copies[:32].astype(np.int32))   # the k-th key is 0: the 32 lowest indices


def test_noisy_sphere_with_the_automatic_grid():
    xyz, _, stray = R.noisy("sphere", 2500 - 50, 50, 5)
    origin, cell, dims = pc_outliers.choose_grid(xyz, 16)
    assert (np.abs(xyz[stray]).max(1) > 1.1).any() and float((origin + cell).min()) > -1.2   # before the widening the box follows the sphere, strays fall outside it
    _agrees(xyz, 16, origin, cell, dims)


# ---- what the filter removes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PN.CLOUDS))
def test_filter_removes_strays_and_no_surface_point(name):
    xyz, _, stray = R.noisy(name, 12000, 120, 3)
    assert stray.sum() == 120 and xyz.shape == (12120, 3)
    for k in (8, 16):
        for r in (1, 2, 3):
            keep, m, T = R.sor_of_noisy(name, 12000, 120, 3, k, float(r))
            removed = int((~keep & stray).sum())
            margin = float((np.abs(m - T) / T).min())
            print(f"{name} k={k} r={r}: {removed} of 120 strays removed, {int((~keep & ~stray).sum())} surface points, nearest |m - T| / T = {margin:.3g}")
            assert not (~keep & ~stray).any()
            assert removed >= 107
            assert margin > 1e-3
    if name == "sphere":
        keep, _, _ = R.sor_of_noisy(name, 12000, 120, 3, 16, 2.0)
        assert int((~keep).sum()) == 111


def test_mean_dist_ref_sums_in_list_order():
    d2 = np.array([[0.0, 1.0, 4.0], [0.0, 0.25, 2.25]], np.float32)
    assert np.array_equal(R.mean_dist_ref(d2), np.array([1.0, 2.0 / 3.0]))


# ---- choose_grid ----------------------------------------------------------------------------------------------------------------------
def test_choose_grid_is_deterministic_and_within_the_limits():
    g = np.random.default_rng(0)
    clouds = [R.noisy("sphere", 12000, 120, 3)[0], PN.lattice(10), np.zeros((100, 3), np.float32), g.uniform(-1, 1, (3, 3)).astype(np.float32),
              (g.uniform(-1, 1, (200000, 3)) * [5.0, 0.01, 1.0]).astype(np.float32), g.uniform(1e6, 1e6 + 1, (5000, 6)), np.full((50, 3), 1e30, np.float32)]
    for xyz in clouds:
        origin, cell, dims = pc_outliers.choose_grid(xyz, 16)
        again = pc_outliers.choose_grid(xyz.copy(), 16)
        assert origin.dtype == np.float32 and origin.shape == (3,) and dims.dtype == np.int32 and dims.shape == (3,) and isinstance(cell, np.float32)
        assert _same(origin, again[0]) and cell == again[1] and _same(dims, again[2])
        assert np.isfinite(origin).all() and np.isfinite(cell) and cell > 0
        assert (dims >= 1).all() and (dims <= 128).all() and int(np.prod(dims.astype(np.int64))) <= 1 << 21
        pc_common.check_grid((origin, cell, dims))
    origin, cell, dims = pc_outliers.choose_grid(clouds[0], 16)
    assert abs(int(dims.max()) - round(np.sqrt(12120 / 256))) <= 1 and abs(float(cell) * (round(np.sqrt(12120 / 256)) - 2) - 2.0) < 0.1   # fitted to the sphere, not to [-2, 2]^3
    assert abs(pc_outliers.choose_grid(clouds[4], 16)[2].tolist()[0] - round(np.sqrt(200000 / 256))) <= 1
    big = np.resize(clouds[0], (1 << 22, 3))                         # the cloud over and over, 2^22 rows: the cap of 128
    assert pc_outliers.choose_grid(big, 16)[2].max() == 128
    assert pc_outliers.choose_grid(clouds[0], 16, along=64)[2].max() in (64, 65)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    pc_outliers.choose_grid(clouds[0], 16)
    assert np.array_equal(np.random.get_state()[1], before)


# ---- refusals before the first device call --------------------------------------------------------------------------------------------
def test_python_refusals_come_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    grid = (np.zeros(3, np.float32), np.float32(1.0), np.ones(3, np.int32))
    for bad, kw in [(pts.double(), {}), (torch.zeros((100, 4)), {}), (torch.zeros(100), {}), (np.zeros((100, 3), np.float32), {}), (pts, {"k": 2}),
                    (pts, {"k": 33}), (pts, {"k": 16.5}), (pts, {"k": True}), (pts[:10], {"k": 16}), (pts, {"want": ()}), (pts, {"want": ("idx", "normals")}),
                    (pts, {"grid": (np.zeros(3), 0.0, (1, 1, 1))}), (pts, {"grid": (np.zeros(3), float("nan"), (1, 1, 1))}),
                    (pts, {"grid": (np.zeros(2), 1.0, (1, 1, 1))}), (pts, {"grid": ([0, 0, float("inf")], 1.0, (1, 1, 1))}),
                    (pts, {"grid": (np.zeros(3), 1.0, (129, 1, 1))}), (pts, {"grid": (np.zeros(3), 1.0, (0, 1, 1))}),
                    (pts, {"grid": (np.zeros(3), 1.0, (128, 128, 129))}), (pts, {"grid": (np.zeros(3), 1.0, (1.5, 1, 1))}), (pts, {"grid": 7})]:
        with pytest.raises(ValueError):
            pc_outliers.grid_knn(bad, **kw)
    with pytest.raises(ValueError, match="CUDA tensor"):             # a valid call stops at the device check: no CPU fallback
        pc_outliers.grid_knn(pts, 16, grid)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pc_outliers.grid_knn(pts, 16, None, want="mean")
    for kw in ({"form": 3}, {"form": -1}, {"form": True}, {"form": 1.0}, {"k": 2}):
        with pytest.raises(ValueError):
            pc_outliers.knn_mean_distance(pts, **kw)
    for form in (0, 1, 2):
        with pytest.raises(ValueError, match="CUDA tensor"):
            pc_outliers.knn_mean_distance(pts, 16, form)
    assert pc_outliers.resolve_form(100, 1) == 1 and pc_outliers.resolve_form(1 << 22, 2) == 2
    assert {pc_outliers.resolve_form(n, 0) for n in (16, 1 << 22)} <= {1, 2} and pc_outliers.resolve_form(1 << 22, 0) == 2
    assert pc_outliers.resolve_form(pc_outliers.GRID_FROM_N, 0) == 2 and pc_outliers.resolve_form(pc_outliers.GRID_FROM_N - 1, 0) == 1


def test_remove_statistical_outliers_checks_its_arguments_first():
    good = np.zeros((5000, 3), np.float32)
    nan = good.copy()
    nan[17, 1] = np.nan
    for bad, kw in [(np.zeros((5000, 2), np.float32), {}), (np.zeros(5000, np.float32), {}), (np.zeros((5000, 3), np.int32), {}), (nan, {}),
                    (good, {"k": 2}), (good, {"k": 33}), (good[:10], {"k": 16}), (good, {"std_ratio": -0.5}), (good, {"std_ratio": float("nan")}),
                    (good, {"std_ratio": float("inf")}), (good, {"std_ratio": "2"}), (good, {"form": 5}),
                    (np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 22) + 1, 3), (0, 4)), {}),
                    (np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 20) + 1, 3), (0, 4)), {"form": 1})]:
        with pytest.raises(ValueError):
            pc_outliers.remove_statistical_outliers(bad, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_outliers.remove_statistical_outliers(good, device="cpu")
    wide = np.concatenate([good, np.full((5000, 3), np.inf, np.float32)], 1)
    assert pc_outliers.check_outlier_args(wide, 16, 0.0) is wide     # columns after the third are not read; std_ratio 0 is allowed


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    a256 = lambda n: (n + 255) // 256 * 256                          # noqa: E731
    size = lib.ma_pc_knn_grid_workspace_bytes
    assert size(4096, 16, 4, 5, 6) == a256(4096 * 4) + a256(120 * 4) + a256(121 * 4) + a256(1024 * 4) + a256(4096 * 16)
    assert size(4096, 3, 4, 5, 6) == size(4096, 32, 4, 5, 6)         # the lists live in registers: k does not enter
    assert size(1 << 22, 32, 128, 128, 128) < 100 << 20              # 2^22 points over 2^21 cells: 96 MB and change, no (N, k) lists
    for N, k, nx, ny, nz in [(15, 16, 1, 1, 1), ((1 << 22) + 1, 16, 1, 1, 1), (100, 2, 1, 1, 1), (100, 33, 1, 1, 1), (100, 16, 0, 1, 1), (100, 16, 1, 129, 1),
                             (100, 16, 128, 128, 129), (100, 16, 1, 1, -1)]:
        assert size(N, k, nx, ny, nz) == 0, (N, k, nx, ny, nz)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    origin, dims, big = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4), 1 << 40

    def bad(word, *args):
        assert lib.ma_op_pc_knn_grid(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_knn_grid:") and word in msg, msg

    bad("null", None, 100, 3, 16, origin, 1.0, dims, p, p, p, p, big, None)
    bad("null", p, 100, 3, 16, None, 1.0, dims, p, p, p, p, big, None)
    bad("null", p, 100, 3, 16, origin, 1.0, None, p, p, p, p, big, None)
    bad("null", p, 100, 3, 16, origin, 1.0, dims, p, p, p, None, big, None)
    bad("at least one", p, 100, 3, 16, origin, 1.0, dims, None, None, None, p, big, None)
    bad("k <= N", p, 15, 3, 16, origin, 1.0, dims, p, p, p, p, big, None)
    bad("k <= N", p, 100, 3, 33, origin, 1.0, dims, p, p, p, p, big, None)
    bad("2^22", p, (1 << 22) + 1, 3, 16, origin, 1.0, dims, p, p, p, p, big, None)
    bad("dim", p, 100, 3, 16, origin, 1.0, (C.c_int32 * 3)(4, 129, 4), p, p, p, p, big, None)
    bad("dim", p, 100, 3, 16, origin, 1.0, (C.c_int32 * 3)(4, 0, 4), p, p, p, p, big, None)
    bad("cells", p, 100, 3, 16, origin, 1.0, (C.c_int32 * 3)(128, 128, 129), p, p, p, p, big, None)
    bad("ref_ld", p, 100, 4, 16, origin, 1.0, dims, p, p, p, p, big, None)
    bad("origin", p, 100, 3, 16, (C.c_float * 3)(0, float("nan"), 0), 1.0, dims, p, p, p, p, big, None)
    bad("cell", p, 100, 3, 16, origin, 0.0, dims, p, p, p, p, big, None)
    bad("cell", p, 100, 3, 16, origin, float("inf"), dims, p, p, p, p, big, None)
    bad("workspace", p, 100, 3, 16, origin, 1.0, dims, p, p, p, p, size(100, 16, 4, 4, 4) - 1, None)


# ---- the input side and the command line ----------------------------------------------------------------------------------------------
def test_dataset_with_the_filter_off_consumes_the_rng_as_before(tmp_path):
    p, n = PN.sphere(5000, seed=2)
    path = str(tmp_path / "sphere.npy")
    np.save(path, np.concatenate([p, n.astype(np.float32)], 1))
    np.random.seed(11)
    plain = Dataset("pc_normal", [path])
    state_plain = np.random.get_state()
    np.random.seed(11)
    off = Dataset("pc_normal", [path], outlier_k=0, outlier_std=7.0)
    state_off = np.random.get_state()
    assert _same(plain.data[0]["pc_normal"], off.data[0]["pc_normal"])
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]


def test_dataset_refusals(tmp_path):
    p, n = PN.sphere(5000, seed=2)
    path = str(tmp_path / "sphere.npy")
    np.save(path, np.concatenate([p, n.astype(np.float32)], 1))
    with pytest.raises(ValueError, match="mesh"):
        Dataset("mesh", [], outlier_k=16)
    for kind in ("pc_normal", "pc_xyz"):
        for kw in ({"outlier_k": 2}, {"outlier_k": 33}, {"outlier_k": 16, "outlier_std": -1.0}, {"outlier_k": 16, "outlier_std": float("nan")}):
            with pytest.raises(ValueError):
                Dataset(kind, [path], **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            Dataset(kind, [path], outlier_k=16, sample_device="cpu")


def test_command_line_flags(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert a.outlier_k == 0 and a.outlier_std == 2.0
    a = main.get_args(base + ["--input_type", "pc_normal", "--outlier_k", "16", "--outlier_std", "1.5", "--point_sampling", "fps"])
    assert a.outlier_k == 16 and a.outlier_std == 1.5
    assert main.get_args(base + ["--input_type", "pc_xyz", "--outlier_k", "3", "--outlier_std", "0"]).outlier_k == 3
    assert main.get_args(base + ["--input_type", "mesh", "--outlier_k", "0"]).outlier_k == 0
    for bad, word in [(["--input_type", "pc_xyz", "--outlier_k", "2"], "--outlier_k"), (["--input_type", "pc_xyz", "--outlier_k", "33"], "--outlier_k"),
                      (["--input_type", "pc_xyz", "--outlier_k", "-1"], "--outlier_k"), (["--input_type", "mesh", "--outlier_k", "16"], "mesh"),
                      (["--input_type", "pc_xyz", "--outlier_k", "16", "--outlier_std", "-1"], "--outlier_std"),
                      (["--input_type", "pc_xyz", "--outlier_k", "16", "--outlier_std", "nan"], "--outlier_std"),
                      (["--input_type", "pc_xyz", "--outlier_std", "inf"], "--outlier_std")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err
