"""Smoothing of input clouds (`--smooth_radius`, meshanything_amd/pc_smooth.py) without a GPU: the numpy restatement's own properties
(tests/pc_smooth_ref.py), its two summation orders against each other, every refusal that comes before the first device call, the C
ABI's argument checks, `Dataset` with the step off, and the command line's new flags."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import pc_normals_ref as PN
import pc_smooth_ref as SR

REPO = SR.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, pc_smooth              # noqa: E402
from meshanything_amd.data import Dataset                        # noqa: E402


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_one_pass_more_than_halves_the_noise_on_the_sphere():
    """RMS distance to the unit sphere after one pass at R = 0.2 below 0.6 of the RMS before: 0.00448 against 0.00997, ratio 0.449.
    The figure includes the inward bias of a plane fit, R^2 / (8 * 1) = 0.005 at the rim weight 0: the mean radius becomes 0.9967."""
    p, true = SR.noisy_sphere()
    assert p.shape == (3000, 3) and p.dtype == np.float32
    got = SR.reference("n3000_ld3")
    before = np.sqrt(((np.linalg.norm(p.astype(np.float64), axis=1) - 1.0) ** 2).mean())
    radii = np.linalg.norm(got["moved"], axis=1)
    after = np.sqrt(((radii - 1.0) ** 2).mean())
    cos = np.abs(np.einsum("ij,ij->i", got["normals"], true))
    print(f"sphere: rms {before:.5f} -> {after:.5f} (ratio {after / before:.3f}), mean radius {radii.mean():.4f}, |cos| min {cos.min():.3f} mean {cos.mean():.4f}")
    assert 0.009 < before < 0.011 and after < 0.6 * before
    assert 0.99 < radii.mean() < 1.0                                 # shrunk, by less than R^2 / 8
    assert cos.min() > 0.95 and cos.mean() > 0.995
    assert np.abs(np.linalg.norm(got["normals"], axis=1) - 1).max() < 1e-14
    assert (np.linalg.norm(got["moved"] - p, axis=1) <= SR.SPHERE_RADIUS).all()


@pytest.mark.parametrize("name", ["n3000_ld3", "cube"])
def test_the_two_summation_orders_agree(name):
    """Every term is the same float64 number in both orders; a sum of at most 50 of them differs by at most 50 * 2^-53 = 5.6e-15 of the sum
    of their magnitudes, and a gap ratio of 0.05 or more amplifies that by at most 1 / 0.05 in the normal: below 1e-12, the floor of the
    GPU tolerance, with room to spare.  Measured: sphere 7.9e-16 / 8.6e-16 / 1.4e-15, cube 8.9e-16 / 1.8e-15 / 1.9e-15 (moved / R, sine,
    eigenvalues)."""
    a, b = SR.reference(name), SR.reference(name, True)
    assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["count"], SR.count_ref(*SR.count_cases()[name][:2]))
    assert a["count"].min() >= 12                                    # no row of either cloud lacks neighbours
    assert SR.well_posed(a).all()                                    # and the restatement leaves no row out
    spread = SR.spread(name)
    print(f"{name}: spread between the two orders {spread[0]:.2e} (moved / R), {spread[1]:.2e} (sine), {spread[2]:.2e} (eigenvalues)")
    assert max(spread) < 1e-13
    assert SR.tolerance(name) == (1e-12, 1e-12, 1e-12)


def test_the_rim_weight_is_zero_and_ties_count():
    cloud, radius, _ = SR.count_cases()["lattice_1"]
    got = SR.reference("lattice_1")
    inner = ((cloud >= 1) & (cloud <= 6)).all(1)
    assert (got["count"][inner] == 7).all() and got["count"].min() == 4          # the six neighbours' keys EQUAL r2: equality counts
    assert np.array_equal(got["moved"], cloud.astype(np.float64))               # ... and their weight is 0: nothing moves
    assert (got["eigvals"] == 0).all()
    assert SR.count_ref(cloud, np.nextafter(np.float32(1), np.float32(0))).max() == 1
    two = SR.reference("lattice_2")
    assert two["count"].max() == 33 and np.isfinite(two["moved"]).all()          # 1 + 6 + 12 + 8 + 6, the last six on the rim
    few = SR.smooth_ref(cloud[:5], 1.0)
    assert (few["count"] < 6).all() and np.array_equal(few["moved"], cloud[:5].astype(np.float64)) and (few["normals"] == (0, 0, 1)).all()
    tripled, radius, _ = SR.count_cases()["tripled"]
    t = SR.reference("tripled")
    assert np.array_equal(t["count"][:600], t["count"][600:1200]) and (t["count"] % 3 == 0).all()
    alone = SR.smooth_ref(np.zeros((9, 3), np.float32) + 0.25, 0.1)             # coincident neighbours: no plane
    assert (alone["count"] == 9).all() and (alone["moved"] == 0.25).all() and (alone["eigvals"] == 0).all()


# ---- refusals before the first device call ----------------------------------------------------------------------------------------------------
def test_smooth_points_refusals_come_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    for bad, radius, kw in [(pts.double(), 0.1, {}), (torch.zeros((100, 4)), 0.1, {}), (torch.zeros(100), 0.1, {}), (np.zeros((100, 3), np.float32), 0.1, {}),
                            (pts[:0], 0.1, {}), (pts, 0.0, {}), (pts, -0.1, {}), (pts, float("nan"), {}), (pts, float("inf"), {}), (pts, "0.1", {}),
                            (pts, True, {}), (pts, 0.1, {"want": ()}), (pts, 0.1, {"want": ("moved", "labels")}), (pts, 0.1, {"max_pairs": 0}),
                            (pts, 0.1, {"max_pairs": 1.5}), (pts, 0.1, {"max_pairs": 1 << 64}), (pts, 0.1, {"min_count": 2}), (pts, 0.1, {"min_count": 6.0}),
                            (pts, 0.1, {"min_count": True}), (pts, 0.1, {"grid": (np.zeros(3), 0.0, (1, 1, 1))}),
                            (pts, 0.1, {"grid": (np.zeros(3), 1.0, (129, 1, 1))}), (pts, 0.1, {"grid": 7}),
                            (pts, 2.01, {"grid": (np.zeros(3), 0.25, (8, 8, 8))})]:             # radius / cell > 8
        with pytest.raises(ValueError):
            pc_smooth.smooth_points(bad, radius, **kw)
    grid = (np.zeros(3, np.float32), np.float32(1.0), np.ones(3, np.int32))
    for kw in ({}, {"grid": grid}, {"want": "count"}, {"want": pc_smooth.WANT}, {"max_pairs": 1000}, {"min_count": 3}):
        with pytest.raises(ValueError, match="CUDA tensor"):         # a valid call stops at the device check: no CPU fallback
            pc_smooth.smooth_points(pts, 0.1, **kw)


def test_smooth_rows_checks_its_arguments_first():
    good = np.zeros((5000, 3), np.float32)
    nan = good.copy()
    nan[17, 1] = np.nan
    for bad, kw in [(np.zeros((5000, 2), np.float32), {}), (np.zeros(5000, np.float32), {}), (np.zeros((5000, 3), np.int32), {}), (nan, {}),
                    (good[:0], {}), (good, {"radius": 0.0}), (good, {"radius": float("nan")}), (good, {"iters": 0}), (good, {"iters": 9}),
                    (good, {"iters": 1.0}), (good, {"iters": True}),
                    (np.lib.stride_tricks.as_strided(np.zeros(3, np.float32), ((1 << 22) + 1, 3), (0, 4)), {})]:
        args = dict(radius=0.1, iters=1, uid="x")
        args.update(kw)
        with pytest.raises(ValueError):
            pc_smooth.smooth_rows(bad, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_smooth.smooth_rows(good, 0.1, 2, "x", device="cpu")
    assert pc_smooth.check_smooth_args(np.float32(0.5), np.int64(8)) == (0.5, 8)
    for radius, iters in [(0.0, 1), (-1.0, 1), (float("inf"), 1), ("1", 1), (0.1, 0), (0.1, 9), (0.1, "2")]:
        with pytest.raises(ValueError):
            pc_smooth.check_smooth_args(radius, iters)


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    size = lib.ma_pc_smooth_workspace_bytes
    assert size(4096, 4, 5, 6) == lib.ma_pc_knn_grid_workspace_bytes(4096, 16, 4, 5, 6) + 256      # the grid's layout and the total
    assert size(1, 1, 1, 1) > 0 and size(1 << 22, 128, 128, 128) < 120 << 20
    for N, nx, ny, nz in [(0, 1, 1, 1), ((1 << 22) + 1, 1, 1, 1), (100, 0, 1, 1), (100, 1, 129, 1), (100, 128, 128, 129), (100, 1, 1, -1)]:
        assert size(N, nx, ny, nz) == 0, (N, nx, ny, nz)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    origin, dims, big = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4), 1 << 40
    bound = C.c_uint64(7)

    def bad(word, *args):
        assert lib.ma_op_pc_smooth(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_smooth:") and word in msg, msg
        assert bound.value == 7                                      # no bound was computed

    out = (p, p, p, p)
    bad("null", None, 100, 3, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, None, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, origin, 1.0, None, 6, 0, *out, C.byref(bound), p, big, None)
    bad("null", p, 100, 3, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), None, big, None)
    bad("no output", p, 100, 3, 0.5, origin, 1.0, dims, 6, 0, None, None, None, None, C.byref(bound), p, big, None)
    bad("1 <= N", p, 0, 3, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("2^22", p, (1 << 22) + 1, 3, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("dim", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(4, 129, 4), 6, 0, *out, C.byref(bound), p, big, None)
    bad("dim", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(4, 0, 4), 6, 0, *out, C.byref(bound), p, big, None)
    bad("cells", p, 100, 3, 0.5, origin, 1.0, (C.c_int32 * 3)(128, 128, 129), 6, 0, *out, C.byref(bound), p, big, None)
    bad("ref_ld", p, 100, 4, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        bad("radius", p, 100, 3, radius, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    for min_count in (2, 0, -5):
        bad("min_count", p, 100, 3, 0.5, origin, 1.0, dims, min_count, 0, *out, C.byref(bound), p, big, None)
    bad("origin", p, 100, 3, 0.5, (C.c_float * 3)(0, float("nan"), 0), 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("cell", p, 100, 3, 0.5, origin, 0.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("cell", p, 100, 3, 0.5, origin, float("inf"), dims, 6, 0, *out, C.byref(bound), p, big, None)
    bad("radius / cell", p, 100, 3, 8.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, big, None)
    # faces that coincide in float32 (an origin huge against the cell): the pair bound would not hold, refused on the host
    bad("faces", p, 100, 3, 1e-3, (C.c_float * 3)(1e6, 0, 0), 1e-3, (C.c_int32 * 3)(64, 4, 4), 6, 0, *out, C.byref(bound), p, big, None)
    bad("workspace", p, 100, 3, 0.5, origin, 1.0, dims, 6, 0, *out, C.byref(bound), p, size(100, 4, 4, 4) - 1, None)


# ---- the input side and the command line ------------------------------------------------------------------------------------------------------
def _sphere_file(tmp_path):
    p, n = PN.sphere(5000, seed=2)
    path = str(tmp_path / "sphere.npy")
    np.save(path, np.concatenate([p, n.astype(np.float32)], 1))
    return path


def test_dataset_with_smoothing_off_is_todays(tmp_path, capsys):
    path = _sphere_file(tmp_path)
    np.random.seed(11)
    plain = Dataset("pc_normal", [path])
    state_plain = np.random.get_state()
    said_plain = capsys.readouterr().out
    np.random.seed(11)
    off = Dataset("pc_normal", [path], smooth_radius=0.0, smooth_iters=5)
    state_off = np.random.get_state()
    assert capsys.readouterr().out == said_plain and "smoothing" not in said_plain
    assert plain.data[0]["pc_normal"].tobytes() == off.data[0]["pc_normal"].tobytes()
    assert plain[0]["pc_normal"].tobytes() == off[0]["pc_normal"].tobytes() and plain[0]["uid"] == off[0]["uid"]
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    assert sorted(off.data[0]) == ["pc_normal", "uid"] and sorted(off[0]) == ["pc_normal", "uid"] and off.groups() == [0]


def test_dataset_refusals(tmp_path):
    path = _sphere_file(tmp_path)
    with pytest.raises(ValueError, match="smooth_radius applies to pc_normal and pc_xyz"):
        Dataset("mesh", [], smooth_radius=0.1)
    missing = str(tmp_path / "no_such_file.npy")                     # checked before any file is read
    for kind in ("pc_normal", "pc_xyz"):
        for kw in ({"smooth_radius": -0.1}, {"smooth_radius": float("nan")}, {"smooth_radius": float("inf")}, {"smooth_radius": 0.1, "smooth_iters": 0},
                   {"smooth_radius": 0.1, "smooth_iters": 9}, {"smooth_radius": 0.1, "smooth_iters": 1.5}):
            with pytest.raises(ValueError):
                Dataset(kind, [missing], **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            Dataset(kind, [path], smooth_radius=0.1, sample_device="cpu")


def test_command_line_flags(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert a.smooth_radius == 0.0 and a.smooth_iters == 1
    a = main.get_args(base + ["--input_type", "pc_normal", "--smooth_radius", "0.2", "--smooth_iters", "3"])
    assert a.smooth_radius == 0.2 and a.smooth_iters == 3
    assert main.get_args(base + ["--input_type", "pc_xyz", "--smooth_radius", "2"]).smooth_iters == 1
    assert main.get_args(base + ["--input_type", "mesh", "--smooth_radius", "0"]).smooth_radius == 0.0
    for bad, word in [(["--input_type", "pc_xyz", "--smooth_radius", "-1"], "--smooth_radius"), (["--input_type", "pc_xyz", "--smooth_radius", "nan"], "--smooth_radius"),
                      (["--input_type", "pc_xyz", "--smooth_radius", "inf"], "--smooth_radius"),
                      (["--input_type", "pc_xyz", "--smooth_radius", "0.1", "--smooth_iters", "0"], "--smooth_iters must be in 1..8"),
                      (["--input_type", "pc_xyz", "--smooth_radius", "0.1", "--smooth_iters", "9"], "--smooth_iters must be in 1..8"),
                      (["--input_type", "pc_xyz", "--smooth_iters", "2"], "needs --smooth_radius"),
                      (["--input_type", "pc_normal", "--smooth_radius", "0", "--smooth_iters", "1"], "needs --smooth_radius"),
                      (["--input_type", "mesh", "--smooth_radius", "0.1"], "mesh"), (["--input_type", "mesh", "--smooth_iters", "1"], "mesh")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err
