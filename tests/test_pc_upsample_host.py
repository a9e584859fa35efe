"""Upsampling of sparse input clouds (`--upsample_radius`, meshanything_amd/pc_upsample.py) without a GPU: the numpy restatement
(tests/pc_upsample_ref.py) on a case derived by hand, the frame rule, every refusal that comes before the first device call, the C ABI's
argument checks, the ladder of `upsample_rows` with a faked counter, `Dataset` with the step off and its refusals, and the command
line's new flags."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import pc_normals_ref as PN
import pc_upsample_ref as UR

REPO = UR.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, pc_upsample            # noqa: E402
from meshanything_amd.data import Dataset                        # noqa: E402

# The rows (x, y, 0), x and y in 0..2, row 3x + y, normals (0, 0, 1), R = 1, m = 2: u = (1, 0, 0), v = (0, 1, 0), so candidate (a, b) of
# the seed at (x, y) lies at (x + a/2, y + b/2), a*a + b*b <= 4.  It is kept iff no other row is nearer and no row of lower index as near:
# a step of 1 lands on a row unless it leaves the lattice; a step of 1/2 lies midway between two rows and goes to the lower; a diagonal
# half step is the centre of four rows (or, outside the lattice, midway between two) and goes to the lowest.
HAND = [(0, -2, 0), (0, -1, -1), (0, -1, 0), (0, -1, 1), (0, 0, -2), (0, 0, -1), (0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1),
        (1, -2, 0), (1, -1, 0), (1, -1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1),
        (2, -2, 0), (2, -1, 0), (2, -1, 1), (2, 0, 1), (2, 0, 2), (2, 1, 0), (2, 1, 1),
        (3, 0, -2), (3, 0, -1), (3, 0, 1), (3, 1, -1), (3, 1, 0), (3, 1, 1),
        (4, 0, 1), (4, 1, 0), (4, 1, 1),
        (5, 0, 1), (5, 0, 2), (5, 1, 0), (5, 1, 1),
        (6, 0, -2), (6, 0, -1), (6, 0, 1), (6, 1, -1), (6, 1, 0), (6, 1, 1), (6, 2, 0),
        (7, 0, 1), (7, 1, 0), (7, 1, 1), (7, 2, 0),
        (8, 0, 1), (8, 0, 2), (8, 1, 0), (8, 1, 1), (8, 2, 0)]


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_restatement_on_the_three_by_three_lattice():
    rows = np.array([(x, y, 0) for x in range(3) for y in range(3)], np.float32)
    got = UR.upsample_ref(rows, np.tile([[0.0, 0.0, 1.0]], (9, 1)), 1.0, 2, with_ab=True)
    assert got["ab"] == HAND
    assert (4, 0, 1) in HAND and (5, 0, -1) not in HAND              # midway between rows 4 and 5: to the lower
    assert (0, 1, 1) in HAND and all((s, a, b) not in HAND for s, a, b in [(1, 1, -1), (3, -1, 1), (4, -1, -1)])   # the centre of rows 0 1 3 4
    assert (0, -1, 1) in HAND and (1, -1, -1) not in HAND            # outside the lattice, midway between rows 0 and 1
    assert got["counts"].tolist() == [10, 6, 7, 6, 3, 4, 7, 4, 5] and got["counts"].sum() == len(HAND)
    assert got["seed"].tolist() == [s for s, _, _ in HAND] and got["xyz"].dtype == np.float32 and got["seed"].dtype == np.int32
    want = np.array([(s // 3 + a / 2, s % 3 + b / 2, 0) for s, a, b in HAND], np.float32)
    assert np.array_equal(got["xyz"], want)
    # every candidate is given to at most one seed, and the patches cover each lattice point within reach at most once
    assert len({tuple(r) for r in got["xyz"].tolist()}) == len(HAND)
    off = UR.upsample_ref(rows, np.tile([[0.0, 0.0, 1.0]], (9, 1)), 1.0, 2, active=np.arange(9) != 4, with_ab=True)
    assert off["ab"] == [t for t in HAND if t[0] != 4]               # an inactive row seeds nothing and still owns its neighbourhood


def test_restatement_duplicates_and_non_finite_rows():
    rows = np.array([(0, 0, 0), (1, 0, 0), (0, 0, 0), (np.nan, 0, 0), (0.25, np.inf, 0)], np.float32)
    nrm = np.tile([[0.0, 0.0, 1.0]], (5, 1))
    nrm[1] = (np.nan, 0.0, 1.0)
    got = UR.upsample_ref(rows, nrm, 0.5, 1)
    # row 2 duplicates row 0 and gives it everything; (0.5, 0, 0) is a tie of rows 0 and 1, to row 0; row 1's normal is NaN; rows 3 and 4 are not finite
    assert got["counts"].tolist() == [4, 0, 0, 0, 0] and got["seed"].tolist() == [0, 0, 0, 0]
    assert got["xyz"].tolist() == [[-0.5, 0, 0], [0, -0.5, 0], [0, 0.5, 0], [0.5, 0, 0]]


def test_frame_rule():
    assert UR.frame_ref([0, 0, 1]) == ([1, 0, 0], [0, 1, 0])         # |n_x| = |n_y| = 0: the lowest axis
    assert UR.frame_ref([1, 0, 0]) == ([0, 1, 0], [0, 0, 1])         # |n_y| = |n_z|: y
    assert UR.frame_ref([0, 1, 0]) == ([1, 0, 0], [0, 0, -1])
    assert UR.frame_ref([0, 0, -1]) == ([1, 0, 0], [0, -1, 0])
    s = 1 / np.sqrt(3.0)
    u, v = UR.frame_ref([s, s, s])                                   # a three-way tie: x
    assert u[0] > 0 and u[1] == u[2] < 0 and abs(v[0]) < 1e-16 and v[1] == -v[2]
    u, v = UR.frame_ref([0.6, -0.48, 0.64])                          # the smallest magnitude decides, not the smallest value
    assert u[1] > 0.8
    g = np.random.default_rng(0)
    for n in UR.unit(g.normal(size=(50, 3))):
        u, v = (np.array(x) for x in UR.frame_ref(n))
        assert abs(np.linalg.norm(u) - 1) < 1e-15 and abs(np.linalg.norm(v) - 1) < 1e-15
        assert max(abs(u @ n), abs(v @ n), abs(u @ v)) < 1e-15
        assert np.abs(np.cross(u, v) - n).max() < 1e-15             # right-handed: u x v = n


def test_lattice_order_and_size():
    a, b = UR.lattice(1)
    assert list(zip(a.tolist(), b.tolist())) == [(-1, 0), (0, -1), (0, 1), (1, 0)]
    for m in (1, 2, 3, 8, 64):
        assert UR.lattice(m)[0].shape[0] == pc_upsample.lattice_size(m)
    assert pc_upsample.lattice_size(2) == 12 and pc_upsample.lattice_size(64) == 12852
    assert pc_upsample.LADDER == UR.LADDER == (2, 4, 8, 16, 32, 64) and pc_upsample.MIN_ROWS == 64 and pc_upsample.MAX_M == 64


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------
def test_the_ladder_takes_the_first_m_that_reaches_the_target():
    asked = []

    def count(m):
        asked.append(m)
        return 10 * m * m

    assert pc_upsample.choose_m(count, 1000, 4096, 0.1) == (32, 10240) and asked == [2, 4, 8, 16, 32]
    asked.clear()
    assert pc_upsample.choose_m(count, 1000, 1040, 0.1) == (2, 40) and asked == [2]          # N + total == target is enough
    asked.clear()
    assert pc_upsample.choose_m(count, 1000, 1041, 0.1) == (4, 160) and asked == [2, 4]
    asked.clear()
    with pytest.raises(ValueError, match=r"upsampling 1000 rows at radius 0\.1 reaches 41960 rows at m = 64, fewer than the 50000 asked for: use a larger radius"):
        pc_upsample.choose_m(count, 1000, 50000, 0.1)
    assert asked == [2, 4, 8, 16, 32, 64]
    asked.clear()
    with pytest.raises(ValueError, match="reaches 1000 rows at m = 64"):
        pc_upsample.choose_m(lambda m: 0, 1000, 4096, 0.1)
    # N * (2m+1)^2 <= 2^31 ends the ladder early: 2^20 rows allow m = 22 at the most
    with pytest.raises(ValueError, match="at m = 16"):
        pc_upsample.choose_m(count, 1 << 20, 1 << 22, 0.1)
    assert asked == [2, 4, 8, 16]


# ---- refusals before the first device call ----------------------------------------------------------------------------------------------------
def test_upsample_points_refusals_come_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    nrm = torch.zeros((100, 3), dtype=torch.float64)
    act = torch.ones(100, dtype=torch.bool)
    for p, n, radius, m, kw in [(pts.double(), nrm, 0.1, 2, {}), (torch.zeros((100, 4)), nrm, 0.1, 2, {}), (np.zeros((100, 3), np.float32), nrm, 0.1, 2, {}),
                                (pts[:0], nrm[:0], 0.1, 2, {}), (pts, nrm.float(), 0.1, 2, {}), (pts, nrm[:99], 0.1, 2, {}), (pts, nrm.numpy(), 0.1, 2, {}),
                                (pts, nrm, 0.0, 2, {}), (pts, nrm, float("nan"), 2, {}), (pts, nrm, float("inf"), 2, {}), (pts, nrm, "0.1", 2, {}),
                                (pts, nrm, 0.1, 0, {}), (pts, nrm, 0.1, 65, {}), (pts, nrm, 0.1, 2.0, {}), (pts, nrm, 0.1, True, {}),
                                (pts, nrm, 0.1, 2, {"active": act[:99]}), (pts, nrm, 0.1, 2, {"active": act.float()}), (pts, nrm, 0.1, 2, {"active": [1] * 100}),
                                (pts, nrm, 0.1, 2, {"capacity": -1}), (pts, nrm, 0.1, 2, {"capacity": (1 << 22) + 1}), (pts, nrm, 0.1, 2, {"capacity": 1.5}),
                                (pts, nrm, 0.1, 2, {"max_pairs": 0}), (pts, nrm, 0.1, 2, {"grid": (np.zeros(3), 0.0, (1, 1, 1))}), (pts, nrm, 0.1, 2, {"grid": 7}),
                                (pts, nrm, 2.01, 2, {"grid": (np.zeros(3), 0.25, (8, 8, 8))})]:          # radius / cell > 8
        with pytest.raises(ValueError):
            pc_upsample.upsample_points(p, n, radius, m, **kw)
    big = torch.zeros(3, dtype=torch.float32).as_strided(((1 << 20), 3), (0, 1))
    with pytest.raises(ValueError, match=r"N \* \(2m\+1\)\^2"):
        pc_upsample.upsample_points(big, torch.zeros(3, dtype=torch.float64).as_strided(((1 << 20), 3), (0, 1)), 0.1, 32)
    grid = (np.zeros(3, np.float32), np.float32(1.0), np.ones(3, np.int32))
    for kw in ({}, {"grid": grid}, {"active": act}, {"active": act.to(torch.uint8)}, {"count_only": True}, {"capacity": 10}, {"max_pairs": 1000}):
        with pytest.raises(ValueError, match="CUDA tensor"):         # a valid call stops at the device check: no CPU fallback
            pc_upsample.upsample_points(pts, nrm, 0.1, 2, **kw)


def test_upsample_rows_checks_its_arguments_first(capsys):
    good = np.zeros((1500, 3), np.float32)
    nan = good.copy()
    nan[17, 1] = np.nan
    for bad, kw in [(np.zeros((1500, 2), np.float32), {}), (np.zeros(1500, np.float32), {}), (np.zeros((1500, 3), np.int32), {}), (nan, {}), (good[:0], {}),
                    (good, {"radius": 0.0}), (good, {"radius": float("nan")}), (good, {"target": 4095}), (good, {"target": (1 << 22) + 1}),
                    (good, {"target": 8192.0}), (good, {"target": True})]:
        args = dict(radius=0.1, target=8192, uid="x")
        args.update(kw)
        with pytest.raises(ValueError):
            pc_upsample.upsample_rows(bad, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_upsample.upsample_rows(good, 0.1, 8192, "x", device="cpu")
    assert pc_upsample.check_upsample_args(np.float32(0.5), np.int64(4096)) == (0.5, 4096)
    assert pc_upsample.check_upsample_args(0.5, 1 << 22) == (0.5, 1 << 22) and pc_upsample.check_upsample_args(0.5, 100, 100) == (0.5, 100)
    for radius, target in [(0.0, 8192), (-1.0, 8192), (float("inf"), 8192), ("1", 8192), (0.1, 4095), (0.1, (1 << 22) + 1), (0.1, "8192")]:
        with pytest.raises(ValueError):
            pc_upsample.check_upsample_args(radius, target)


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    size = lib.ma_pc_upsample_workspace_bytes
    assert size(4096, 4, 5, 6) > lib.ma_pc_smooth_workspace_bytes(4096, 4, 5, 6) + 4097 * 8       # the smoothing layout, the offsets, the scan's tiles
    assert size(1, 1, 1, 1) > 0 and size(1 << 22, 128, 128, 128) < 160 << 20
    for N, nx, ny, nz in [(0, 1, 1, 1), ((1 << 22) + 1, 1, 1, 1), (100, 0, 1, 1), (100, 1, 129, 1), (100, 128, 128, 129), (100, 1, 1, -1)]:
        assert size(N, nx, ny, nz) == 0, (N, nx, ny, nz)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    origin, dims, big = (C.c_float * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4), 1 << 40
    total, bound = C.c_uint64(7), C.c_uint64(7)

    def bad(word, ref, N, ld, nrm, m, step, origin, cell, dims, xyz, seed, tot, ws, nbytes):
        assert lib.ma_op_pc_upsample(ref, N, ld, nrm, None, m, step, origin, cell, dims, 0, p, xyz, seed, 1000, tot, C.byref(bound), ws, nbytes, None) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_upsample:") and word in msg, msg
        assert bound.value == 7 and total.value == 7                 # nothing was computed

    ok = dict(ref=p, N=100, ld=3, nrm=p, m=2, step=0.25, origin=origin, cell=1.0, dims=dims, xyz=p, seed=p, tot=C.byref(total), ws=p, nbytes=big)
    for word, change in [("null", {"ref": None}), ("null", {"nrm": None}), ("null", {"origin": None}), ("null", {"dims": None}), ("null", {"tot": None}),
                         ("null", {"ws": None}), ("out_seed without out_xyz", {"xyz": None}), ("1 <= N", {"N": 0}), ("2^22", {"N": (1 << 22) + 1}),
                         ("dim", {"dims": (C.c_int32 * 3)(4, 129, 4)}), ("dim", {"dims": (C.c_int32 * 3)(4, 0, 4)}),
                         ("cells", {"dims": (C.c_int32 * 3)(128, 128, 129)}), ("ref_ld", {"ld": 2}), ("m must be in 1..64", {"m": 0}),
                         ("m must be in 1..64", {"m": 65}), ("2^31", {"N": 1 << 20, "m": 32}), ("step", {"step": 0.0}), ("step", {"step": -1.0}),
                         ("step", {"step": float("nan")}), ("step", {"step": float("inf")}), ("step", {"step": 1e300}), ("step", {"step": 1e-300}),
                         ("origin", {"origin": (C.c_float * 3)(0, float("nan"), 0)}), ("cell", {"cell": 0.0}), ("cell", {"cell": float("inf")}),
                         ("m * step / cell", {"step": 4.25}),
                         ("faces", {"step": 5e-4, "origin": (C.c_float * 3)(1e6, 0, 0), "cell": 1e-3, "dims": (C.c_int32 * 3)(64, 4, 4)}),
                         ("workspace", {"nbytes": size(100, 4, 4, 4) - 1})]:
        bad(word, **{**ok, **change})


# ---- the input side and the command line ------------------------------------------------------------------------------------------------------
def _sphere_file(tmp_path, n=5000):
    p, nrm = PN.sphere(n, seed=2)
    path = str(tmp_path / f"sphere{n}.npy")
    np.save(path, np.concatenate([p, nrm.astype(np.float32)], 1))
    return path


def test_dataset_with_upsampling_off_is_todays(tmp_path, capsys):
    path = _sphere_file(tmp_path)
    np.random.seed(11)
    plain = Dataset("pc_normal", [path])
    state_plain = np.random.get_state()
    said_plain = capsys.readouterr().out
    np.random.seed(11)
    off = Dataset("pc_normal", [path], upsample_radius=0.0)
    state_off = np.random.get_state()
    assert capsys.readouterr().out == said_plain and "upsampling" not in said_plain
    assert plain.data[0]["pc_normal"].tobytes() == off.data[0]["pc_normal"].tobytes()
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    assert sorted(off.data[0]) == ["pc_normal", "uid"] and sorted(off[0]) == ["pc_normal", "uid"] and off.groups() == [0]
    short = _sphere_file(tmp_path, 1500)                             # with the step off a short file is refused as before
    with pytest.raises(AssertionError, match="at least 4096 points"):
        Dataset("pc_normal", [short])
    with pytest.raises(ValueError, match="at least 4096 points"):
        Dataset("pc_xyz", [short])
    with pytest.raises(ValueError, match="cluster_min_points = 64 is less than the 4096 rows the encoder takes"):
        Dataset("pc_normal", [short], cluster_radius=0.1, cluster_min_points=64)


def test_dataset_refusals(tmp_path):
    path = _sphere_file(tmp_path, 1500)
    with pytest.raises(ValueError, match="upsample_radius applies to pc_normal and pc_xyz"):
        Dataset("mesh", [], upsample_radius=0.1)
    with pytest.raises(ValueError, match="upsample_points needs upsample_radius > 0"):
        Dataset("mesh", [], upsample_points=8192)
    missing = str(tmp_path / "no_such_file.npy")                     # checked before any file is read
    for kind in ("pc_normal", "pc_xyz"):
        for kw in ({"upsample_radius": -0.1}, {"upsample_radius": float("nan")}, {"upsample_radius": float("inf")}, {"upsample_points": 8192},
                   {"upsample_radius": 0.1, "upsample_points": 4095}, {"upsample_radius": 0.1, "upsample_points": (1 << 22) + 1},
                   {"upsample_radius": 0.1, "upsample_points": 8192.0},
                   {"upsample_radius": 0.1, "cluster_radius": 0.1, "cluster_min_points": 63}):
            with pytest.raises(ValueError):
                Dataset(kind, [missing], **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            Dataset(kind, [path], upsample_radius=0.1, sample_device="cpu")
    tiny = str(tmp_path / "tiny.npy")
    np.save(tiny, np.load(path)[:63])
    with pytest.raises(ValueError, match="at least 64"):            # the floor with upsampling on
        Dataset("pc_normal", [tiny], upsample_radius=0.1)
    with pytest.raises(ValueError, match="at least 64"):
        Dataset("pc_xyz", [tiny], upsample_radius=0.1)


def test_command_line_flags(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert a.upsample_radius == 0.0 and a.upsample_points == 16384 and a.cluster_min_points == 4096
    a = main.get_args(base + ["--input_type", "pc_normal", "--upsample_radius", "0.2", "--upsample_points", "8192"])
    assert a.upsample_radius == 0.2 and a.upsample_points == 8192
    assert main.get_args(base + ["--input_type", "pc_xyz", "--upsample_radius", "2"]).upsample_points == 16384
    assert main.get_args(base + ["--input_type", "mesh", "--upsample_radius", "0"]).upsample_radius == 0.0
    a = main.get_args(base + ["--input_type", "pc_xyz", "--upsample_radius", "0.1", "--cluster_radius", "0.1", "--cluster_min_points", "64"])
    assert a.cluster_min_points == 64
    assert main.get_args(base + ["--input_type", "pc_xyz", "--upsample_radius", "0.1", "--cluster_radius", "0.1"]).cluster_min_points == 4096
    for bad, word in [(["--input_type", "pc_xyz", "--upsample_radius", "-1"], "--upsample_radius"), (["--input_type", "pc_xyz", "--upsample_radius", "nan"], "--upsample_radius"),
                      (["--input_type", "pc_xyz", "--upsample_radius", "inf"], "--upsample_radius"),
                      (["--input_type", "pc_xyz", "--upsample_radius", "0.1", "--upsample_points", "4095"], "--upsample_points must be in 4096..4194304"),
                      (["--input_type", "pc_xyz", "--upsample_radius", "0.1", "--upsample_points", "4194305"], "--upsample_points must be in 4096..4194304"),
                      (["--input_type", "pc_xyz", "--upsample_points", "8192"], "needs --upsample_radius"),
                      (["--input_type", "pc_normal", "--upsample_radius", "0", "--upsample_points", "8192"], "needs --upsample_radius"),
                      (["--input_type", "mesh", "--upsample_radius", "0.1"], "mesh"), (["--input_type", "mesh", "--upsample_points", "8192"], "mesh"),
                      (["--input_type", "pc_xyz", "--upsample_radius", "0.1", "--cluster_radius", "0.1", "--cluster_min_points", "63"], "at least 64"),
                      (["--input_type", "pc_xyz", "--cluster_radius", "0.1", "--cluster_min_points", "64"], "at least 4096")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    helped = " ".join(capsys.readouterr().out.split())
    assert "--upsample_radius" in helped and "use --point_sampling fps" in helped and "the patch sticks out" in helped
