"""The host side of registration (meshanything_amd/pc_register.py, cloud_prep, data, main.py) without a GPU: the two solvers, the
composition, the loop's stop rule and refusals, the options and the command line, and the whole algorithm on the numpy restatement
`pc_register_ref`, whose accuracy over eight seeds gives the bounds of tests/test_gpu_pc_register.py.

MEASURED on the restatement (plane metric, three scans of the solid per seed, 3 072 surface samples each before its cut, poses of 5 degrees
and 0.03, D = 0.1, seeds 0..7; `test_accuracy_of_the_restatement_gives_the_gpu_bounds` prints the figures):
    file normals (pc_normal):         worst rotation error 4.603e-3 rad, worst displacement of a scan row 3.233e-3
    estimated normals (pc_xyz, k=16): 1.349e-2 rad and 1.135e-2; the fitted planes tilt at the solid's edges
    paired share of a scan: 0.700 .. 1.0, never below the 0.3 of min_overlap
BOUNDS, which the GPU test imports, are twice WORST.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_register_ref as R

from meshanything_amd import cloud_prep, pc_register               # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402

REPO = R.REPO
sys.path.insert(0, REPO) if REPO not in sys.path else None
import main as cli                                                 # noqa: E402

WORST = {"pc_normal": (4.7e-3, 3.3e-3), "pc_xyz": (1.35e-2, 1.14e-2)}   # (rotation error in rad, displacement), rounded up from the measured worst
BOUNDS = {k: (2 * a, 2 * m) for k, (a, m) in WORST.items()}
SEEDS = range(8)


# ---- the solvers -------------------------------------------------------------------------------------------------------------------------
def _lattice_cloud():
    """216 rows on a jittered 6^3 lattice of pitch 0.2: the least distance between two rows is above 0.1"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.2
    return (g + rng.uniform(-0.04, 0.04, g.shape)).astype(np.float32)


def test_solve_point_undoes_a_small_motion_in_one_step():
    """The source is a moved copy of target rows and no row moves by half the least inter-row distance, so every pair is the right one and
    Kabsch over exact correspondences returns the inverse motion; what is left is the float32 rounding of the stored rows, 2^-24 relative
    on coordinates of at most 1.1: under 1e-6 in t and in the rotation."""
    tgt = _lattice_cloud()
    d = np.linalg.norm(tgt[:, None].astype(np.float64) - tgt[None].astype(np.float64), axis=-1)
    least = d[d > 0].min()
    Rm, tm = R.rotation((3, -1, 2), 1.5), np.array([0.01, -0.008, 0.012])
    rows = np.arange(0, 216, 2)
    src = ((tgt[rows].astype(np.float64) - tm) @ Rm).astype(np.float32)   # x = R^T (q - t): (R, t) takes it back
    assert np.linalg.norm(src.astype(np.float64) - tgt[rows], axis=1).max() < least / 2
    centre = src.astype(np.float64).mean(0).astype(np.float32)
    calls = []

    def step(pose):
        s, _, idx, _ = R.sums_ref(tgt, src, pc_register.pose12(pose), centre, 0.1)
        calls.append(idx)
        return s
    res = pc_register.icp(step, centre.astype(np.float64), src.shape[0], iters=1, tol=0.0, metric="point", min_overlap=1.0)
    assert np.array_equal(calls[0], rows) and res["iterations"] == 1 and res["share"] == 1.0
    angle, move = R.pose_errors(res["pose"], (Rm, tm), src)
    assert angle < 1e-6 and move < 1e-6, (angle, move)
    assert res["rms_last"] < 1e-6 < res["rms_first"]


def test_solve_plane_on_hand_built_sums():
    """Residuals that are exactly linear in a known (w, v): r_i = -J_i . (w, v).  The solver returns exp(w) and c + v - exp(w) c."""
    rng = np.random.default_rng(2)
    c = np.array([0.3, -0.2, 0.5])
    u = rng.standard_normal((40, 3))
    n = rng.standard_normal((40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    J = np.concatenate([np.cross(u, n), n], 1)
    x = np.array([0.01, -0.02, 0.015, 0.003, -0.001, 0.002])
    r = -J @ x
    sums = np.zeros(32)
    sums[0], sums[2], sums[3:9] = 40, (r * r).sum(), (J * r[:, None]).sum(0)
    iu = np.triu_indices(6)
    sums[9:30] = (J[:, iu[0]] * J[:, iu[1]]).sum(0)
    dR, dt = pc_register.solve_plane(sums, c)
    want = pc_register.exp_so3(x[:3])
    assert np.abs(dR - want).max() < 1e-12 and np.abs(dt - (c + x[3:] - want @ c)).max() < 1e-12
    assert np.abs(dR @ dR.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(dR) - 1) < 1e-15
    K = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    series = np.eye(3) + K + K @ K / 2 + K @ K @ K / 6 + K @ K @ K @ K / 24
    assert np.abs(want - series).max() < 1e-9                        # the exponential, not its first-order stand-in
    assert np.array_equal(pc_register.exp_so3(np.zeros(3)), np.eye(3))
    with pytest.raises(ValueError, match="singular"):
        pc_register.solve_plane(np.zeros(32), c)
    with pytest.raises(ValueError, match="32 numbers"):
        pc_register.solve_plane(np.zeros(31), c)


def test_solve_point_fixes_a_reflection():
    """Flat, mirrored data: the SVD's best orthogonal map is a reflection; the determinant is fixed and a rotation comes back."""
    rng = np.random.default_rng(4)
    u = np.concatenate([rng.standard_normal((30, 2)), np.zeros((30, 1))], 1)
    v = u * np.array([1.0, -1.0, 1.0])
    sums = np.zeros(32)
    sums[0], sums[2:5], sums[5:8], sums[8:17] = 30, u.sum(0), v.sum(0), (u[:, :, None] * v[:, None, :]).sum(0).reshape(9)
    dR, _ = pc_register.solve_point(sums, np.zeros(3))
    assert abs(np.linalg.det(dR) - 1) < 1e-12 and np.abs(dR @ dR.T - np.eye(3)).max() < 1e-12


def test_compose_keeps_the_rotation_orthonormal_over_256_steps():
    rng = np.random.default_rng(0)
    pose = pc_register.IDENTITY
    point = np.array([0.3, -0.4, 0.5])
    want = point.copy()
    for _ in range(256):
        step = (pc_register.exp_so3(rng.standard_normal(3) * 0.2), rng.standard_normal(3) * 0.1)
        pose = pc_register.compose(pose, step)
        want = step[0] @ want + step[1]
    R256, t256 = pose
    assert R256.dtype == np.float64 and np.abs(R256 @ R256.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R256) - 1) < 1e-14
    assert np.abs(R256 @ point + t256 - want).max() < 1e-11
    assert pc_register.pose12(pose).dtype == np.float32 and pc_register.pose12(pose).shape == (12,)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def _fake(rms, used=100.0, skipped=0.0, metric="plane"):
    """Sums with the given RMS whose solve is the identity motion."""
    s = np.zeros(32)
    s[0], s[30] = used, skipped
    if metric == "plane":
        s[2] = rms * rms * used
        s[[9, 15, 20, 24, 27, 29]] = 1.0                             # the diagonal of sum J J^T
    else:
        s[1] = rms * rms * used
        s[8], s[12], s[16] = 1.0, 1.0, 1.0
    return s


def _run(rms_list, **kw):
    calls = []

    def step(pose):
        calls.append(pose)
        return _fake(rms_list[min(len(calls), len(rms_list)) - 1], **{k: v for k, v in kw.items() if k in ("used", "skipped", "metric")})
    res = pc_register.icp(step, np.zeros(3), kw.pop("rows", 100), **{k: v for k, v in kw.items() if k not in ("used", "skipped")})
    return res, len(calls)


def test_the_loop_stops_on_a_steady_rms_or_after_iters():
    res, calls = _run([1.0, 0.5, 0.5, 0.1], tol=1e-6)
    assert (res["iterations"], calls, res["rms_first"], res["rms_last"]) == (2, 3, 1.0, 0.5)
    res, calls = _run([1.0, 0.5, 0.4999999], tol=1e-6)                 # a change of 2e-7 of the previous value is within 1e-6
    assert (res["iterations"], calls) == (2, 3)
    res, calls = _run([1.0, 0.5, 0.4999], tol=1e-6, iters=30)
    assert (res["iterations"], calls) == (3, 4)                        # ... 0.4999, 0.4999: steady one evaluation later
    res, calls = _run([2.0 ** -i for i in range(40)], tol=1e-6, iters=3)
    assert (res["iterations"], calls, res["rms_last"]) == (3, 4, 0.125)   # three solves, and the sums of the last pose are evaluated
    res, calls = _run([1.0, 1.0], tol=0.0)
    assert (res["iterations"], calls) == (1, 2)
    res, calls = _run([1.0, 0.5, 0.5], tol=1e-6, metric="point")
    assert (res["iterations"], calls, res["share"]) == (2, 3, 1.0)


def test_the_loop_refuses_too_few_pairs_and_low_overlap():
    with pytest.raises(ValueError, match=r"chair: registration of scan side found 5 usable pairs, fewer than the 6 the plane metric needs"):
        _run([1.0], used=5.0, scan="side", uid="chair")
    with pytest.raises(ValueError, match=r"found 2 usable pairs, fewer than the 3 the point metric needs"):
        _run([1.0], used=2.0, metric="point")
    _run([1.0, 1.0], used=3.0, metric="point", rows=3)
    with pytest.raises(ValueError, match=r"chair: registration of scan side paired 0\.250 of its rows, below the minimum overlap 0\.3: do the scans start within"):
        _run([1.0, 1.0], used=20.0, skipped=5.0, scan="side", uid="chair")
    res, _ = _run([1.0, 1.0], used=25.0, skipped=5.0)                  # skipped pairs are pairs: 0.3 of the rows
    assert res["share"] == 0.3


def test_register_rows_refuses_before_it_touches_a_device():
    ok = np.zeros((64, 3), np.float32)
    with pytest.raises(ValueError, match="chair: scan b has 63 rows, fewer than the 64 registration takes"):
        pc_register.register_rows([ok, ok[:63]], 0.1, uid="chair", names=["a", "b"], metric="point")
    big = np.zeros(((1 << 21) + 1, 3), np.float32)
    with pytest.raises(ValueError, match=r"chair: the union of the scans has 4194306 rows, more than 2\^22: thin the scans with --voxel_size"):
        pc_register.register_rows([big, big], 0.1, uid="chair", metric="point")
    with pytest.raises(ValueError, match="non-finite"):
        pc_register.register_rows([ok, np.full((64, 3), np.nan, np.float32)], 0.1, metric="point")
    with pytest.raises(ValueError, match="6 columns"):
        pc_register.register_rows([ok, np.zeros((64, 6), np.float32)], 0.1, metric="point")
    with pytest.raises(ValueError, match="plane metric needs normals"):
        pc_register.register_rows([ok, ok], 0.1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_register.register_rows([ok, ok], 0.1, metric="point", device="cpu")


def test_normals_turn_with_the_points():
    Rm, tm = R.rotation((1, 2, 3), 30.0), np.array([1.0, 2.0, 3.0])
    rows = np.concatenate([np.eye(3), np.eye(3), np.full((3, 1), 7.0)], 1).astype(np.float32)
    out = pc_register.apply_pose(rows, (Rm, tm))
    assert out.dtype == np.float32 and np.abs(out[:, :3] - (Rm.T + tm)).max() < 1e-6 and np.abs(out[:, 3:6] - Rm.T).max() < 1e-7 and (out[:, 6] == 7).all()
    kept = pc_register.apply_pose(rows, (Rm, tm), normals=False)
    assert np.array_equal(kept[:, 3:], rows[:, 3:]) and np.array_equal(kept[:, :3], out[:, :3]) and np.array_equal(rows[:, :3], np.eye(3, dtype=np.float32))


# ---- options, Dataset and the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, message", [
    (dict(register_dist=-1.0), "radius must be finite and > 0"), (dict(register_dist=float("nan")), "radius must be finite and > 0"),
    (dict(register_dist=0.1, register_iters=0), "iters must be an integer in 1..256"), (dict(register_dist=0.1, register_iters=257), "iters must be an integer in 1..256"),
    (dict(register_dist=0.1, register_tol=1.0), r"tol must be in \[0, 1\)"), (dict(register_dist=0.1, register_tol=-1e-9), r"tol must be in \[0, 1\)"),
    (dict(register_dist=0.1, register_metric="planes"), "metric must be one of"),
    (dict(register_dist=0.1, register_min_overlap=0.0), r"min_overlap must be in \(0, 1\]"), (dict(register_dist=0.1, register_min_overlap=1.5), r"min_overlap must be in \(0, 1\]"),
    (dict(register_iters=10), "register_iters needs register_dist > 0"), (dict(register_tol=1e-3), "register_tol needs register_dist > 0"),
    (dict(register_metric="point"), "register_metric needs register_dist > 0"), (dict(register_min_overlap=0.5), "register_min_overlap needs register_dist > 0")])
def test_dataset_refuses_bad_options_before_it_reads_a_file(kw, message):
    with pytest.raises(ValueError, match=message):
        Dataset("pc_normal", ["/no/such/file.npy"], **kw)


def test_mesh_inputs_are_refused_and_the_stage_list_is_unchanged():
    with pytest.raises(ValueError, match="register_dist applies to pc_normal and pc_xyz inputs"):
        Dataset("mesh", ["/no/such/file.obj"], register_dist=0.1)
    assert [s.switch for s in cloud_prep.STAGES] == ["voxel_size", "outlier_k", "plane_threshold", "cluster_radius", "smooth_radius", "upsample_radius"]
    assert cloud_prep.SCANS.switch == "register_dist" and cloud_prep.SCANS.module == "pc_register" and cloud_prep.SCANS not in cloud_prep.STAGES
    p = cloud_prep.CloudPrep()
    assert (p.register_dist, p.register_iters, p.register_tol, p.register_metric, p.register_min_overlap) == (0.0, 30, 1e-6, "plane", 0.3) and p.scans() == []


@pytest.mark.parametrize("argv, message", [
    (["--register_dist", "-1"], "--register_dist must be finite and >= 0"), (["--register_dist", "inf"], "--register_dist must be finite and >= 0"),
    (["--register_iters", "5"], "--register_iters, --register_tol, --register_metric and --register_min_overlap need --register_dist > 0"), (["--register_tol", "1e-3"], "--register_iters, --register_tol, --register_metric and --register_min_overlap need --register_dist > 0"),
    (["--register_metric", "point"], "--register_iters, --register_tol, --register_metric and --register_min_overlap need --register_dist > 0"), (["--register_min_overlap", "0.5"], "--register_iters, --register_tol, --register_metric and --register_min_overlap need --register_dist > 0"),
    (["--register_dist", "0.1", "--register_iters", "0"], "--register_iters must be in 1..256"), (["--register_dist", "0.1", "--register_iters", "257"], "--register_iters must be in 1..256"),
    (["--register_dist", "0.1", "--register_tol", "1"], "--register_tol must be in [0, 1)"), (["--register_dist", "0.1", "--register_min_overlap", "0"], "--register_min_overlap must be in (0, 1]"),
    (["--register_dist", "0.1", "--register_metric", "planes"], "invalid choice"),
    (["--register_dist", "0.1", "--input_type", "mesh"], "--register_dist, --register_iters, --register_tol, --register_metric and --register_min_overlap apply to --input_type pc_normal and pc_xyz")])
def test_cli_errors(argv, message, capsys):
    with pytest.raises(SystemExit):
        cli.get_args((["--input_type", "pc_normal"] if "--input_type" not in argv else []) + argv)
    assert message in capsys.readouterr().err


def test_cli_defaults_and_values():
    a = cli.get_args(["--input_type", "pc_xyz"])
    assert (a.register_dist, a.register_iters, a.register_tol, a.register_metric, a.register_min_overlap) == (0.0, 30, 1e-6, "plane", 0.3)
    assert cloud_prep.CloudPrep.from_args(a) == cloud_prep.CloudPrep()
    a = cli.get_args(["--input_type", "pc_xyz", "--register_dist", "0.2", "--register_iters", "7", "--register_tol", "0", "--register_metric", "point", "--register_min_overlap", "1"])
    p = cloud_prep.CloudPrep.from_args(a)
    assert (p.register_dist, p.register_iters, p.register_tol, p.register_metric, p.register_min_overlap) == (0.2, 7, 0.0, "point", 1.0)


def test_the_switch_off_imports_nothing_and_a_directory_fails_as_before(tmp_path):
    rows = np.concatenate([np.random.default_rng(0).random((4096, 3)), np.tile([0.0, 0.0, 1.0], (4096, 1))], 1).astype(np.float32)
    np.save(tmp_path / "a.npy", rows)
    (tmp_path / "scans").mkdir()
    code = f"""
import sys
sys.path.insert(0, {REPO!r})
import numpy as np
import main
from meshanything_amd.cloud_prep import CloudPrep
from meshanything_amd.data import Dataset
args = main.get_args(["--input_type", "pc_normal", "--input_path", {str(tmp_path / "a.npy")!r}])
np.random.seed(0)
ds = Dataset("pc_normal", [args.input_path], **vars(CloudPrep.from_args(args)))
assert sorted(ds[0]) == ["pc_normal", "uid"]
assert "meshanything_amd.pc_register" not in sys.modules
try:
    Dataset("pc_normal", [{str(tmp_path / "scans")!r}])
    raise SystemExit("a directory loaded")
except (IsADirectoryError, OSError):
    pass
assert "meshanything_amd.pc_register" not in sys.modules
print("off: ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines() == ["dataset total data samples: 1", "off: ok"], r.stdout + r.stderr


def test_a_directory_is_one_object_and_its_files_are_scans_in_sorted_order(tmp_path, monkeypatch):
    folder = tmp_path / "chair"
    folder.mkdir()
    rng = np.random.default_rng(1)
    for name, rows in (("b_side.npy", 3000), ("a_front.npy", 2000), ("c_back.PLY.npy", 1500), ("notes.md", 0)):
        if rows:
            np.save(folder / name, np.concatenate([rng.random((rows, 3)), np.tile([0.0, 0.0, 1.0], (rows, 1))], 1).astype(np.float32))
        else:
            (folder / name).write_text("not a scan")
    (folder / "sub.npy").mkdir()
    seen = {}

    def fake(scans, dist, iters, tol, metric, min_overlap, normal_k, uid, device="cuda", names=None):
        seen.update(rows=[s.shape[0] for s in scans], names=names, uid=uid, args=(dist, iters, tol, metric, min_overlap, normal_k))
        return np.concatenate(scans), [pc_register.IDENTITY] * len(scans)
    monkeypatch.setattr(pc_register, "register_rows", fake)
    np.random.seed(0)
    ds = Dataset("pc_normal", [str(folder) + "/"], register_dist=0.25, register_iters=9)
    assert seen == dict(rows=[2000, 3000, 1500], names=["a_front", "b_side", "c_back"], uid="chair", args=(0.25, 9, 1e-6, "plane", 0.3, None))
    item = ds[0]
    assert len(ds) == 1 and item["uid"] == "chair" and sorted(item) == ["pc_normal", "scan_poses", "uid"] and len(item["scan_poses"]) == 3
    assert item["pc_normal"].shape == (4096, 6)
    with pytest.raises(ValueError, match="empty: the directory holds no pc_normal scan"):
        (tmp_path / "empty").mkdir()
        Dataset("pc_normal", [str(tmp_path / "empty")], register_dist=0.25)


# ---- the whole algorithm on the restatement ------------------------------------------------------------------------------------------------
def test_the_solid_and_its_scans():
    xyz, nrm = R.solid_surface(20000, 0)
    assert xyz.min(0).tolist() == pytest.approx([0, 0, 0], abs=1e-3) and xyz.max(0).tolist() == pytest.approx([1.0, 0.6, 0.6], abs=1e-3)
    assert (np.abs(nrm).sum(1) == 1).all() and not ((xyz[:, 2] == 0.3) & (xyz[:, 0] < 0.3) & (xyz[:, 1] < 0.3)).any()
    scans = R.solid_scans(0)
    assert len(scans) == 3 and all(s.dtype == np.float32 and s.shape[1] == 6 and 1500 < s.shape[0] < R.SCAN_ROWS for s in scans)
    for s, (Rt, tt) in zip(scans, R.TRUE_POSES):                       # the true pose takes every scan back onto the solid
        back = s[:, :3].astype(np.float64) @ Rt.T + tt
        assert back.min() > -1e-6 and (back.max(0) < np.array([1.0, 0.6, 0.6]) + 1e-6).all()
    assert sum(s.shape[0] for s in scans) >= 4096                      # the union feeds the encoder's 4096 rows


@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_accuracy_of_the_restatement_gives_the_gpu_bounds(kind):
    worst_angle = worst_move = 0.0
    shares = []
    for seed in SEEDS:
        scans = R.solid_scans(seed)
        normals = None if kind == "pc_normal" else [R.pca_normals(s[:, :3]) for s in scans]
        poses, results = R.register_ref(scans, R.DIST, normals=normals)
        for j in (1, 2):
            angle, move = R.pose_errors(poses[j], R.TRUE_POSES[j], scans[j][:, :3])
            start = R.pose_errors(pc_register.IDENTITY, R.TRUE_POSES[j], scans[j][:, :3])
            assert angle < start[0] / 4 and move < start[1] / 4        # it started 5 degrees (0.087 rad) and about 0.05 away: it went the right way
            worst_angle, worst_move = max(worst_angle, angle), max(worst_move, move)
            shares.append(results[j]["share"])
            assert 1 <= results[j]["iterations"] <= 30 and results[j]["rms_last"] < results[j]["rms_first"]
    print(f"{kind}: worst rotation error {worst_angle:.4e} rad, worst displacement {worst_move:.4e}, paired shares {min(shares):.3f} .. {max(shares):.3f}")
    assert min(shares) >= 0.3                                          # the reference itself keeps min_overlap of every scan paired
    assert worst_angle <= WORST[kind][0] and worst_move <= WORST[kind][1]
    assert worst_angle >= WORST[kind][0] / 2 and worst_move >= WORST[kind][1] / 2   # and the recorded figures are not slack


def test_the_point_metric_stalls_where_the_plane_metric_converges():
    """Flat faces resist sliding under point-to-point pairs: after the 30 default iterations the point metric is still far from where the plane metric ends."""
    scans = R.solid_scans(0)[:2]
    plane, _ = R.register_ref(scans, R.DIST)
    point, _ = R.register_ref([s[:, :3] for s in scans], R.DIST, metric="point")
    a_plane, a_point = (R.pose_errors(p[1], R.TRUE_POSES[1], scans[1][:, :3])[0] for p in (plane, point))
    print(f"rotation error after at most 30 iterations: plane {a_plane:.3e} rad, point {a_point:.3e} rad")
    assert a_point > 3 * a_plane
