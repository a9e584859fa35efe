"""The host side of coarse registration (meshanything_amd/pc_coarse.py, pc_register.register_rows(coarse=...), cloud_prep, data, main.py)
without a GPU: the numpy restatement `pc_coarse_ref` against a plain float64 brute force, triple pruning and the batched Kabsch, the
refusals, the options and the command line, the off state, and the whole algorithm on the restatement, whose accuracy over six seeds
gives the bounds of tests/test_gpu_pc_coarse.py.

MEASURED on the restatement (two cut scans of the bumpy ellipsoid per seed, about 2 600 rows each, scan 1 turned by 30 .. 180 degrees about a
random axis and shifted by 0.5 normal(3); F = 0.15, K = 512, H = 4096, T = 0.04, then pc_register.icp at D = 0.1 with the plane metric;
seeds 0..5; `test_accuracy_of_the_restatement_gives_the_gpu_bounds` prints the figures):
    mutual matches 159 .. 198, surviving triples 268 .. 436, best agreement count 30 .. 50
    coarse pose:  worst rotation error 8.511e-2 rad, worst displacement of a scan row 5.426e-2: inside D, which is all ICP asks
    after ICP:    4 .. 6 iterations, paired share 0.884 .. 0.897, worst rotation error 4.022e-3 rad, worst displacement 2.854e-3
    with the defaults K = 1024 and T = F / 4: 274 .. 331 mutual matches, counts 50 .. 97, coarse 6.03e-2 rad and 4.08e-2: the defaults hold
BOUNDS, which the GPU test imports, are twice WORST.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_coarse_ref as CR
import pc_register_ref as RR

from meshanything_amd import cloud_prep, pc_coarse, pc_register      # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402

REPO = CR.REPO
sys.path.insert(0, REPO) if REPO not in sys.path else None
import main as cli                                                 # noqa: E402

WORST = {"coarse": (8.6e-2, 5.5e-2), "icp": (4.1e-3, 2.9e-3)}        # (rotation error in rad, displacement), rounded up from the measured worst
BOUNDS = {k: (2 * a, 2 * m) for k, (a, m) in WORST.items()}


# ---- the restatement against the plain definition ----------------------------------------------------------------------------------------
def _small_cloud(n=160, seed=4):
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    return xyz, (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)


def test_the_restatement_equals_a_float64_brute_force_on_a_small_cloud():
    xyz, nrm = _small_cloud()
    hist = CR.spfh_ref(xyz, nrm, 0.3)
    plain = CR.spfh_plain(xyz, nrm, 0.3)
    assert hist.dtype == np.uint32 and hist.shape == (160, 34) and np.array_equal(hist, plain)
    assert 5 < hist[:, 33].mean() < 40 and (hist[:, :11].sum(1) == hist[:, 33]).all() and (hist[:, 11:22].sum(1) == hist[:, 33]).all() and (hist[:, 22:33].sum(1) == hist[:, 33]).all()
    query = np.array([0, 159, 7, 7, 80])
    desc = CR.gather_ref(xyz, hist, 0.3, query)
    d2 = ((xyz[query, None, :].astype(np.float64) - xyz[None].astype(np.float64)) ** 2).sum(-1)
    want = np.stack([plain[q, :33] + plain[(d2[j] > 0) & (d2[j] <= 0.09), :33].sum(0) for j, q in enumerate(query)])
    assert desc.dtype == np.uint32 and np.array_equal(desc, want) and np.array_equal(desc[2], desc[3])


def test_match_and_score_equal_a_float64_brute_force():
    rng = np.random.default_rng(2)
    A, B = rng.integers(0, 500, (70, 33)).astype(np.uint32), rng.integers(0, 500, (90, 33)).astype(np.uint32)
    B[5] = B[60] = A[3]                                                # a tie at distance 0: the lower index
    A[9, 11:22] = 0                                                    # a zero block stays zero
    norm = lambda D: np.concatenate([np.where(b.sum(1, keepdims=True) > 0, b / np.maximum(b.sum(1, keepdims=True), 1), 0.0) for b in np.split(D.astype(np.float64), 3, 1)], 1)
    dist = ((norm(A)[:, None, :] - norm(B)[None]) ** 2).sum(-1)
    idx, d = CR.match_ref(A, B)
    assert idx.dtype == np.int32 and d.dtype == np.float32 and idx[3] == 5 and d[3] == 0 and np.array_equal(idx, dist.argmin(1))
    assert np.allclose(d, dist.min(1), rtol=1e-5, atol=1e-9) and np.isfinite(CR.normalise_ref(A)).all() and not CR.normalise_ref(A)[9, 11:22].any()
    P, Q = rng.random((50, 3)), rng.random((50, 3))
    poses = np.stack([np.concatenate([RR.rotation(rng.normal(size=3), 40.0 * h).reshape(9), 0.1 * rng.normal(size=3)]) for h in range(7)])
    poses[4] = poses[2]                                                # equal counts: the lower index
    counts, best = CR.score_ref(poses, P, Q, 0.45)
    want = [int((np.linalg.norm(P @ p[:9].reshape(3, 3).T + p[9:] - Q, axis=1) <= 0.45).sum()) for p in poses]
    assert counts.tolist() == want and best == int(np.argmax(want)) and counts[4] == counts[2]
    assert np.array_equal(pc_coarse.agreeing(poses[1], P, Q, 0.45), np.linalg.norm(P @ poses[1][:9].reshape(3, 3).T + poses[1][9:] - Q, axis=1) <= 0.45)


# ---- the host steps ----------------------------------------------------------------------------------------------------------------------------
def test_mutual_matches_and_the_fallback():
    ab = np.arange(40) % 20
    ba = np.arange(20)
    assert pc_coarse.mutual_matches(ab, ba).tolist() == [[a, a] for a in range(20)]             # 20 mutual: kept alone
    ba[:8] = 39
    assert pc_coarse.mutual_matches(ab, ba).tolist() == [[a, a % 20] for a in range(40)]        # 12 mutual, fewer than 16: every source -> target match


def test_triples_come_from_a_private_generator_and_are_pruned_by_index_and_edge_length():
    np.random.seed(7)
    before = np.random.get_state()[1].copy()
    t = pc_coarse.draw_triples(100, 4096)
    assert t.shape == (4096, 3) and t.dtype == np.int64 and t.min() >= 0 and t.max() == 99 and np.array_equal(t, pc_coarse.draw_triples(100, 4096))
    assert np.array_equal(np.random.get_state()[1], before)
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.05, 0, 0], [0, 0, 1]], float)
    Q = P.copy()
    Q[4] = [0, 0, 0.85]                                                # edges 0-4: 1 against 0.85, below the factor 0.9
    triples = np.array([[0, 1, 2], [0, 0, 1], [1, 2, 1], [0, 3, 2], [0, 1, 4], [1, 2, 4]])
    kept = pc_coarse.prune_triples(triples, P, Q, 0.04)
    assert kept.tolist() == [[0, 1, 2], [1, 2, 4]]                      # a repeated index twice, an edge of 0.05 < 2 T, 0.85 / 1 < 0.9; sqrt(1.7225) / sqrt(2) = 0.928 stays
    assert pc_coarse.prune_triples(triples, P, Q, 0.02).tolist() == [[0, 1, 2], [0, 3, 2], [1, 2, 4]]


def test_batched_kabsch_is_the_exact_inverse_and_never_a_reflection():
    rng = np.random.default_rng(3)
    P = rng.normal(size=(5, 3, 3))
    Rs = np.stack([RR.rotation(rng.normal(size=3), 35.0 * (h + 1)) for h in range(5)])
    ts = rng.normal(size=(5, 3))
    Q = P @ np.swapaxes(Rs, 1, 2) + ts[:, None, :]
    R, t = pc_coarse.kabsch(P, Q)
    assert R.shape == (5, 3, 3) and t.shape == (5, 3) and np.abs(R - Rs).max() < 1e-12 and np.abs(t - ts).max() < 1e-12
    R1, t1 = pc_coarse.kabsch(P[2], Q[2])                              # unbatched
    assert np.abs(R1 - Rs[2]).max() < 1e-12 and np.abs(t1 - ts[2]).max() < 1e-12
    mirrored = P * np.array([1.0, 1.0, -1.0])                          # no rotation maps a triangle's mirror image with its normal flipped ... but one fits it best
    R, t = pc_coarse.kabsch(np.concatenate([P, rng.normal(size=(5, 1, 3))], 1), np.concatenate([mirrored, rng.normal(size=(5, 1, 3))], 1))
    assert np.allclose(np.linalg.det(R), 1.0) and np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-12
    assert pc_coarse.poses12(Rs, ts).shape == (5, 12) and pc_coarse.poses12(Rs, ts).dtype == np.float32


class _FakeOps:
    """keypoints = the first k rows; descriptors and matches as told"""

    def __init__(self, st, ts, counts=None):
        self.st, self.ts, self.counts, self.asked = np.asarray(st), np.asarray(ts), counts, 0

    def keypoints(self, xyz, k):
        return np.arange(k)

    def describe(self, xyz, normals, radius, query):
        return np.zeros((query.shape[0], 33), np.int64)

    def match(self, A, B):
        self.asked += 1                                                 # source -> target is asked first
        return self.st if self.asked % 2 else self.ts

    def score(self, poses, P, Q, dist):
        return CR.score_ref(poses, P, Q, dist) if self.counts is None else (np.full(poses.shape[0], self.counts, np.int32), 0)


def test_each_refusal_names_scan_and_uid():
    rng = np.random.default_rng(0)
    x = rng.random((64, 3)).astype(np.float32)
    n = np.tile(np.float32([0, 0, 1]), (64, 1))
    run = lambda ops, tgt=x, k=64: pc_coarse.coarse_pose(tgt, n[:tgt.shape[0]], x, n, 0.2, k, 256, 0.05, ops=ops, scan="side", uid="chair")    # noqa: E731
    with pytest.raises(ValueError, match="chair: coarse registration of scan side found 2 matches, fewer than the 3"):
        pc_coarse.coarse_pose(x[:2], n[:2], x[:2], n[:2], 0.2, 64, 256, 0.05, ops=_FakeOps([0, 1], [0, 1]), scan="side", uid="chair")
    with pytest.raises(ValueError, match="chair: coarse registration of scan side: none of 256 triples of its 64 matches has edges of matching length"):
        run(_FakeOps(np.arange(64), np.arange(64)), tgt=x * np.float32(3.0))                    # a target three times the size: no triangle matches
    with pytest.raises(ValueError, match="chair: coarse registration of scan side: the best of [0-9]+ hypotheses agrees with 3 matches, fewer than 4"):
        run(_FakeOps(np.arange(64), np.arange(64), counts=3))
    got = run(_FakeOps(np.arange(64), np.arange(64)))                                          # the same cloud, every match right: the identity, every match agreeing
    assert got["mutual"] == 64 and got["count"] == 64 and got["triples"] > 0 and got["angle"] < 1e-4 and np.abs(got["pose"][1]).max() < 1e-6


def test_register_rows_checks_the_coarse_options_before_it_touches_a_device():
    ok = np.random.default_rng(0).random((64, 3)).astype(np.float32)
    for coarse, message in (((0.0, 1024, 4096, None), "radius must be finite and > 0"), ((0.1, 63, 4096, None), "coarse_points must be an integer in 64..4096"),
                            ((0.1, 1024, 255, None), "coarse_iters must be an integer in 256..65536"), ((0.1, 1024, 4096, 0.0), "coarse_dist must be finite and > 0")):
        with pytest.raises(ValueError, match=message):
            pc_register.register_rows([ok, ok], 0.1, metric="point", coarse=coarse)
    with pytest.raises(ValueError, match="coarse registration needs normals in columns 3:6, or normal_k"):
        pc_register.register_rows([ok, ok], 0.1, metric="point", coarse=(0.1, 64, 256, None))
    assert pc_coarse.check_coarse_args(0.2, 64, 65536, None) == (0.2, 64, 65536, 0.05)


# ---- options, Dataset and the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, message", [
    (dict(coarse_radius=0.1), "coarse_radius needs register_dist > 0"), (dict(coarse_points=512), "coarse_points needs coarse_radius > 0"),
    (dict(coarse_iters=512), "coarse_iters needs coarse_radius > 0"), (dict(coarse_dist=0.1), "coarse_dist needs coarse_radius > 0"),
    (dict(register_dist=0.1, coarse_points=512), "coarse_points needs coarse_radius > 0"),
    (dict(coarse_radius=0.1, coarse_points=512), "coarse_radius needs register_dist > 0"),
    (dict(register_dist=0.1, coarse_radius=-1.0), "radius must be finite and > 0"), (dict(register_dist=0.1, coarse_radius=float("nan")), "radius must be finite and > 0"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_points=63), "coarse_points must be an integer in 64..4096"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_points=4097), "coarse_points must be an integer in 64..4096"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_iters=255), "coarse_iters must be an integer in 256..65536"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_iters=65537), "coarse_iters must be an integer in 256..65536"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_dist=0.0), "coarse_dist must be finite and > 0"),
    (dict(register_dist=0.1, coarse_radius=0.1, coarse_dist=float("inf")), "coarse_dist must be finite and > 0")])
def test_dataset_refuses_bad_options_before_it_reads_a_file(kw, message):
    with pytest.raises(ValueError, match=message):
        Dataset("pc_normal", ["/no/such/file.npy"], **kw)


@pytest.mark.parametrize("kw", [dict(coarse_radius=0.1), dict(coarse_points=512), dict(coarse_iters=512), dict(coarse_dist=0.1)])
def test_mesh_inputs_are_refused(kw):
    with pytest.raises(ValueError, match=f"{next(iter(kw))} applies to the scans of pc_normal and pc_xyz inputs, not to mesh inputs"):
        Dataset("mesh", ["/no/such/file.obj"], register_dist=0.1, **kw)


_NEED = "--coarse_points, --coarse_iters and --coarse_dist need --coarse_radius > 0"


@pytest.mark.parametrize("argv, message", [
    (["--coarse_radius", "-1"], "--coarse_radius must be finite and >= 0"), (["--coarse_radius", "inf"], "--coarse_radius must be finite and >= 0"),
    (["--coarse_radius", "0.1"], "--coarse_radius needs --register_dist > 0"),
    (["--coarse_points", "512"], _NEED), (["--coarse_iters", "512"], _NEED), (["--coarse_dist", "0.1"], _NEED), (["--register_dist", "0.1", "--coarse_points", "512"], _NEED),
    (["--register_dist", "0.1", "--coarse_radius", "0.1", "--coarse_points", "63"], "--coarse_points must be in 64..4096"),
    (["--register_dist", "0.1", "--coarse_radius", "0.1", "--coarse_points", "4097"], "--coarse_points must be in 64..4096"),
    (["--register_dist", "0.1", "--coarse_radius", "0.1", "--coarse_iters", "255"], "--coarse_iters must be in 256..65536"),
    (["--register_dist", "0.1", "--coarse_radius", "0.1", "--coarse_iters", "65537"], "--coarse_iters must be in 256..65536"),
    (["--register_dist", "0.1", "--coarse_radius", "0.1", "--coarse_dist", "0"], "--coarse_dist must be finite and > 0"),
    (["--coarse_radius", "0.1", "--input_type", "mesh"], "--coarse_radius, --coarse_points, --coarse_iters and --coarse_dist apply to --input_type pc_normal and pc_xyz"),
    (["--coarse_iters", "512", "--input_type", "mesh"], "--coarse_radius, --coarse_points, --coarse_iters and --coarse_dist apply to --input_type pc_normal and pc_xyz")])
def test_cli_errors(argv, message, capsys):
    with pytest.raises(SystemExit):
        cli.get_args((["--input_type", "pc_normal"] if "--input_type" not in argv else []) + argv)
    assert message in capsys.readouterr().err


def test_defaults_and_values_from_the_command_line():
    p = cloud_prep.CloudPrep()
    assert (p.coarse_radius, p.coarse_points, p.coarse_iters, p.coarse_dist) == (0.0, 1024, 4096, None)
    assert (pc_coarse.DEFAULT_POINTS, pc_coarse.DEFAULT_ITERS) == (1024, 4096)
    a = cli.get_args(["--input_type", "pc_xyz"])
    assert (a.coarse_radius, a.coarse_points, a.coarse_iters, a.coarse_dist) == (0.0, 1024, 4096, None) and cloud_prep.CloudPrep.from_args(a) == p
    a = cli.get_args(["--input_type", "pc_xyz", "--register_dist", "0.2", "--coarse_radius", "0.3", "--coarse_points", "64", "--coarse_iters", "65536", "--coarse_dist", "0.01"])
    q = cloud_prep.CloudPrep.from_args(a)
    assert (q.register_dist, q.coarse_radius, q.coarse_points, q.coarse_iters, q.coarse_dist) == (0.2, 0.3, 64, 65536, 0.01) and q.check("pc_xyz", 4096) == 4096
    assert "--coarse_radius" in cli.__doc__ and [s.switch for s in cloud_prep.STAGES] == ["voxel_size", "outlier_k", "plane_threshold", "cluster_radius", "smooth_radius", "upsample_radius"]


def _write_two_scans(folder):
    folder.mkdir()
    rng = np.random.default_rng(1)
    for name, rows in (("a.npy", 3000), ("b.npy", 2000)):
        np.save(folder / name, np.concatenate([rng.random((rows, 3)), np.tile([0.0, 0.0, 1.0], (rows, 1))], 1).astype(np.float32))


def test_the_switch_off_imports_nothing_and_makes_the_call_of_before(tmp_path):
    """In a fresh interpreter: register_rows is replaced by a function with the signature it had before the stage existed."""
    _write_two_scans(tmp_path / "chair")
    code = f"""
import sys
sys.path.insert(0, {REPO!r})
import numpy as np
import main
from meshanything_amd import pc_register
from meshanything_amd.cloud_prep import CloudPrep
from meshanything_amd.data import Dataset
seen = []
def fake(scans, dist, iters=30, tol=1e-6, metric="plane", min_overlap=0.3, normal_k=None, uid="?", device="cuda", names=None):
    seen.append((len(scans), dist, iters, tol, metric, min_overlap, normal_k, uid, names))
    return np.concatenate(scans), [pc_register.IDENTITY] * len(scans)
pc_register.register_rows = fake
args = main.get_args(["--input_type", "pc_normal", "--input_path", {str(tmp_path / "chair")!r}, "--register_dist", "0.25"])
np.random.seed(0)
ds = Dataset("pc_normal", [args.input_path], **vars(CloudPrep.from_args(args)))
assert seen == [(2, 0.25, 30, 1e-6, "plane", 0.3, None, "chair", ["a", "b"])], seen
assert sorted(ds[0]) == ["pc_normal", "scan_poses", "uid"]
assert "meshanything_amd.pc_coarse" not in sys.modules
print("off: ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines() == ["dataset total data samples: 1", "off: ok"], r.stdout + r.stderr


def test_the_switch_on_passes_the_options_to_register_rows(tmp_path, monkeypatch):
    _write_two_scans(tmp_path / "chair")
    seen = {}

    def fake(scans, dist, iters, tol, metric, min_overlap, normal_k, uid, device="cuda", names=None, coarse=None):
        seen.update(coarse=coarse, names=names, dist=dist)
        return np.concatenate(scans), [pc_register.IDENTITY] * len(scans)
    monkeypatch.setattr(pc_register, "register_rows", fake)
    np.random.seed(0)
    Dataset("pc_normal", [str(tmp_path / "chair")], register_dist=0.25, coarse_radius=0.5, coarse_iters=512)
    assert seen == dict(coarse=(0.5, 1024, 512, None), names=["a", "b"], dist=0.25)


# ---- the whole algorithm on the restatement ------------------------------------------------------------------------------------------------
def test_the_fixture():
    a, b = CR.scans(3)
    assert a.dtype == b.dtype == np.float32 and a.shape[1] == b.shape[1] == 6 and 2400 < a.shape[0] < 2800 and 2400 < b.shape[0] < 2800
    assert np.allclose(np.linalg.norm(a[:, 3:6], axis=1), 1.0, atol=1e-5)
    out = CR.ellipsoid(4096, 0)
    sign = np.sign((a[:, 3:6] * a[:, :3]).sum(1))
    assert 0.2 < (sign > 0).mean() < 0.8                               # the normals are UNORIENTED: about half point inward
    assert out[:, 0].min() < -0.35 and out[:, 0].max() > 0.35          # both cuts remove something: each scan misses what the other has
    R, t = CR.true_pose(3)
    assert abs(np.degrees(np.arccos((np.trace(R) - 1) / 2)) - 120.0) < 1e-9 and CR.scans(3)[0] is a


def test_accuracy_of_the_restatement_gives_the_gpu_bounds():
    worst = {"coarse": [0.0, 0.0], "icp": [0.0, 0.0]}
    stats = []
    for s in CR.SEEDS:
        b = CR.scans(s)[1]
        c, r = CR.coarse_ref(s), CR.icp_ref(s)
        stats.append((c["mutual"], c["triples"], c["count"], r["iterations"], r["share"]))
        assert abs(c["angle"] - (30.0 + 30.0 * s)) < 6.0                # the turn it reports is the turn the scan was given, to within the coarse error
        for kind, pose in (("coarse", c["pose"]), ("icp", r["pose"])):
            angle, move = RR.pose_errors(pose, CR.true_pose(s), b[:, :3])
            worst[kind] = [max(worst[kind][0], angle), max(worst[kind][1], move)]
        assert RR.pose_errors(c["pose"], CR.true_pose(s), b[:, :3])[1] < CR.ICP_DIST      # the coarse pose puts every row within D of its place
    m = np.array(stats)
    print(f"mutual {m[:, 0].min():.0f} .. {m[:, 0].max():.0f}, triples {m[:, 1].min():.0f} .. {m[:, 1].max():.0f}, counts {m[:, 2].min():.0f} .. {m[:, 2].max():.0f}, "
          f"ICP iterations {m[:, 3].min():.0f} .. {m[:, 3].max():.0f}, shares {m[:, 4].min():.3f} .. {m[:, 4].max():.3f}")
    for kind in worst:
        print(f"{kind}: worst rotation error {worst[kind][0]:.4e} rad, worst displacement {worst[kind][1]:.4e}")
        assert worst[kind][0] <= WORST[kind][0] and worst[kind][1] <= WORST[kind][1]
        assert worst[kind][0] >= WORST[kind][0] / 2 and worst[kind][1] >= WORST[kind][1] / 2    # and the recorded figures are not slack
    assert m[:, 2].min() >= pc_coarse.MIN_AGREE and m[:, 4].min() >= 0.3


@pytest.mark.parametrize("s", [3, 5])
def test_without_the_coarse_stage_icp_refuses_the_same_scans(s):
    """The point of the feature: from the identity, ICP at the same D finds no pair (seed 3, the GPU test's) or too little overlap (seed 5) and says so."""
    with pytest.raises(ValueError, match="do the scans start within --register_dist of each other"):
        CR.icp_ref(s, coarse=False)
