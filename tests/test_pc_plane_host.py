"""Dominant-plane removal (`--plane_threshold`, meshanything_amd/pc_plane.py) without a GPU: the numpy restatement (tests/pc_plane_ref.py)
against float64 geometry on hand-made planes, the row exactly on the threshold included; the degenerate triples; the scene the GPU tests
rest on; `draw_triples` and `fit_plane`; every refusal that comes before the first device call; the C ABI's argument errors; the command
line's new flags; the `Dataset` argument checks."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import pc_plane_ref as PR
import pc_normals_ref as PN

REPO = PR.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, pc_plane                   # noqa: E402
from meshanything_amd.data import Dataset                            # noqa: E402

F32 = np.float32


# ---- the restatement against float64 geometry -------------------------------------------------------------------------------------------------
def test_the_row_on_the_threshold_is_an_inlier_and_the_next_float_is_not():
    above = np.nextafter(F32(0.25), F32(1))
    cloud = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.5, 0.5, 0.25], [0.5, 0.5, above], [1, 1, -0.25], [1, 1, -above], [7, -3, 0.125]], F32)
    planes, counts, best = PR.score_ref(cloud, [[0, 1, 2]], 0.25)
    assert planes.tolist() == [[0, 0, 0, 0, 0, 4]] and best == 0
    rhs, deg = PR.rhs_of(planes[:, 3:], 0.25)
    assert rhs.tolist() == [1.0] and not deg.any()                   # t2 = 1/16, len2 = 16: s*s = 16 * z*z = 1 exactly at z = 1/4
    assert PR.inliers_ref(cloud, planes[0], 0.25).tolist() == [True, True, True, True, False, True, False, True]
    assert counts.tolist() == [6]


def test_restatement_agrees_with_float64_geometry_away_from_the_threshold():
    g = np.random.default_rng(0)
    cloud = g.uniform(-1, 1, (4000, 3)).astype(F32)
    tri = g.integers(0, 4000, (50, 3)).astype(np.int32)
    planes, counts, best = PR.score_ref(cloud, tri, 0.1)
    assert (counts > 0).all() and counts[best] == counts.max() and (counts[:best] < counts[best]).all()
    for h in range(50):
        dist = np.abs(PR.distance64(cloud, planes[h]))
        far = np.abs(dist - 0.1) > 1e-4                              # float32 rounding of s moves the decision by far less than that
        assert np.array_equal(PR.inliers_ref(cloud, planes[h], 0.1)[far], (dist <= 0.1)[far])
        assert far.sum() > 3900
    # a normal of any length: the same rows
    dist = np.abs(PR.distance64(cloud, planes[0]))
    far = np.abs(dist - 0.1) > 1e-4
    for scale in (2.0 ** -40, 3.0, 2.0 ** 30):
        scaled = planes[0] * np.array([1, 1, 1, scale, scale, scale], F32)
        assert np.array_equal(PR.inliers_ref(cloud, scaled, 0.1)[far], (dist <= 0.1)[far])


def test_degenerate_triples():
    cloud, tri, t, (planes, counts, best), expect = PR.lattice_case()
    assert np.array_equal(counts, expect) and counts.tolist().count(-1) == 5 and 0 <= best < 30 and counts[best] == 300
    assert (planes[-2:] == 0).all()                                  # an index equal to N, a negative index: six zeros, nothing read
    assert (planes[-5:-2, 3:] == 0).all()                            # collinear lattice points and a repeated index: the normal is exactly 0
    assert not PR.inliers_ref(cloud, planes[-5:], t).any()           # a degenerate plane has no inliers, not even its own point
    _, counts, best = PR.degenerate_case()[3]
    assert (counts == -1).all() and best == -1
    # rhs that is not finite: a huge normal
    rhs, deg = PR.rhs_of(np.array([[1e20, 0, 0], [0, 0, 0], [np.nan, 1, 1], [1e-30, 0, 0]], F32), 1.0)
    assert deg.tolist() == [True, True, True, True]                  # overflow, zero, NaN, and a len2 that underflows to 0
    cloud, tri, t, (planes, counts, best) = PR.nonfinite_case()
    assert counts[2:5].tolist() == [-1, -1, -1] and counts[0] > 0
    inl = PR.inliers_ref(cloud, planes[0], 10.0)                     # every finite row lies within 10: the NaN and the Inf row alone are out
    assert inl.sum() == 255 and not inl[5] and not inl[9]


def test_twin_hypotheses_and_the_scene():
    _, tri, _, (_, counts, best) = PR.twin_case()
    assert np.array_equal(tri[3], tri[10]) and best == 3 and counts[3] == counts[10] >= 1500 and (np.delete(counts, [3, 10]) < 1500).all()
    xyz, normals, kind = PR.scene(0)
    kept, found, stopped = PR.scene_reference()
    M = xyz.shape[0]
    print(f"scene: {M} rows, table {int((kind == 0).sum())}, best plane {found[0]['first']} inliers ({found[0]['first'] / M:.3f} of the rows, "
          f"{found[0]['ties']} hypotheses tie), refit {found[0]['refit']}, {kept.shape[0]} survive, gap {found[0]['gap'] / PR.SCENE_T:.3f} t")
    assert xyz.dtype == F32 and 14700 < M < 14850 and int((kind == 0).sum()) == 6000 and not stopped and len(found) == 1
    assert (kind[np.setdiff1d(np.arange(M), kept)] == 0).sum() == 6000           # the whole table went, with the sphere's foot
    assert (kind[kept] == 1).all() and 6100 < found[0]["count"] < 6200 and 0.4 < found[0]["count"] / M < 0.43
    assert found[0]["refit"] >= found[0]["first"] - 5 and found[0]["gap"] >= 0.2 * PR.SCENE_T
    kept, found, stopped = PR.scene_reference(0, 0.5)
    assert stopped and found == [] and kept.shape[0] == M


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------------
def test_draw_triples_is_private_and_deterministic():
    np.random.seed(5)
    before = np.random.get_state()
    a = pc_plane.draw_triples(1000, 64, 0)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert a.dtype == np.int32 and a.shape == (64, 3) and a.min() >= 0 and a.max() < 1000
    assert np.array_equal(a, pc_plane.draw_triples(1000, 64, 0)) and np.array_equal(a, PR.draw_ref(1000, 64, 0))
    assert not np.array_equal(a, pc_plane.draw_triples(1000, 64, 1))
    assert np.array_equal(a, np.random.Generator(np.random.PCG64([0x706c616e65, 0])).integers(0, 1000, (64, 3)).astype(np.int32))
    assert (pc_plane.draw_triples(1, 5, 0) == 0).all()
    for bad in ((0, 64, 0), (1000, 0, 0), (1000, 65537, 0), (1000, 64, -1), (1000.0, 64, 0), (True, 64, 0)):
        with pytest.raises(ValueError):
            pc_plane.draw_triples(*bad)


def test_fit_plane_on_exact_dyadic_moments():
    # the four rows (+-1, +-2, 0) about a = (0.5, 0.25, 4): every moment is a dyadic number, exact in float64
    rows = np.array([[1, 2, 0], [1, -2, 0], [-1, 2, 0], [-1, -2, 0]], np.float64)
    a = np.array([0.5, 0.25, 4.0])
    q = rows - a
    m = np.array([4, *q.sum(0), (q[:, 0] ** 2).sum(), (q[:, 0] * q[:, 1]).sum(), (q[:, 0] * q[:, 2]).sum(), (q[:, 1] ** 2).sum(), (q[:, 1] * q[:, 2]).sum(),
                  (q[:, 2] ** 2).sum()])
    assert np.array_equal(m, PR.moments_ref(rows, np.ones(4, bool), a)[0])
    c, n = pc_plane.fit_plane(m, a)
    assert c.dtype == F32 and n.dtype == F32 and c.tolist() == [0, 0, 0] and np.abs(n).tolist() == [0, 0, 1]   # covariance diag(1, 4, 0)
    c, n = pc_plane.fit_plane(np.zeros(10), a)                       # no rows: a degenerate plane
    assert n.tolist() == [0, 0, 0]
    assert pc_plane.fit_plane(np.full(10, np.nan), a)[1].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        pc_plane.fit_plane(np.zeros(9), a)
    # and against the restatement's refit on the scene's first plane
    xyz = PR.scene(0)[0]
    plane = PR.scene_reference()[1][0]["plane"]
    mom = PR.moments_ref(xyz, PR.inliers_ref(xyz, plane, PR.SCENE_T), plane[:3])[0]
    c, n = pc_plane.fit_plane(mom, plane[:3])
    c2, n2 = PR.fit_ref(mom, plane[:3])
    assert np.array_equal(c, c2) and np.array_equal(n, n2) and abs(float(np.linalg.norm(n.astype(np.float64))) - 1) < 1e-6
    assert np.abs(PR.distance64(xyz[PR.scene(0)[2] == 0], np.concatenate([c, n]))).max() < 0.3 * PR.SCENE_T    # the table lies within 0.2 t of its plane


# ---- refusals before the first device call ------------------------------------------------------------------------------------------------------
def test_score_and_apply_refusals_come_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    tri = torch.zeros((8, 3), dtype=torch.int32)
    for p, t, thr, kw in [(pts.double(), tri, 0.1, {}), (torch.zeros((100, 4)), tri, 0.1, {}), (torch.zeros(100), tri, 0.1, {}), (np.zeros((100, 3), F32), tri, 0.1, {}),
                          (pts[:2], tri, 0.1, {}), (pts, tri, 0.0, {}), (pts, tri, -0.1, {}), (pts, tri, float("nan"), {}), (pts, tri, float("inf"), {}),
                          (pts, tri, "0.1", {}), (pts, tri, True, {}), (pts, tri, 1e-50, {}), (pts, tri[:0], 0.1, {}), (pts, torch.zeros((65537, 3), dtype=torch.int32), 0.1, {}),
                          (pts, tri.long(), 0.1, {}), (pts, tri[:, :2], 0.1, {}), (pts, np.zeros((8, 3), np.int32), 0.1, {}), (pts, tri, 0.1, {"want": ()}),
                          (pts, tri, 0.1, {"want": ("counts", "mask")})]:
        with pytest.raises(ValueError):
            pc_plane.score_planes(p, t, thr, **kw)
    for kw in ({}, {"want": "planes"}, {"want": pc_plane.SCORE_WANT}):
        with pytest.raises(ValueError, match="CUDA tensor"):         # a valid call stops at the device check: no CPU fallback
            pc_plane.score_planes(pts, tri, 0.1, **kw)
    plane = [0, 0, 0, 0, 0, 1]
    for p, pl, thr, kw in [(pts.double(), plane, 0.1, {}), (pts[:2], plane, 0.1, {}), (pts, plane[:5], 0.1, {}), (pts, "plane", 0.1, {}), (pts, plane, 0.0, {}),
                           (pts, plane, float("nan"), {}), (pts, plane, float("inf"), {}), (pts, plane, -1.0, {}), (pts, plane, 0.1, {"want": ()}),
                           (pts, plane, 0.1, {"want": ("mask", "best")})]:
        with pytest.raises(ValueError):
            pc_plane.apply_plane(p, pl, thr, **kw)
    for kw in ({}, {"want": "moments"}, {"want": pc_plane.APPLY_WANT}):
        with pytest.raises(ValueError, match="CUDA tensor"):
            pc_plane.apply_plane(pts, plane, 0.1, **kw)


def test_remove_planes_checks_its_arguments_first():
    good = np.zeros((5000, 3), F32)
    nan = good.copy()
    nan[17, 1] = np.nan
    for bad, kw in [(np.zeros((5000, 2), F32), {}), (np.zeros(5000, F32), {}), (np.zeros((5000, 3), np.int32), {}), (nan, {}), (good[:2], {}),
                    (good, {"threshold": 0.0}), (good, {"threshold": float("nan")}), (good, {"iters": 0}), (good, {"iters": 65537}), (good, {"iters": 2.5}),
                    (good, {"count": 0}), (good, {"count": 9}), (good, {"min_fraction": 0.0}), (good, {"min_fraction": 1.5}), (good, {"min_fraction": float("nan")}),
                    (np.lib.stride_tricks.as_strided(np.zeros(3, F32), ((1 << 22) + 1, 3), (0, 4)), {})]:
        args = dict(threshold=0.1, iters=64, count=1, min_fraction=0.2, n_points=4096, uid="x")
        args.update(kw)
        with pytest.raises(ValueError):
            pc_plane.remove_planes(bad, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_plane.remove_planes(good, 0.1, 64, 1, 0.2, 4096, "x", device="cpu")


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    a256 = lambda n: (n + 255) // 256 * 256                          # noqa: E731
    size = lib.ma_pc_plane_workspace_bytes
    assert size(4096, 1024) == a256(4 * 10 * 8) + a256(4 * 4) + 1024 * 32          # four workgroups' partials and counts, eight floats a hypothesis
    assert size(3, 1) > 0 and size(1 << 22, 1 << 16) < 4 << 20
    for N, H in [(2, 1), ((1 << 22) + 1, 1), (100, 0), (100, (1 << 16) + 1), (-1, 5), (100, -1)]:
        assert size(N, H) == 0, (N, H)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    big = 1 << 30
    plane = (C.c_float * 6)(0, 0, 0, 0, 0, 1)

    def bad(fn, word, *args):
        assert getattr(lib, fn)(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    s = "ma_op_pc_plane_score"
    bad(s, "null", None, 100, 3, p, 8, 0.1, p, p, p, p, big, None)
    bad(s, "null", p, 100, 3, None, 8, 0.1, p, p, p, p, big, None)
    bad(s, "null", p, 100, 3, p, 8, 0.1, p, None, p, p, big, None)
    bad(s, "null", p, 100, 3, p, 8, 0.1, p, p, None, p, big, None)
    bad(s, "null", p, 100, 3, p, 8, 0.1, p, p, p, None, big, None)
    bad(s, "3 <= N", p, 2, 3, p, 8, 0.1, p, p, p, p, big, None)
    bad(s, "2^22", p, (1 << 22) + 1, 3, p, 8, 0.1, p, p, p, p, big, None)
    bad(s, "H <= 2^16", p, 100, 3, p, 0, 0.1, p, p, p, p, big, None)
    bad(s, "H <= 2^16", p, 100, 3, p, (1 << 16) + 1, 0.1, p, p, p, p, big, None)
    bad(s, "ref_ld", p, 100, 4, p, 8, 0.1, p, p, p, p, big, None)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        bad(s, "threshold", p, 100, 3, p, 8, t, p, p, p, p, big, None)
    bad(s, "workspace", p, 100, 3, p, 8, 0.1, p, p, p, p, size(100, 8) - 1, None)
    a = "ma_op_pc_plane_apply"
    bad(a, "null", None, 100, 3, plane, 0.1, p, p, p, p, big, None)
    bad(a, "null", p, 100, 3, None, 0.1, p, p, p, p, big, None)
    bad(a, "null", p, 100, 3, plane, 0.1, p, p, p, None, big, None)
    bad(a, "at least one", p, 100, 3, plane, 0.1, None, None, None, p, big, None)
    bad(a, "3 <= N", p, 2, 3, plane, 0.1, p, p, p, p, big, None)
    bad(a, "2^22", p, (1 << 22) + 1, 3, plane, 0.1, p, p, p, p, big, None)
    bad(a, "ref_ld", p, 100, 5, plane, 0.1, p, p, p, p, big, None)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        bad(a, "threshold", p, 100, 3, plane, t, p, p, p, p, big, None)
    bad(a, "workspace", p, 100, 3, plane, 0.1, p, p, p, p, size(100, 1) - 1, None)


# ---- the input side and the command line ----------------------------------------------------------------------------------------------------------
def _sphere_file(tmp_path):
    p, n = PN.sphere(5000, seed=2)
    path = str(tmp_path / "sphere.npy")
    np.save(path, np.concatenate([p, n.astype(F32)], 1))
    return path


def test_dataset_with_plane_removal_off_consumes_the_rng_as_before(tmp_path):
    path = _sphere_file(tmp_path)
    np.random.seed(11)
    plain = Dataset("pc_normal", [path])
    state_plain = np.random.get_state()
    np.random.seed(11)
    off = Dataset("pc_normal", [path], plane_threshold=0.0, plane_iters=7, plane_count=3, plane_min_fraction=0.9)
    state_off = np.random.get_state()
    assert plain.data[0]["pc_normal"].tobytes() == off.data[0]["pc_normal"].tobytes()
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    assert sorted(off[0]) == ["pc_normal", "uid"]


def test_dataset_refusals_come_before_a_file_is_read(tmp_path):
    missing = str(tmp_path / "not_there.npy")                        # reading it would be a FileNotFoundError
    with pytest.raises(ValueError, match="mesh"):
        Dataset("mesh", [missing], plane_threshold=0.1)
    for kind in ("pc_normal", "pc_xyz"):
        for kw in ({"plane_threshold": -0.1}, {"plane_threshold": float("nan")}, {"plane_threshold": float("inf")}, {"plane_threshold": 0.1, "plane_iters": 0},
                   {"plane_threshold": 0.1, "plane_iters": 65537}, {"plane_threshold": 0.1, "plane_count": 0}, {"plane_threshold": 0.1, "plane_count": 9},
                   {"plane_threshold": 0.1, "plane_min_fraction": 0.0}, {"plane_threshold": 0.1, "plane_min_fraction": 1.01}):
            with pytest.raises(ValueError):
                Dataset(kind, [missing], **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):
            Dataset(kind, [_sphere_file(tmp_path)], plane_threshold=0.1, sample_device="cpu")


def test_command_line_flags(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert (a.plane_threshold, a.plane_iters, a.plane_count, a.plane_min_fraction) == (0.0, 1024, 1, 0.2)
    a = main.get_args(base + ["--input_type", "pc_normal", "--plane_threshold", "0.02", "--plane_iters", "65536", "--plane_count", "8", "--plane_min_fraction", "1"])
    assert (a.plane_threshold, a.plane_iters, a.plane_count, a.plane_min_fraction) == (0.02, 65536, 8, 1.0)
    assert main.get_args(base + ["--input_type", "pc_xyz", "--plane_threshold", "2"]).plane_iters == 1024
    assert main.get_args(base + ["--input_type", "mesh", "--plane_threshold", "0"]).plane_threshold == 0.0
    on = ["--input_type", "pc_xyz", "--plane_threshold", "0.1"]
    for bad, word in [(["--input_type", "pc_xyz", "--plane_threshold", "-1"], "--plane_threshold"), (["--input_type", "pc_xyz", "--plane_threshold", "nan"], "--plane_threshold"),
                      (["--input_type", "pc_xyz", "--plane_threshold", "inf"], "--plane_threshold"),
                      (on + ["--plane_iters", "0"], "--plane_iters"), (on + ["--plane_iters", "65537"], "--plane_iters"),
                      (on + ["--plane_count", "0"], "--plane_count"), (on + ["--plane_count", "9"], "--plane_count"),
                      (on + ["--plane_min_fraction", "0"], "--plane_min_fraction"), (on + ["--plane_min_fraction", "1.5"], "--plane_min_fraction"),
                      (on + ["--plane_min_fraction", "nan"], "--plane_min_fraction"),
                      (["--input_type", "pc_xyz", "--plane_iters", "64"], "need --plane_threshold"),
                      (["--input_type", "pc_xyz", "--plane_count", "2"], "need --plane_threshold"),
                      (["--input_type", "pc_xyz", "--plane_min_fraction", "0.3"], "need --plane_threshold"),
                      (["--input_type", "mesh", "--plane_threshold", "0.1"], "mesh"), (["--input_type", "mesh", "--plane_iters", "64"], "mesh"),
                      (["--input_type", "mesh", "--plane_count", "1"], "mesh"), (["--input_type", "mesh", "--plane_min_fraction", "0.2"], "mesh")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err
