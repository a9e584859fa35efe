"""Alignment to the tightest box (`--align_iters`, meshanything_amd/pc_align.py) without a GPU: the numpy restatement
(tests/pc_align_ref.py) against a float64 brute force; the cube's rotations, the nearest representative and the draws; the whole search on
the restatement (a turned box, a tilted box, a ball); `align_rows` with `box_extents` standing on the restatement; `data.to_file_frame`; the
step's place after `cloud_prep.STAGES` through `Dataset` with stand-ins for the GPU functions; that `align_iters=0` leaves the numpy RNG and
the imported modules as they were; and the command line.

The bounds of the search tests, measured on the CPU over the seeds 0..7 of `pc_align_ref.box_surface(6000, seed)` with iters 4 096 and
rounds 4: the worst volume excess V_best / 0.18 - 1 was 4.13e-4 (all eight within 4.04e-4..4.13e-4; the spacing of the last round is
1.5e-4 rad and the box's extent ratios sum to 8.4, so about 1e-3 was to be expected), the worst angle to the nearest cube rotation
9.53e-5 rad, and 7.53e-5 rad to the identity for the 10 degree tilt.  TAU and ALPHA are twice the worst."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

import pc_align_ref as R

REPO = R.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build, cloud_prep, data, pc_align, pc_cluster, pc_fps, pc_normals, pc_upsample   # noqa: E402
from meshanything_amd.data import Dataset                         # noqa: E402

TAU = 2 * 4.13e-4
ALPHA = 2 * 9.53e-5
ITERS, ROUNDS = 4096, 4


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_a_float64_brute_force():
    cloud, rot, centre, (ext, vol, best) = R.uniform_case(257, 6, 65)
    assert ext.dtype == np.float32 and ext.shape == (65, 6) and vol.dtype == np.float64 and vol.shape == (65,)
    want = R.brute64(cloud, rot, centre)
    size = np.tile(want[:, 3:] - want[:, :3], 2)                     # per axis the extent, whose ulp is the unit
    assert (np.abs(ext.astype(np.float64) - want) <= 4 * np.spacing(size.astype(np.float32)).astype(np.float64)).all()
    assert best == int(np.argmin(vol)) and np.isfinite(vol).all()
    assert np.allclose(vol, np.prod(want[:, 3:] - want[:, :3], axis=1), rtol=1e-5)
    assert _same(ext[0], np.concatenate([(cloud[:, :3] - centre).min(0), (cloud[:, :3] - centre).max(0)]))   # index 0 is the identity


def test_restatement_on_the_content_cases():
    cases = R.content_cases()
    ext, vol, best = cases["at_centre"][3]
    assert (ext == 0).all() and not np.signbit(ext).any() and (vol == 0).all() and best == 0
    ext, vol, best = cases["minus_zero"][3]
    assert not np.signbit(ext[ext == 0]).any() and (ext == 0).sum() >= 14
    assert cases["twin"][3][2] == 4 and cases["twin"][3][1][4] == cases["twin"][3][1][13]
    ext, vol, best = cases["nan_entry"][3]
    assert np.isinf(vol).tolist() == [False, False, True, False, False, True, False, False, False] and np.isnan(ext[[2, 5]]).all() and best not in (2, 5)
    ext, vol, best = cases["overflow"][3]
    assert np.isinf(vol[3]) and np.isfinite(vol[[1, 6]]).all() and np.isinf(vol).sum() >= 3 and np.isfinite(vol[best]) and np.isnan(ext[3]).all()
    ext, vol, best = cases["all_bad"][3]
    assert best == -1 and np.isinf(vol).all() and (vol > 0).all() and np.isnan(ext).all()


# ---- rotations ------------------------------------------------------------------------------------------------------------------------------
def test_cube_rotations():
    cube = pc_align.cube_rotations()
    assert cube.shape == (24, 3, 3) and cube.dtype == np.float64 and _same(cube[0], np.eye(3))
    keys = {c.tobytes() for c in (cube + 0.0)}
    assert len(keys) == 24
    for c in cube:
        assert np.array_equal(c @ c.T, np.eye(3)) and np.linalg.det(c) == pytest.approx(1.0, abs=1e-15)
        assert set(np.abs(c).sum(0).tolist()) == {1.0} and set(np.abs(c).sum(1).tolist()) == {1.0}
    for a in cube:
        for b in cube:
            assert ((a @ b) + 0.0).tobytes() in keys                 # closed under the product
    assert _same(cube, pc_align.cube_rotations())


def test_nearest_representative():
    cube = pc_align.cube_rotations()
    assert _same(pc_align.nearest_representative(np.eye(3)), np.eye(3))
    Rz = R.R_10Z
    assert _same(pc_align.nearest_representative(Rz), Rz)
    for seed in range(20):
        M = pc_align.draw_rotations(30, 0)[1 + seed]
        got = pc_align.nearest_representative(M)
        traces = np.trace(cube @ M, axis1=1, axis2=2)
        assert np.trace(got) >= traces.max() and _same(got, (cube @ M)[int(np.argmax(traces))])
        assert R.angle_between(got, np.eye(3)) <= np.radians(63)     # no rotation is farther than 62.8 degrees from the nearest of the 24
    for c in cube:                                                   # every equivalent of a frame near the file's comes back to it
        assert np.abs(pc_align.nearest_representative(c @ Rz) - Rz).max() < 1e-15
    with pytest.raises(ValueError):
        pc_align.nearest_representative(np.eye(4))


def test_draw_rotations():
    state = np.random.get_state()
    first = pc_align.draw_rotations(500, 0)
    assert first.shape == (500, 3, 3) and first.dtype == np.float64 and _same(first, pc_align.draw_rotations(500, 0)) and _same(first[0], np.eye(3))
    about = first[7]
    ball = pc_align.draw_rotations(500, 2, about=about, radius=0.05)
    assert _same(ball, pc_align.draw_rotations(500, 2, about=about, radius=0.05)) and _same(ball[0], about)
    assert not _same(ball, pc_align.draw_rotations(500, 3, about=about, radius=0.05))
    for rots in (first, ball):
        assert np.abs(rots @ rots.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(rots) - 1).max() < 1e-12
    angles = np.array([R.angle_between(m, about) for m in ball])
    assert angles.max() <= 0.05 + 1e-12 and angles.max() > 0.045 and np.median(angles) > 0.03   # uniform in the ball: half the volume lies beyond 0.79 of the radius
    far = np.array([R.angle_between(m, np.eye(3)) for m in first[1:]])
    assert far.max() > 3.0 and 1.9 < far.mean() < 2.4                # uniform over the rotations: the mean angle is pi / 2 + 2 / pi = 2.21
    now = np.random.get_state()
    assert np.array_equal(state[1], now[1]) and state[2:] == now[2:]
    for bad in [dict(H=0, round=0), dict(H=(1 << 16) + 1, round=0), dict(H=10, round=-1), dict(H=10, round=0, about=np.eye(3)), dict(H=10, round=1),
                dict(H=10, round=1, about=np.eye(3)), dict(H=10, round=1, about=np.eye(3), radius=0.0), dict(H=10, round=1, about=np.eye(2), radius=0.1)]:
        with pytest.raises(ValueError):
            pc_align.draw_rotations(**bad)


def test_radii_follow_from_the_hypothesis_count():
    got = pc_align.radii(4096, 4)
    s0 = (8 * np.pi ** 2 / 24 / 4096) ** (1 / 3)
    f = 2 * (4 * np.pi / 3 / 4096) ** (1 / 3)
    assert np.allclose(got, [2 * s0, 2 * s0 * f, 2 * s0 * f ** 2, 2 * s0 * f ** 3], rtol=1e-14) and pc_align.radii(4096, 0) == []
    assert 1.4e-4 < got[3] * f / 2 < 1.6e-4                          # the spacing of the last round
    assert pc_align.radii(256, 8)[0] <= np.pi


# ---- the search, on the restatement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    xyz, normals = R.box_surface(6000, 0)
    return xyz, normals


def test_search_finds_the_turned_box(box):
    cloud = R.turn(box[0], R.R_25).astype(np.float32)
    Rp, v_identity, v_best = pc_align.search(R.score_of(cloud), ITERS, ROUNDS, 0.02)
    excess, angle = v_best / R.BOX_VOLUME - 1, R.angle_to_cube(Rp @ R.R_25, pc_align.cube_rotations())
    print(f"volume excess {excess:.3e} (bound {TAU:.3e}), angle to the nearest cube rotation {angle:.3e} rad (bound {ALPHA:.3e}), identity volume {v_identity:.4f}")
    assert TAU <= 2e-2 and v_best <= (1 + TAU) * R.BOX_VOLUME
    assert angle <= ALPHA
    assert v_identity > 3 * R.BOX_VOLUME and np.abs(Rp @ Rp.T - np.eye(3)).max() < 1e-12
    assert _same(Rp, pc_align.nearest_representative(Rp))            # of the 24 equivalents the one nearest the file's frame


def test_search_keeps_up_for_a_tilted_box(box):
    cloud = R.turn(box[0], R.R_10Z, shift=(3.0, -2.0, 5.0)).astype(np.float32)
    Rp, v_identity, v_best = pc_align.search(R.score_of(cloud), ITERS, ROUNDS, 0.02)
    angle = R.angle_between(Rp @ R.R_10Z, np.eye(3))
    print(f"angle to the identity {angle:.3e} rad (bound {ALPHA:.3e}), volume excess {v_best / R.BOX_VOLUME - 1:.3e}")
    assert angle <= ALPHA                                            # the IDENTITY among the 24: up stays up
    assert v_best < v_identity


def test_search_leaves_a_ball_alone():
    cloud = R.ball(6000, 0).astype(np.float32)
    seen = []

    def score(rot32):
        seen.append(R.score_of(cloud)(rot32))
        return seen[-1]
    Rp, v_identity, v_best = pc_align.search(score, ITERS, ROUNDS, 0.02)
    gain = 1 - v_best / v_identity
    print(f"the best gain on the ball: {gain:.4f}")
    assert 0 <= gain < 0.02 and len(seen) == 1 + ROUNDS              # the restatement's best gain really is under the default
    assert _same(Rp, np.eye(3))
    assert all(v[vol_best] == v.min() for v, vol_best in seen) and seen[-1][0].min() == v_best
    assert [float(v[0]) for v, _ in seen[1:]] == [float(v.min()) for v, _ in seen[:-1]]   # index 0 reproduces the best so far, bit for bit
    Rp0, _, v0 = pc_align.search(R.score_of(cloud), ITERS, ROUNDS, 0.0)   # with no floor the same search does turn it
    assert v0 == v_best and not _same(Rp0, np.eye(3))


def test_search_with_every_hypothesis_bad_is_the_identity():
    Rp, v_identity, v_best = pc_align.search(lambda rot32: (np.full(rot32.shape[0], np.inf), -1), 256, 2, 0.02)
    assert _same(Rp, np.eye(3)) and v_identity == np.inf


def test_check_align_args():
    assert pc_align.check_align_args(256) == (256, 4, 0.02) and pc_align.check_align_args(np.int64(65536), 0, 0) == (65536, 0, 0.0)
    assert pc_align.check_align_args(4096, 8, 0.999) == (4096, 8, 0.999)
    for bad in [(255,), (65537,), (4096.0,), (True,), ("4096",), (4096, -1), (4096, 9), (4096, 2.0), (4096, 4, -0.01), (4096, 4, 1.0), (4096, 4, float("nan")),
                (4096, 4, "0.1"), (4096, 4, None)]:
        with pytest.raises(ValueError, match="iters|rounds|min_gain"):
            pc_align.check_align_args(*bad)


# ---- align_rows -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def on_the_restatement(monkeypatch):
    """`box_extents` answers from the restatement and the uploads stay on the host; what it was asked is logged"""
    log = []

    def box_extents(points, rotations, centre, want=("volumes", "best")):
        log.append((tuple(points.shape), points.dtype, tuple(rotations.shape), np.asarray(centre).copy(), tuple(want)))
        _, vol, best = R.extents_ref(points.numpy(), rotations.numpy(), centre)
        return {"volumes": torch.from_numpy(vol), "best": torch.tensor([best], dtype=torch.int32)}
    monkeypatch.setattr(pc_align, "box_extents", box_extents)
    monkeypatch.setattr(pc_align, "_upload", lambda array, dev: (log.append(("upload", str(dev))), torch.from_numpy(array))[1])
    return log


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_align_rows_turns_points_and_normals(on_the_restatement, capsys, box, dtype):
    xyz, normals = box
    shift = np.array([3.0, -2.0, 5.0])
    rows = np.concatenate([R.turn(xyz[:1500], R.R_25, shift), normals[:1500] @ R.R_25.T, np.arange(3000.0).reshape(1500, 2) % 7], 1).astype(dtype)
    before = rows.copy()
    got, (Rp, c) = pc_align.align_rows(rows, 1024, 3, 0.02, "scan", device="cuda:1")
    assert _same(rows, before) and got is not rows
    assert got.dtype == (np.float32 if dtype == np.float16 else dtype) and got.shape == rows.shape
    assert _same(got[:, 6:], rows[:, 6:].astype(got.dtype))          # further columns are copied
    x32 = rows[:, :3].astype(np.float32)
    assert c.dtype == np.float64 and _same(c, ((x32.min(0) + x32.max(0)) / np.float32(2)).astype(np.float64))
    assert Rp.dtype == np.float64 and np.abs(Rp @ Rp.T - np.eye(3)).max() < 1e-12
    want = c + (rows[:, :3].astype(np.float64) - c) @ Rp.T
    assert _same(got[:, :3], want.astype(got.dtype))
    assert _same(got[:, 3:6], (rows[:, 3:6].astype(np.float64) @ Rp.T).astype(got.dtype))
    tol = 2e-3 if dtype == np.float16 else 1e-6
    assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1).max() < tol   # still unit length
    # 1 024 hypotheses in four rounds (a last spacing of 5e-3 rad) leave the box a little off: the normals have turned WITH the points, each
    # along the face its point lies on
    off = R.angle_to_cube(Rp @ R.R_25, pc_align.cube_rotations())
    assert off < 0.05
    M = Rp @ R.R_25                                                   # the box's own frame -> the aligned one
    assert np.abs(got[:, 3:6].astype(np.float64) - normals[:1500] @ M.T).max() < (5e-3 if dtype == np.float16 else 1e-6)
    assert (np.abs(got[:, 3:6].astype(np.float64)).max(1) > np.cos(off) - 5e-3).all()
    uploads = [e for e in on_the_restatement if e[0] == "upload"]
    calls = [e for e in on_the_restatement if e[0] != "upload"]
    assert uploads == [("upload", "cuda:1")] * 5 and len(calls) == 4
    assert all(call[0] == (1500, 3) and call[1] == torch.float32 and call[2] == (1024, 9) and _same(call[3], c.astype(np.float32)) for call in calls)
    line = capsys.readouterr().out
    angle = np.degrees(R.angle_between(Rp, np.eye(3)))
    assert line.startswith(f"scan: alignment turned the cloud {angle:.3f} deg about (") and line.endswith(", 4096 hypotheses\n") and "box volume " in line and " -> " in line
    assert line.count("\n") == 1


def test_align_rows_returns_the_rows_themselves_for_the_identity(on_the_restatement, capsys):
    rows = np.concatenate([R.ball(3000, 1), R.ball(3000, 1)], 1).astype(np.float32)
    got, (Rp, c) = pc_align.align_rows(rows, 256, 1, 0.5, "ball")
    assert got is rows and _same(Rp, np.eye(3)) and c.shape == (3,)
    line = capsys.readouterr().out
    assert line.startswith("ball: alignment kept the file's axes") and "512 hypotheses" in line and line.count("\n") == 1
    xyz_only, _ = pc_align.align_rows(rows[:, :3], 256, 1, 0.5, "ball")
    assert xyz_only.shape == (3000, 3)


def test_align_rows_refusals():
    good = R.ball(300, 2).astype(np.float32)
    nan = good.copy()
    nan[5, 1] = np.nan
    for bad in (good[:, :2], good.astype(np.int32), good[:0], nan):
        with pytest.raises(ValueError):
            pc_align.align_rows(bad, 256, 1, 0.02, "x")
    for args in ((100, 1, 0.02), (256, 9, 0.02), (256, 1, 1.0)):
        with pytest.raises(ValueError, match="iters|rounds|min_gain"):
            pc_align.align_rows(good, *args, "x")
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_align.align_rows(good, 256, 1, 0.02, "x", device="cpu")
    p, r = torch.zeros((10, 3)), torch.zeros((4, 9))
    for pts, rot, centre, kw in [(p, r, (0, 0, 0), {}), (p.double(), r, (0, 0, 0), {}), (torch.zeros((10, 4)), r, (0, 0, 0), {}), (p[:0], r, (0, 0, 0), {}),
                                 (p, r.double(), (0, 0, 0), {}), (p, torch.zeros((4, 8)), (0, 0, 0), {}), (p, r[:0], (0, 0, 0), {}), (p, r.numpy(), (0, 0, 0), {}),
                                 (p, r, (0, 0), {}), (p, r, "abc", {}), (p, r, (0, 0, 0), {"want": ()}), (p, r, (0, 0, 0), {"want": ("volume",)})]:
        with pytest.raises(ValueError):
            pc_align.box_extents(pts, rot, centre, **kw)
    with pytest.raises(ValueError, match="CUDA tensor"):
        pc_align.box_extents(p, r, (0, 0, 0))
    with pytest.raises(ValueError, match="2\\^16"):
        pc_align.box_extents(p, torch.zeros(((1 << 16) + 1, 9)), (0, 0, 0))


def test_c_abi_checks_every_argument_before_hip():
    build.build(force=False, verbose=False)
    lib = _lib.load()
    size = lib.ma_pc_align_workspace_bytes
    assert size(1, 1) == 512 and size(1 << 22, 1 << 16) == (1 << 16) * 40 and size(5000, 9) == 512 + 256
    for N, H in ((0, 1), (1, 0), ((1 << 22) + 1, 1), (1, (1 << 16) + 1), (-1, 5)):
        assert size(N, H) == 0, (N, H)
    p = C.c_void_p(4096)                                             # never dereferenced: every call below fails its checks
    centre = (C.c_float * 3)(0, 0, 0)
    fn = "ma_op_pc_align_extents"

    def bad(word, *args):
        assert getattr(lib, fn)(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith(fn + ":") and word in msg, msg

    bad("null", None, 100, 3, centre, p, 8, p, p, p, p, 1 << 20, None)
    bad("null", p, 100, 3, None, p, 8, p, p, p, p, 1 << 20, None)
    bad("null", p, 100, 3, centre, None, 8, p, p, p, p, 1 << 20, None)
    bad("null", p, 100, 3, centre, p, 8, p, p, p, None, 1 << 20, None)
    bad("at least one", p, 100, 3, centre, p, 8, None, None, None, p, 1 << 20, None)
    bad("N <=", p, 0, 3, centre, p, 8, p, p, p, p, 1 << 20, None)
    bad("N <=", p, (1 << 22) + 1, 3, centre, p, 8, p, p, p, p, 1 << 30, None)
    bad("H <=", p, 100, 3, centre, p, 0, p, p, p, p, 1 << 20, None)
    bad("H <=", p, 100, 3, centre, p, (1 << 16) + 1, p, p, p, p, 1 << 30, None)
    bad("ref_ld", p, 100, 4, centre, p, 8, p, p, p, p, 1 << 20, None)
    bad("ref_ld", p, 100, 0, centre, p, 8, p, p, p, p, 1 << 20, None)
    bad("workspace", p, 100, 3, centre, p, 8, p, p, p, p, 511, None)
    bad("workspace", p, 100, 6, centre, p, 8, None, p, None, p, 0, None)


# ---- the file frame -----------------------------------------------------------------------------------------------------------------------------
def test_to_file_frame():
    g = np.random.default_rng(5)
    verts = g.uniform(-0.5, 0.5, (50, 3)).astype(np.float32)
    centre, scale = g.uniform(-3, 3, 3), 1.7
    old = centre[None, :] + scale * 2.0 * verts.astype(np.float64)   # main.py's expression before the function was factored out
    assert _same(data.to_file_frame(verts, (centre, scale)), old) and _same(data.to_file_frame(verts, (centre, scale), None), old)
    # known points through a pose and back: a file's rows, aligned, normalised, and the "mesh" of those very points
    rows = R.turn(R.box_surface(500, 4)[0], R.R_25, (3.0, -2.0, 5.0))
    Rp, c = pc_align.nearest_representative(R.R_25.T), np.array([3.01, -2.02, 4.97])
    aligned = c + (rows - c) @ Rp.T
    frame = data.pc_frame(aligned)
    mesh = (aligned - frame[0]) / frame[1] / 2.0                     # what the decoder would give for these points: the +-0.5 box
    back = data.to_file_frame(mesh, frame, (Rp, c))
    assert back.dtype == np.float64 and np.abs(back - rows).max() < 1e-12
    assert np.abs(data.to_file_frame(mesh, frame) - aligned).max() < 1e-12


# ---- the step's place -------------------------------------------------------------------------------------------------------------------------
N_POINTS = 4096
DROP_CLUSTER = 50


def origin_of(rows):
    return int(rows[0, 1]), int(rows[0, 0])


@pytest.fixture
def calls(monkeypatch):
    """the stand-ins tests/test_pc_voxel_host.py uses for the GPU calls, and one for align_rows, which marks what it saw in column 2"""
    log = []

    def split_rows(xyz, radius, min_points, mode, uid, device="cuda"):
        log.append(("cluster", uid, origin_of(xyz), xyz.shape[0], None, device))
        half = xyz.shape[0] // 2
        return [np.arange(half), np.arange(half, xyz.shape[0] - DROP_CLUSTER)][:2 if mode == "split" else 1]

    def upsample_rows(rows, radius, target, uid, device="cuda"):
        log.append(("upsample", uid, origin_of(rows), rows.shape[0], target, device))
        return rows if rows.shape[0] >= target else np.concatenate([rows, rows[np.arange(target - rows.shape[0]) % rows.shape[0]]])

    def align_rows(rows, iters, rounds, min_gain, uid, device="cuda"):
        log.append(("align", uid, origin_of(rows), rows.shape[0], (iters, rounds, min_gain), device))
        out = rows.copy()
        out[:, 2] = 7.0
        return out, (R.R_10Z, np.array([1.0, 2.0, 3.0]))

    def fps_rows(xyz, n_points, device="cuda"):
        log.append(("pick", None, origin_of(xyz), xyz.shape[0], float(xyz[0, 2]), device))
        return np.arange(n_points) % xyz.shape[0]

    def xyz_to_pc_normal(xyz, n_points=4096, k=16, device="cuda", sampling="random"):
        log.append(("pick", None, origin_of(xyz), xyz.shape[0], float(xyz[0, 2]), device))
        return np.concatenate([xyz[np.arange(n_points) % xyz.shape[0], :3], np.tile(np.float32([0, 0, 1]), (n_points, 1))], axis=1)

    for module, fn in ((pc_cluster, split_rows), (pc_upsample, upsample_rows), (pc_align, align_rows), (pc_fps, fps_rows), (pc_normals, xyz_to_pc_normal)):
        monkeypatch.setattr(module, fn.__name__, fn)
    return log


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Two files of 20 000 and 18 000 rows: column 0 = the row, column 1 = the file, unit normals"""
    d = tmp_path_factory.mktemp("align_prep")
    paths = []
    for f, (name, n) in enumerate((("first", 20000), ("second", 18000))):
        rows = np.zeros((n, 6), np.float32)
        rows[:, 0], rows[:, 1], rows[:, 5] = np.arange(n), f, 1.0
        paths.append(str(d / f"{name}.npy"))
        np.save(paths[-1], rows)
    return paths


def test_the_stage_list_is_the_six_and_the_pose_stands_beside_it():
    assert [s.switch for s in cloud_prep.STAGES] == ["voxel_size", "outlier_k", "plane_threshold", "cluster_radius", "smooth_radius", "upsample_radius"]
    assert cloud_prep.POSE.switch == "align_iters" and cloud_prep.POSE.module == "pc_align" and cloud_prep.POSE not in cloud_prep.STAGES
    p = cloud_prep.CloudPrep()
    assert (p.align_iters, p.align_rounds, p.align_min_gain) == (0, 4, 0.02) and p.on() == [] and p.pose() == []
    p = cloud_prep.CloudPrep(align_iters=512, voxel_size=0.5)
    assert [s.switch for s, _ in p.on()] == ["voxel_size"] and [(s.switch, m) for s, m in p.pose()] == [("align_iters", pc_align)]


@pytest.mark.parametrize("mode", ["largest", "split"])
@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_alignment_runs_after_upsampling_and_before_the_pick_once_per_part(kind, mode, calls, files):
    for upsample, device in ((False, None), (True, "cuda:3")):
        del calls[:]
        kw = dict(upsample_radius=0.1, cluster_min_points=64) if upsample else {}
        ds = Dataset(kind, files, sample_device=device, point_sampling="fps", cluster_radius=0.1, cluster_mode=mode, align_iters=512, align_rounds=3,
                     align_min_gain=0.1, **kw)
        dev = device or "cuda"
        want = []
        for f, (uid, n) in enumerate((("first", 20000), ("second", 18000))):
            want.append(("cluster", uid, (f, 0), n, None, dev))
            half = n // 2
            parts = [(uid, 0, half)] if mode == "largest" else [(f"{uid}_part0", 0, half), (f"{uid}_part1", half, n - DROP_CLUSTER - half)]
            if upsample:
                want += [("upsample", part, (f, start), m, 4 * N_POINTS, dev) for part, start, m in parts]
                parts = [(part, start, max(m, 4 * N_POINTS)) for part, start, m in parts]
            want += [("align", part, (f, start), m, (512, 3, 0.1), dev) for part, start, m in parts]
            want += [("pick", None, (f, start), m, 7.0, dev) for _, start, m in parts]       # the pick sees what alignment returned
        assert calls == want, (upsample, device)
        assert len(ds) == (2 if mode == "largest" else 4)
        for i in range(len(ds)):
            item = ds[i]
            assert sorted(item) == (["frame", "group", "part", "pc_normal", "pose", "uid"] if mode == "split" else ["pc_normal", "pose", "uid"])
            assert _same(item["pose"][0], R.R_10Z) and item["pose"][1].tolist() == [1.0, 2.0, 3.0] and item["pose"] is ds.data[i]["pose"]


def test_alignment_alone_and_its_refusals(calls, files):
    ds = Dataset("pc_normal", files[:1], point_sampling="fps", align_iters=256)
    assert [c[0] for c in calls] == ["align", "pick"] and calls[0][3:] == (20000, (256, 4, 0.02), "cuda") and len(ds) == 1 and "pose" in ds[0]
    del calls[:]
    with pytest.raises(ValueError, match="align_iters applies to pc_normal and pc_xyz inputs"):
        Dataset("mesh", [], align_iters=256)
    missing = ["/nonexistent/never_read.npy"]                        # refused before a file is read
    for kind in ("pc_normal", "pc_xyz"):
        for kw, word in [(dict(align_iters=255), "iters"), (dict(align_iters=65537), "iters"), (dict(align_iters=-1), "iters"), (dict(align_iters=512.0), "iters"),
                         (dict(align_iters="512"), "iters"), (dict(align_iters=512, align_rounds=9), "rounds"), (dict(align_iters=512, align_rounds=-1), "rounds"),
                         (dict(align_iters=512, align_rounds=1.5), "rounds"), (dict(align_iters=512, align_min_gain=1.0), "min_gain"),
                         (dict(align_iters=512, align_min_gain=-0.1), "min_gain"), (dict(align_iters=512, align_min_gain=float("nan")), "min_gain")]:
            with pytest.raises(ValueError, match=word):
                Dataset(kind, missing, **kw)
    assert calls == []


def test_off_leaves_the_rng_and_the_imports_as_before(files):
    np.random.seed(11)
    plain = Dataset("pc_normal", files[:1])
    state_plain = np.random.get_state()
    np.random.seed(11)
    off = Dataset("pc_normal", files[:1], align_iters=0, align_rounds=2, align_min_gain=0.5)
    state_off = np.random.get_state()
    assert _same(plain.data[0]["pc_normal"], off.data[0]["pc_normal"]) and sorted(off.data[0]) == ["pc_normal", "uid"] and sorted(off[0]) == ["pc_normal", "uid"]
    assert np.array_equal(state_plain[1], state_off[1]) and state_plain[2:] == state_off[2:]
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "import meshanything_amd.data as data\n"
            "assert len(data.Dataset('pc_normal', [sys.argv[2]], align_iters=0)) == 1\n"
            "loaded = sorted(m for m in sys.modules if m.startswith('meshanything_amd.pc_'))\n"
            "assert not loaded and 'torch' not in sys.modules, loaded\n")
    r = subprocess.run([sys.executable, "-c", code, REPO, files[0]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_command_line_flags(capsys):
    import main
    base = ["--input_path", "x.npy"]
    a = main.get_args(base + ["--input_type", "pc_xyz"])
    assert (a.align_iters, a.align_rounds, a.align_min_gain) == (0, 4, 0.02)
    a = main.get_args(base + ["--input_type", "pc_normal", "--align_iters", "4096"])
    assert (a.align_iters, a.align_rounds, a.align_min_gain) == (4096, 4, 0.02)
    a = main.get_args(base + ["--input_type", "pc_xyz", "--align_iters", "256", "--align_rounds", "0", "--align_min_gain", "0", "--voxel_size", "0.5"])
    prep = cloud_prep.CloudPrep.from_args(a)
    assert (prep.align_iters, prep.align_rounds, prep.align_min_gain, prep.voxel_size) == (256, 0, 0.0, 0.5)
    assert main.get_args(base + ["--input_type", "mesh", "--align_iters", "0"]).align_iters == 0
    everything = "--align_iters, --align_rounds and --align_min_gain apply to --input_type pc_normal and pc_xyz, not to mesh inputs"
    for bad, word in [(["--input_type", "pc_xyz", "--align_iters", "-1"], "--align_iters must be finite and >= 0 (0 = off)"),
                      (["--input_type", "pc_xyz", "--align_iters", "255"], "--align_iters must be 0 (off) or in 256..65536"),
                      (["--input_type", "pc_normal", "--align_iters", "65537"], "--align_iters must be 0 (off) or in 256..65536"),
                      (["--input_type", "pc_xyz", "--align_iters", "1e3"], "invalid int value"),
                      (["--input_type", "mesh", "--align_iters", "512"], everything),
                      (["--input_type", "mesh", "--align_rounds", "2"], everything),
                      (["--input_type", "pc_xyz", "--align_rounds", "2"], "--align_rounds and --align_min_gain need --align_iters > 0"),
                      (["--input_type", "pc_xyz", "--align_rounds", "2", "--align_min_gain", "0.1"], "--align_rounds and --align_min_gain need --align_iters > 0"),
                      (["--input_type", "pc_xyz", "--align_iters", "512", "--align_rounds", "9"], "--align_rounds must be in 0..8"),
                      (["--input_type", "pc_xyz", "--align_iters", "512", "--align_rounds", "-1"], "--align_rounds must be in 0..8"),
                      (["--input_type", "pc_xyz", "--align_iters", "512", "--align_min_gain", "1"], "--align_min_gain must be in [0, 1)"),
                      (["--input_type", "pc_xyz", "--align_iters", "512", "--align_min_gain", "nan"], "--align_min_gain must be in [0, 1)")]:
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):
        main.get_args(["--help"])
    out = capsys.readouterr().out
    assert all(f in out and f in main.__doc__ for f in ("--align_iters", "--align_rounds", "--align_min_gain"))
