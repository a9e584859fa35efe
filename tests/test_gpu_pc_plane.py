"""Dominant-plane removal on the MI355X (csrc/pc_plane.hpp, meshanything_amd/pc_plane.py): counts, best and planes against the numpy
restatement `pc_plane_ref.score_ref`, the mask, count and moments of one plane, through `Dataset(..., plane_threshold=...)` and through
`main.py --plane_threshold ...`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

The counts are sums of integer atomics: a function of the inputs alone, so they must EQUAL the restatement's and a second run's.  The
moments come from a reduction of fixed shape: the same bits on two runs, and within n * 2^-52 * sum|term| of numpy's sum.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_plane_ref as PR

pytestmark = pytest.mark.gpu

REPO = PR.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
APPLY_CASES = ((3, 3, 1), (257, 6, 65), (1025, 3, 64), (2500, 6, 300))   # (N, ld, H) of uniform_case: one row group, ..., three groups of 1 024 rows

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_plane_ref as PR
import test_gpu_pc_plane as T
from meshanything_amd import pc_plane
out = {{}}
"""


def _gpu(tmp_path, body, timeout=300):
    """Run `body` (after _PRELUDE) in a fresh interpreter; it fills the dict `out`, which comes back as a dict of arrays, and its stdout."""
    script = tmp_path / "job.py"
    res = tmp_path / "out.npz"
    script.write_text(_PRELUDE + body + f"\nnp.savez({str(res)!r}, **out)\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(res) as z:
        return {k: z[k] for k in z.files}, r.stdout


def named_cases():
    """name -> (cloud, tri, threshold, (planes, counts, best)) of the cases that are not the uniform grid"""
    return {"lattice": PR.lattice_case()[:4], "twin": PR.twin_case(), "degenerate": PR.degenerate_case(), "nonfinite": PR.nonfinite_case()}


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
_SCORE = """
def same(a, b):
    return all(bool(torch.equal(a[w], b[w])) or w == "planes" and bool(torch.equal(a[w].isnan(), b[w].isnan()) and torch.equal(a[w].nan_to_num(), b[w].nan_to_num()))
               for w in a)
def run(name, cloud, tri, t):
    p, q = torch.from_numpy(cloud).cuda(), torch.from_numpy(tri).cuda()
    got = pc_plane.score_planes(p, q, t, want=pc_plane.SCORE_WANT)
    out[name + "_twice"] = np.array(same(got, pc_plane.score_planes(p, q, t, want=pc_plane.SCORE_WANT)))
    alone = pc_plane.score_planes(p, q, t)
    out[name + "_default"] = np.array(sorted(alone) == ["best", "counts"] and same(alone, {w: got[w] for w in alone}))
    for w in got:
        out[name + "_" + w] = got[w].cpu().numpy()
for N in PR.SCORE_N:
    for ld in (3, 6):
        for H in PR.SCORE_H:
            run(f"n{N}_ld{ld}_h{H}", *PR.uniform_case(N, ld, H)[:3])
for name, case in T.named_cases().items():
    run(name, *case[:3])
# a strided view of the cloud and of the triples
cloud, tri, t, _ = PR.uniform_case(2500, 6, 300)
p = torch.from_numpy(cloud).cuda()
wide = torch.cat([p, p], 1)
q = torch.from_numpy(np.concatenate([tri, tri], 1)).cuda()
got = pc_plane.score_planes(wide[:, 6:], q[:, 3:], t, want=pc_plane.SCORE_WANT)
for w in got:
    out["view_" + w] = got[w].cpu().numpy()
# refusals with tensors on the device
p3 = p[:, :3].contiguous()
q = q[:, :3].contiguous()
def refused(fn):
    try:
        fn()
        return ""
    except ValueError as e:
        return str(e)
out["errors"] = np.array([refused(lambda: pc_plane.score_planes(p3, q, 0.0)), refused(lambda: pc_plane.score_planes(p3, q, -1.0)),
                          refused(lambda: pc_plane.score_planes(p3, q, float("nan"))), refused(lambda: pc_plane.score_planes(p3, q, float("inf"))),
                          refused(lambda: pc_plane.score_planes(p3, q[:0], 0.1)), refused(lambda: pc_plane.score_planes(p3, torch.zeros((65537, 3), dtype=torch.int32, device="cuda"), 0.1)),
                          refused(lambda: pc_plane.score_planes(p3[:2], q, 0.1)), refused(lambda: pc_plane.score_planes(p3.cpu(), q.cpu(), 0.1)),
                          refused(lambda: pc_plane.score_planes(p3, q.cpu(), 0.1)),
                          refused(lambda: pc_plane.apply_plane(p3, [0, 0, 0, 0, 0, 1], 0.0)), refused(lambda: pc_plane.apply_plane(p3, [0, 0, 0, 0, 0, 1], float("inf"))),
                          refused(lambda: pc_plane.apply_plane(p3[:2], [0, 0, 0, 0, 0, 1], 0.1)), refused(lambda: pc_plane.apply_plane(p3.cpu(), [0, 0, 0, 0, 0, 1], 0.1))])
"""


@pytest.fixture(scope="module")
def score_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_plane"), _SCORE)[0]


def _check(out, name, case, flags=True):
    cloud, tri, _, (planes, counts, best) = case
    H = tri.shape[0]
    got_p, got_c, got_b = out[name + "_planes"], out[name + "_counts"], out[name + "_best"]
    assert got_p.dtype == np.float32 and got_p.shape == (H, 6) and got_c.dtype == np.int32 and got_c.shape == (H,) and got_b.dtype == np.int32 and got_b.shape == (1,), name
    assert np.array_equal(got_c, counts), name
    assert int(got_b[0]) == best and (best == -1 or got_c[best] >= 0), name       # -1 is never chosen over a count
    assert np.array_equal(got_p, planes, equal_nan=True), name
    assert not flags or (bool(out[name + "_twice"]) and bool(out[name + "_default"])), name   # the same bits on a second run; the default call


@pytest.mark.parametrize("N", PR.SCORE_N)
def test_counts_best_and_planes_equal_the_restatement(score_out, N):
    assert PR.SCORE_N == (3, 63, 64, 65, 255, 256, 257, 1025, 2500) and PR.SCORE_H == (1, 63, 64, 65, 300)
    for ld in (3, 6):
        for H in PR.SCORE_H:
            case = PR.uniform_case(N, ld, H)
            assert case[0].shape == (N, ld) and case[1].shape == (H, 3)
            if H >= 63:
                assert (case[3][1][[5, 7, 9]] == -1).all()          # the degenerate hypotheses that were mixed in
            _check(score_out, f"n{N}_ld{ld}_h{H}", case)


@pytest.mark.parametrize("name", ["lattice", "twin", "degenerate", "nonfinite"])
def test_exact_ties_twins_and_degenerate_hypotheses(score_out, name):
    case = named_cases()[name]
    _check(score_out, name, case)
    counts, best = score_out[name + "_counts"], int(score_out[name + "_best"][0])
    if name == "lattice":
        assert np.array_equal(counts, PR.lattice_case()[4]) and best == 1          # rows exactly on the threshold are inliers
    if name == "twin":
        assert best == 3 and counts[3] == counts[10] == counts.max()               # of two identical hypotheses at the top the lower index
    if name == "degenerate":
        assert (counts == -1).all() and best == -1
    if name == "nonfinite":
        assert counts[2:5].tolist() == [-1, -1, -1] and counts[best] > 0


def test_a_strided_view(score_out):
    _check(score_out, "view", PR.uniform_case(2500, 6, 300), flags=False)


def test_refusals(score_out):
    errors = score_out["errors"].tolist()
    assert len(errors) == 13 and all(errors), errors
    assert all("threshold" in e for e in errors[:4] + errors[9:11]) and "H" in errors[4] and "2^16" in errors[5] and "N = 2" in errors[6] and "N = 2" in errors[11]
    assert "CUDA tensor" in errors[7] and "device" in errors[8] and "CUDA tensor" in errors[12]


_APPLY = """
for N, ld, H in T.APPLY_CASES:
    cloud, tri, t, (planes, counts, best) = PR.uniform_case(N, ld, H)
    p = torch.from_numpy(cloud).cuda()
    for tag, plane in (("best", planes[best]), ("hand", np.array([0.1, -0.2, 0.05, 0.0, 0.0, 3.0], np.float32)), ("none", np.array([0, 0, 0, 0, 0, 0], np.float32))):
        name = f"n{N}_{tag}"
        got = pc_plane.apply_plane(p, plane, t, want=pc_plane.APPLY_WANT)
        again = pc_plane.apply_plane(p, torch.from_numpy(plane), t, want=pc_plane.APPLY_WANT)
        out[name + "_twice"] = np.array(all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(got.values(), again.values())))
        alone = [pc_plane.apply_plane(p, plane, t, want=w) for w in pc_plane.APPLY_WANT]
        out[name + "_alone"] = np.array(all(list(a) == [w] and a[w].cpu().numpy().tobytes() == got[w].cpu().numpy().tobytes() for a, w in zip(alone, pc_plane.APPLY_WANT)))
        out[name + "_default"] = np.array(list(pc_plane.apply_plane(p, plane, t)) == ["mask"])
        for w in got:
            out[name + "_" + w] = got[w].cpu().numpy()
"""


@pytest.fixture(scope="module")
def apply_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_plane_apply"), _APPLY)[0]


@pytest.mark.parametrize("case", APPLY_CASES)
def test_apply_plane_mask_count_and_moments(apply_out, case):
    N, ld, H = case
    cloud, tri, t, (planes, counts, best) = PR.uniform_case(N, ld, H)
    for tag, plane in (("best", planes[best]), ("hand", np.array([0.1, -0.2, 0.05, 0.0, 0.0, 3.0], np.float32)), ("none", np.zeros(6, np.float32))):
        name = f"n{N}_{tag}"
        mask, count, moments = apply_out[name + "_mask"], apply_out[name + "_count"], apply_out[name + "_moments"]
        want = PR.inliers_ref(cloud, plane, t)
        assert mask.dtype == np.uint8 and mask.shape == (N,) and np.array_equal(mask.astype(bool), want) and mask.max() <= 1, name
        assert count.dtype == np.int32 and count.tolist() == [int(mask.sum())], name
        if tag == "best":
            assert int(count[0]) == counts[best]                     # one rule for both entry points
        if tag == "none":
            assert int(count[0]) == 0 and (moments == 0).all()       # a degenerate plane has no inliers
        ref, _ = PR.moments_ref(cloud, want, plane[:3])
        bound = PR.moments_bound(cloud, want, plane[:3])
        err = np.abs(moments - ref)
        print(f"{name}: {int(count[0])} inliers, moment errors / bound {np.array2string(err / np.maximum(bound, 1e-300), precision=3)}")
        assert moments.dtype == np.float64 and moments.shape == (10,) and moments[0] == want.sum() and (err <= bound).all(), (name, err, bound)
        assert bool(apply_out[name + "_twice"]) and bool(apply_out[name + "_alone"]) and bool(apply_out[name + "_default"]), name


# ---- the input side --------------------------------------------------------------------------------------------------------------------
_E2E = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
xyz, normals, kind = PR.scene(0)
file = np.concatenate([xyz, normals.astype(np.float32)], 1)
kept = PR.scene_reference()[0]
path, alone = os.path.join(tmp, "scene.npy"), os.path.join(tmp, "alone.npy")
np.save(path, file)
np.save(alone, file[kept])
def state():
    s = np.random.get_state()
    return np.concatenate([s[1], [s[2]]])
out["rows"] = pc_plane.remove_planes(xyz, PR.SCENE_T, 1024, 1, 0.2, 4096, "direct")
for kind_ in ("pc_xyz", "pc_normal"):
    np.random.seed(3)
    ds = Dataset(kind_, [path], plane_threshold=PR.SCENE_T)
    out[kind_ + "_n"], out[kind_ + "_keys"], out[kind_ + "_raw"], out[kind_ + "_item"] = np.array(len(ds)), np.array(sorted(ds[0])), ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    np.random.seed(3)
    ds = Dataset(kind_, [alone])
    out[kind_ + "_alone_raw"], out[kind_ + "_alone_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    np.random.seed(3)
    out[kind_ + "_cluster_raw"] = Dataset(kind_, [path], cluster_radius=0.06).data[0]["pc_normal"]
    np.random.seed(3)
    out[kind_ + "_both_raw"] = Dataset(kind_, [path], plane_threshold=PR.SCENE_T, cluster_radius=0.06).data[0]["pc_normal"]
    np.random.seed(3)
    out[kind_ + "_half_raw"] = Dataset(kind_, [path], plane_threshold=PR.SCENE_T, plane_min_fraction=0.5).data[0]["pc_normal"]
    np.random.seed(9)
    ds = Dataset(kind_, [path], plane_threshold=0.0, plane_iters=5, plane_count=2, plane_min_fraction=0.9)
    out[kind_ + "_off_item"], out[kind_ + "_off_state"] = ds[0]["pc_normal"], state()
    np.random.seed(9)
    ds = Dataset(kind_, [path])
    out[kind_ + "_plain_item"], out[kind_ + "_plain_state"], out[kind_ + "_plain_raw"] = ds[0]["pc_normal"], state(), ds.data[0]["pc_normal"]
np.random.seed(3)
out["plain3_raw"] = Dataset("pc_normal", [path]).data[0]["pc_normal"]
try:
    Dataset("pc_normal", [path], plane_threshold=PR.SCENE_T, n_points=9000)
    out["too_few"] = np.array("")
except ValueError as e:
    out["too_few"] = np.array(str(e))
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_plane_e2e"), _E2E)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rows_of(raw, xyz):
    """the rows of xyz that the item's points are, by their bytes"""
    where = {r.tobytes(): i for i, r in enumerate(xyz)}
    return np.array([where[r.tobytes()] for r in np.ascontiguousarray(raw[:, :3], np.float32)])


def test_the_scene_decides_every_row_with_room_to_spare():
    """On the CPU, from the restatement: no row of the scene lies within 0.2 t of the decision boundary of the first or the refitted
    plane, so no last-bit difference in the moments can move a row and the kept rows must be exactly the restatement's."""
    kept, found, stopped = PR.scene_reference()
    assert not stopped and len(found) == 1 and found[0]["gap"] >= 0.2 * PR.SCENE_T
    assert found[0]["count"] >= 0.2 * PR.scene(0)[0].shape[0]


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_dataset_keeps_exactly_the_restatements_rows(e2e, kind):
    out, stdout = e2e
    xyz, _, what = PR.scene(0)
    kept, found, _ = PR.scene_reference()
    assert np.array_equal(out["rows"], kept) and out["rows"].dtype == np.int64
    assert int(out[kind + "_n"]) == 1 and out[kind + "_keys"].tolist() == ["pc_normal", "uid"] and out[kind + "_raw"].shape == (N_POINTS, 6)
    assert _same(out[kind + "_raw"], out[kind + "_alone_raw"])       # bit for bit the Dataset of the restatement's rows alone, same seed
    assert _same(out[kind + "_item"], out[kind + "_alone_item"]) and out[kind + "_item"].dtype == np.float16
    assert (what[_rows_of(out[kind + "_raw"], xyz)] == 1).all()      # the sphere alone
    n = found[0]["plane"][3:].astype(np.float64)
    n /= np.linalg.norm(n) * (1 if n[np.argmax(np.abs(n))] > 0 else -1)
    line = (f"scene: plane removal (threshold 0.02) removed 1 plane: {found[0]['count']} inliers, normal ({n[0]:+.4f} {n[1]:+.4f} {n[2]:+.4f}), "
            f"dropped {xyz.shape[0] - kept.shape[0]} of {xyz.shape[0]} points")
    assert stdout.count(line) == 5, stdout                          # both types: alone and with clustering; the refused one too
    # the table's normal: a plane that holds rows near opposite corners of the table, 2 sqrt(2) apart and within 0.2 t of the true plane,
    # within t of itself tilts against it by at most 2 * 1.2 t / (2 sqrt(2)) = 0.017 rad
    assert abs(abs(n[2]) - np.cos(PR.SCENE_TILT)) < 0.02 and abs(abs(n[1]) - np.sin(PR.SCENE_TILT)) < 0.02
    msg = str(out["too_few"])
    assert "scene" in msg and str(kept.shape[0]) in msg and "9000" in msg


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_clustering_needs_the_plane_gone(e2e, kind):
    out, stdout = e2e
    xyz, _, what = PR.scene(0)
    alone = what[_rows_of(out[kind + "_cluster_raw"], xyz)]
    assert (alone == 0).sum() > 1000 and (alone == 1).sum() > 1000    # cluster_radius alone: the table and the sphere are one part
    assert (what[_rows_of(out[kind + "_both_raw"], xyz)] == 1).all()  # with both options the item is the sphere alone
    kept = PR.scene_reference()[0]
    assert stdout.count(f"scene: clustering (radius 0.06) found 1 components, kept 1 (sizes {kept.shape[0]}), dropped 0 of {kept.shape[0]} points") == 2
    assert _same(out[kind + "_both_raw"], out[kind + "_raw"])         # one component: the same rows stand in, the same draw


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_threshold_zero_is_todays_and_a_high_floor_removes_nothing(e2e, kind):
    out, stdout = e2e
    assert _same(out[kind + "_off_item"], out[kind + "_plain_item"]) and np.array_equal(out[kind + "_off_state"], out[kind + "_plain_state"])
    M = PR.scene(0)[0].shape[0]
    assert stdout.count(f"scene: plane removal (threshold 0.02) removed 0 planes: no plane of at least 0.5 of the rows found, dropped 0 of {M} points") == 2
    if kind == "pc_normal":
        assert _same(out["pc_normal_half_raw"], out["plain3_raw"])    # nothing removed: the item of the whole file under the same seed


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_removes_the_table_and_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_normal --plane_threshold 0.02 --synthetic_weights --n_max_triangles 8` on the scene, end to end
    (350M shape, seeded synthetic checkpoint, 8-face cap): the plane line and one OBJ file."""
    xyz, normals, _ = PR.scene(0)
    kept, found, _ = PR.scene_reference()
    np.save(tmp_path / "scene.npy", np.concatenate([xyz, normals.astype(np.float32)], 1))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(tmp_path / "scene.npy"), "--input_type", "pc_normal", "--out_dir", str(out),
                        "--plane_threshold", "0.02", "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [f for _, _, fs in os.walk(out) for f in fs if f.endswith(".obj")]
    assert objs == ["scene_gen.obj"]
    assert f"scene: plane removal (threshold 0.02) removed 1 plane: {found[0]['count']} inliers, normal (" in r.stdout
    assert f"dropped {xyz.shape[0] - kept.shape[0]} of {xyz.shape[0]} points" in r.stdout and "dataset total data samples: 1" in r.stdout
