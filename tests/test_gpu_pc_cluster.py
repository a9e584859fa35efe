"""Euclidean clustering on the MI355X (csrc/pc_cluster.hpp, meshanything_amd/pc_cluster.py): the labels against the brute-force restatement
`pc_cluster_ref.cluster_ref`, the pair bound against the restated walk, through `Dataset(..., cluster_radius=...)` and through `main.py
--cluster_radius ... --cluster_mode split`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

labels[i] is the smallest row of i's component: a function of the cloud and the radius alone, so the labels must EQUAL the
restatement's on every grid and, the union-find and the order inside a cell coming from atomics, on a second run.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pc_cluster_ref as CR
import pc_fps_ref as F

pytestmark = pytest.mark.gpu

REPO = CR.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
ON_FACES = {"cell8": ((0.0, 0.0, 0.0), 1 / 8, (10, 10, 10)), "cell16": ((0.0, 0.0, 0.0), 1 / 16, (20, 20, 20))}
SOME = {"auto": None, "8x8x8": ((-1.0, -1.0, -1.0), 0.25, (8, 8, 8))}
BOUND_CASE = (2500, 0.3)                                             # uniform cloud, radius: the pair-bound test

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_cluster_ref as CR
import pc_fps_ref as F
from meshanything_amd import pc_cluster
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


def tie_grids():
    """name -> {grid name: grid}: the lattice over the two grids of test_gpu_pc_outliers.named_cases whose faces its points lie on"""
    import test_gpu_pc_outliers as TO
    assert TO.named_cases()["lattice_k8"][2] == ON_FACES
    return {"lattice_at": ON_FACES, "lattice_below": ON_FACES, "tripled": SOME, "repeated": SOME, "scene": {"auto": None}}


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
_LABELS = """
sys.path.insert(0, {tests!r})
import test_gpu_pc_cluster as T
def same(a, b):
    return all(bool(torch.equal(a[w], b[w])) for w in a)
def run(name, cloud, radius, grids):
    p = torch.from_numpy(cloud).cuda()
    first, agree, twice, alone = None, [], [], []
    for grid in grids:
        got = pc_cluster.euclidean_clusters(p, radius, grid, want=("labels", "sizes"))
        twice.append(same(got, pc_cluster.euclidean_clusters(p, radius, grid, want=("labels", "sizes"))))
        alone.append(bool(torch.equal(got["labels"], pc_cluster.euclidean_clusters(p, radius, grid)["labels"])))
        if first is None:
            first = got
        agree.append(same(first, got))
    for w in first:
        out[name + "_" + w] = first[w].cpu().numpy()
    out[name + "_grids_agree"], out[name + "_twice"], out[name + "_labels_alone"] = np.array(agree), np.array(twice), np.array(alone)
for name, (cloud, radius) in CR.uniform_cases().items():
    run(name, cloud, radius, list(CR.grids_for(radius).values()))
for name, grids in T.tie_grids().items():
    run(name, *CR.all_cases()[name], list(grids.values()))
# a strided view, and the keys of the default call
cloud, radius = CR.uniform_cases()["n2500_ld6_mix"]
p = torch.from_numpy(cloud).cuda()
wide = torch.cat([p, p], 1)
out["view_labels"] = pc_cluster.euclidean_clusters(wide[:, 6:], radius)["labels"].cpu().numpy()
out["default_keys"] = np.array(sorted(pc_cluster.euclidean_clusters(p, radius)))
# the pair bound
N, radius = T.BOUND_CASE
p = torch.from_numpy(F.uniform_cloud(N)).cuda()
try:
    pc_cluster.euclidean_clusters(p, radius, max_pairs=1000)
    out["capped"] = np.array("")
except ValueError as e:
    out["capped"] = np.array(str(e))
out["uncapped_labels"] = pc_cluster.euclidean_clusters(p, radius)["labels"].cpu().numpy()
""".format(tests=TESTS)


@pytest.fixture(scope="module")
def labels_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_cluster"), _LABELS)[0]


def _check(out, name, n_grids):
    cloud, _ = CR.all_cases()[name]
    want = CR.reference(name)
    labels, sizes = out[name + "_labels"], out[name + "_sizes"]
    N = cloud.shape[0]
    assert labels.dtype == np.int32 and labels.shape == (N,) and sizes.dtype == np.int32 and sizes.shape == (N,), name
    assert (labels <= np.arange(N)).all() and np.array_equal(labels[labels], labels), name
    assert np.array_equal(labels, want), name
    assert np.array_equal(sizes, CR.sizes_ref(want)), name
    for flag in ("_grids_agree", "_twice", "_labels_alone"):        # every grid the same labels, every case twice, labels without sizes
        assert out[name + flag].shape == (n_grids,) and out[name + flag].all(), name + flag


@pytest.mark.parametrize("N", CR.UNIFORM_N)
def test_labels_equal_the_restatement_on_every_grid(labels_out, N):
    assert CR.UNIFORM_N == (1, 2, 255, 256, 257, 1025, 2500)
    for ld in (3, 6):
        for kind in CR.KINDS:
            name = f"n{N}_ld{ld}_{kind}"
            cloud, radius = CR.uniform_cases()[name]
            assert cloud.shape == (N, ld)
            grids = CR.grids_for(radius)
            # two points lie up to 3.4 apart and the call takes radius / cell <= 8: a fixed grid too fine for that radius is refused (host test)
            assert len(grids) == 5 or N == 2
            assert {"auto", "1x1x1", "fine"} <= set(grids)
            _check(labels_out, name, len(grids))


@pytest.mark.parametrize("name", ["lattice_at", "lattice_below", "tripled", "repeated"])
def test_exact_ties(labels_out, name):
    _check(labels_out, name, len(tie_grids()[name]))
    labels = labels_out[name + "_labels"]
    if name == "lattice_at":
        assert (labels == 0).all()                                   # every edge has d == r2 exactly, the points lie on the cells' faces
    if name == "lattice_below":
        assert np.array_equal(labels, np.arange(1000))
    if name == "tripled":
        assert np.array_equal(labels, np.tile(np.arange(400), 3))    # r2 == 0: the copies alone, labelled by the first copy's row


def test_scene_labels_and_sizes(labels_out):
    _check(labels_out, "scene", 1)
    sizes = labels_out["scene_sizes"]
    assert sorted(sizes[sizes > 0].tolist(), reverse=True) == [9000, 6000, 150] + [1] * 40


def test_a_view_and_the_default_call(labels_out):
    assert labels_out["default_keys"].tolist() == ["labels"]
    assert np.array_equal(labels_out["view_labels"], labels_out["n2500_ld6_mix_labels"])


def test_pair_bound_refuses_before_the_search(labels_out):
    from meshanything_amd import pc_cluster
    N, radius = BOUND_CASE
    cloud = F.uniform_cloud(N)
    msg = str(labels_out["capped"])
    m = re.search(r"pair bound (\d+) exceeds max_pairs 1000\b", msg)
    assert m, msg
    bound = int(m.group(1))
    origin, cell, dims = pc_cluster.choose_cluster_grid(cloud, radius)             # the grid the call chose: a function of the array alone
    evaluated, _, complete = CR.walk_ref(cloud, radius, origin, cell, dims)
    print(f"uniform {N}, radius {radius}: pair bound {bound}, the walk evaluates {int(evaluated.sum())} keys, N^2 = {N * N}")
    assert complete and bound >= int(evaluated.sum())
    assert bound == CR.bound_ref(cloud, radius, origin, cell, dims) and bound <= N * N
    assert np.array_equal(labels_out["uncapped_labels"], CR.cluster_ref(cloud, radius))   # with the default cap the same call succeeds


# ---- the input side --------------------------------------------------------------------------------------------------------------------
_E2E = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
xyz, normals, kind = CR.scene(0)
file = np.concatenate([xyz, normals.astype(np.float32)], 1)
path, alone = os.path.join(tmp, "scene.npy"), os.path.join(tmp, "alone.npy")
np.save(path, file)
np.save(alone, file[kind == 0])
def state():
    s = np.random.get_state()
    return np.concatenate([s[1], [s[2]]])
for kind_ in ("pc_xyz", "pc_normal"):
    np.random.seed(3)
    ds = Dataset(kind_, [path], cluster_radius=CR.SCENE_RADIUS)
    out[kind_ + "_largest_n"], out[kind_ + "_largest_uid"], out[kind_ + "_largest_keys"] = np.array(len(ds)), np.array(ds[0]["uid"]), np.array(sorted(ds[0]))
    out[kind_ + "_largest_raw"], out[kind_ + "_largest_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    np.random.seed(3)
    ds = Dataset(kind_, [alone])
    out[kind_ + "_alone_raw"], out[kind_ + "_alone_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    np.random.seed(3)
    ds = Dataset(kind_, [path], cluster_radius=CR.SCENE_RADIUS, cluster_mode="split")
    out[kind_ + "_split_uids"], out[kind_ + "_split_groups"] = np.array([ds[i]["uid"] for i in range(len(ds))]), np.array(ds.groups())
    out[kind_ + "_split_keys"] = np.array(sorted(ds[1]))
    for j in range(len(ds)):
        item = ds[j]
        out[f"{{kind_}}_split{{j}}_raw"], out[f"{{kind_}}_split{{j}}_centre"], out[f"{{kind_}}_split{{j}}_scale"] = ds.data[j]["pc_normal"], item["frame"][0], np.array(item["frame"][1])
        out[f"{{kind_}}_split{{j}}_meta"] = np.array([item["group"], str(item["part"])])
    np.random.seed(9)
    ds = Dataset(kind_, [path], cluster_radius=0.0, cluster_mode="split", cluster_min_points=5000)
    out[kind_ + "_off_item"], out[kind_ + "_off_state"], out[kind_ + "_off_keys"] = ds[0]["pc_normal"], state(), np.array(sorted(ds[0]))
    np.random.seed(9)
    ds = Dataset(kind_, [path])
    out[kind_ + "_plain_item"], out[kind_ + "_plain_state"] = ds[0]["pc_normal"], state()
try:
    Dataset("pc_normal", [path], cluster_radius=CR.SCENE_RADIUS, cluster_min_points=9001)
    out["too_few"] = np.array("")
except ValueError as e:
    out["too_few"] = np.array(str(e))
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_cluster_e2e"), _E2E.format())


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_dataset_largest_is_the_large_sphere_alone(e2e, kind):
    out, stdout = e2e
    assert int(out[kind + "_largest_n"]) == 1 and str(out[kind + "_largest_uid"]) == "scene" and out[kind + "_largest_keys"].tolist() == ["pc_normal", "uid"]
    assert out[kind + "_largest_raw"].shape == (N_POINTS, 6)
    assert _same(out[kind + "_largest_raw"], out[kind + "_alone_raw"])           # bit for bit the Dataset of the 9 000 sphere rows, same seed
    assert _same(out[kind + "_largest_item"], out[kind + "_alone_item"]) and out[kind + "_largest_item"].dtype == np.float16
    assert stdout.count("scene: clustering (radius 0.06) found 43 components, kept 1 (sizes 9000), dropped 6190 of 15190 points") == 2   # both types; the refused one prints nothing
    assert stdout.count("scene: clustering (radius 0.06) found 43 components, kept 2 (sizes 9000 6000), dropped 190 of 15190 points") == 2
    msg = str(out["too_few"])
    assert "9001" in msg and "9000" in msg                               # no component of min_points rows: the largest size


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_dataset_split_makes_one_item_per_sphere(e2e, kind):
    out, _ = e2e
    xyz, _, what = CR.scene(0)
    assert out[kind + "_split_uids"].tolist() == ["scene_part0", "scene_part1"] and out[kind + "_split_groups"].tolist() == [0, 0]
    assert out[kind + "_split_keys"].tolist() == ["frame", "group", "part", "pc_normal", "uid"]
    for j, (centre, radius) in enumerate([((-0.7, 0.0, 0.0), 0.5), ((0.6, 0.0, 0.0), 0.3)]):
        raw = out[f"{kind}_split{j}_raw"]
        assert raw.shape == (N_POINTS, 6) and out[f"{kind}_split{j}_meta"].tolist() == ["scene", str(j)]
        have = {r.tobytes() for r in xyz[what == j]}
        assert all(r.tobytes() in have for r in np.ascontiguousarray(raw[:, :3], np.float32))   # rows of that sphere alone
        # 4096 of the sphere's points: the bounding box of the draw reaches within 2 % of the sphere's on every side
        assert np.abs(out[f"{kind}_split{j}_centre"] - centre).max() < 0.02 * radius and abs(float(out[f"{kind}_split{j}_scale"]) - radius / 0.9995) < 0.02 * radius
    assert _same(out[kind + "_split0_raw"], out[kind + "_largest_raw"])          # part 0 is what "largest" keeps, under the same seed


@pytest.mark.parametrize("kind", ["pc_xyz", "pc_normal"])
def test_dataset_with_radius_zero_is_todays(e2e, kind):
    out, _ = e2e
    assert _same(out[kind + "_off_item"], out[kind + "_plain_item"]) and np.array_equal(out[kind + "_off_state"], out[kind + "_plain_state"])
    assert out[kind + "_off_keys"].tolist() == ["pc_normal", "uid"]


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def _read_obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if t and t[0] == "v":
                v.append([float(x) for x in t[1:4]])
            elif t and t[0] == "f":
                f.append([int(x) for x in t[1:4]])
    return np.array(v, np.float64).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 3)


def _main(tmp_path, name, *flags):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(tmp_path / "scene.npy"), "--input_type", "pc_normal", "--out_dir",
                        str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0", *flags], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return {f: os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith(".obj")}, r.stdout


def test_cli_split_writes_the_parts_and_their_merge_in_the_input_frame(tmp_path):
    """`python main.py --input_type pc_normal --cluster_radius 0.06 --cluster_mode split --batchsize_per_gpu 2 --synthetic_weights
    --n_max_triangles 8` end to end (350M shape, seeded synthetic checkpoint, 8-face cap): three OBJ files, the parts in the input's
    frame; and the same command without the flags writes the one file it writes today."""
    from meshanything_amd.data import pc_frame
    xyz, normals, what = CR.scene(0)
    file = np.concatenate([xyz, normals.astype(np.float32)], 1)
    np.save(tmp_path / "scene.npy", file)
    objs, stdout = _main(tmp_path, "split", "--cluster_radius", "0.06", "--cluster_mode", "split", "--batchsize_per_gpu", "2")
    assert sorted(objs) == ["scene_gen.obj", "scene_part0_gen.obj", "scene_part1_gen.obj"]
    assert "scene: clustering (radius 0.06) found 43 components, kept 2 (sizes 9000 6000), dropped 190 of 15190 points" in stdout
    assert "dataset total data samples: 2" in stdout and stdout.count("Over!!") == 3
    parts = [_read_obj(objs[f"scene_part{j}_gen.obj"]) for j in range(2)]
    merged = _read_obj(objs["scene_gen.obj"])
    assert merged[0].shape[0] == sum(v.shape[0] for v, _ in parts) and merged[1].shape[0] == sum(f.shape[0] for _, f in parts)
    assert np.array_equal(merged[0], np.concatenate([v for v, _ in parts], 0))
    assert np.array_equal(merged[1], np.concatenate([parts[0][1], parts[1][1] + parts[0][0].shape[0]], 0))      # 1-based in the file, offset by part 0's vertices
    np.random.seed(0)                                                    # main.py seeds the draws of Dataset with --seed
    for j, (v, f) in enumerate(parts):
        rows = file[what == j]
        centre, scale = pc_frame(rows[np.random.choice(rows.shape[0], N_POINTS, replace=False)])   # the item's rows: the draw over that sphere's rows
        assert v.shape[0] >= 1 and f.shape[0] >= 1 and f.min() >= 1 and f.max() <= v.shape[0]
        # the decoder's coordinates are within +-0.5, times 2 is the unit box of the part's frame; 1e-8 of print rounding
        assert (np.abs(v - centre[None, :]) <= scale + 1e-8).all(), j
    plain, stdout = _main(tmp_path, "plain")
    assert sorted(plain) == ["scene_gen.obj"] and "clustering" not in stdout and "dataset total data samples: 1" in stdout
    v, f = _read_obj(plain["scene_gen.obj"])
    assert v.shape[0] >= 1 and np.abs(v).max() <= 0.5                    # the normalised frame, as today
