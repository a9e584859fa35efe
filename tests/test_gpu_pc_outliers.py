"""Statistical outlier removal on the MI355X: the cell-grid neighbour search (csrc/pc_grid.hpp, meshanything_amd/pc_outliers.py) against the
brute-force restatement `pc_normals_ref.knn_ref`, the filter against `pc_outliers_ref.sor_ref`, through `Dataset(..., outlier_k=16)` and
through `main.py --outlier_k 16`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

The key is float32 arithmetic without contraction and the order (distance, index) is total, so the k best are unique: indices and
distance bits must EQUAL the brute force's on every grid, and, the order of the points inside a cell coming from atomics, on a second
run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_fps_ref as F
import pc_normals_ref as PN
import pc_outliers_ref as R

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
NOISY = ("sphere", 12000, 120, 3)
BIG = ("sphere", 16384 - 160, 160, 5)

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_normals_ref as PN
import pc_outliers_ref as R
from meshanything_amd import pc_normals, pc_outliers
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


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def named_cases():
    """name -> (cloud, k, {grid name: grid or None for the automatic one})"""
    lat = PN.lattice(10)
    on_faces = {"cell8": ((0.0, 0.0, 0.0), 1 / 8, (10, 10, 10)), "cell16": ((0.0, 0.0, 0.0), 1 / 16, (20, 20, 20))}
    some = {"auto": None, "8x8x8": ((-1.0, -1.0, -1.0), 0.25, (8, 8, 8))}
    return {"lattice_k8": (lat, 8, on_faces), "lattice_k32": (lat, 32, on_faces), "tripled_k8": (PN.tripled(400, seed=4), 8, some),
            "tripled_k32": (PN.tripled(400, seed=4), 32, some), "repeated_k32": (R.repeated_point(), 32, some),
            "noisy_sphere_k16": (R.noisy(*BIG)[0], 16, {"auto": None})}


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
_KNN = """
sys.path.insert(0, {tests!r})
import test_gpu_pc_outliers as T
def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t
def same(a, b):
    return all(bool(torch.equal(bits(a[w]), bits(b[w]))) for w in a)
def run(name, cloud, k, grids):
    p = torch.from_numpy(cloud).cuda()
    first, agree, twice, alone = None, [], [], []
    for grid in grids:
        got = pc_outliers.grid_knn(p, k, grid, want=("idx", "d2", "mean"))
        twice.append(same(got, pc_outliers.grid_knn(p, k, grid, want=("idx", "d2", "mean"))))
        alone.append(bool(torch.equal(bits(got["mean"]), bits(pc_outliers.grid_knn(p, k, grid, want="mean")["mean"]))))
        if first is None:
            first = got
        agree.append(same(first, got))
    for w in first:
        out[name + "_" + w] = first[w].cpu().numpy()
    out[name + "_grids_agree"], out[name + "_twice"], out[name + "_mean_alone"] = np.array(agree), np.array(twice), np.array(alone)
for k in R.GRID_SIZES_K:
    for N in R.grid_sizes(k):
        for ld in (3, 6):
            name = f"k{{k}}_n{{N}}_ld{{ld}}"
            cloud = PN.knn_cases()[name + "_all"][0]
            run(name, cloud, k, [None] + list(R.uniform_grid_cases(cloud).values()))
for name, (cloud, k, grids) in T.named_cases().items():
    run(name, cloud, k, list(grids.values()))
# the lists alone, the brute force of the library on the same cloud, and a strided view
cloud = PN.knn_cases()["k16_n2500_ld6_all"][0]
p = torch.from_numpy(cloud).cuda()
lists = pc_outliers.grid_knn(p, 16)
brute = pc_normals.knn(p, None, 16)
out["lists_only_keys"] = np.array(sorted(lists))
out["equals_library_brute_force"] = np.array(bool(torch.equal(lists["idx"], brute[0])) and bool(torch.equal(bits(lists["d2"]), bits(brute[1]))))
wide = torch.cat([p, p], 1)
out["view_idx"] = pc_outliers.grid_knn(wide[:, 6:], 16, want="idx")["idx"].cpu().numpy()
""".format(tests=TESTS)


@pytest.fixture(scope="module")
def knn_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_grid"), _KNN)[0]


def _check(knn_out, name, cloud, k, n_grids):
    want_idx, want_d2 = PN.knn_ref(cloud, None, k)
    idx, d2, mean = knn_out[name + "_idx"], knn_out[name + "_d2"], knn_out[name + "_mean"]
    N = cloud.shape[0]
    assert idx.dtype == np.int32 and idx.shape == (N, k) and d2.dtype == np.float32 and d2.shape == (N, k) and mean.dtype == np.float64 and mean.shape == (N,), name
    assert np.array_equal(idx, want_idx), name
    assert _same(d2, want_d2), name
    for flag in ("_grids_agree", "_twice", "_mean_alone"):          # every grid the same bits, every case twice, mean_dist alone
        assert knn_out[name + flag].shape == (n_grids,) and knn_out[name + flag].all(), name + flag
    want_mean = R.mean_dist_ref(want_d2)
    some = want_mean > 0                                            # k coincident points: every term is 0 and so is the mean, exactly
    assert (mean[~some] == 0).all(), name
    err = float((np.abs(mean - want_mean)[some] / want_mean[some]).max())
    assert err <= 1e-14, (name, err)                                # <= 32 additions, a division, square roots of one ulp: about 35 * 2^-52 = 7.8e-15
    return err


@pytest.mark.parametrize("k", R.GRID_SIZES_K)
def test_lists_equal_the_brute_force_on_every_grid(knn_out, k):
    assert R.grid_sizes(k) == (k, k + 1, 255, 257, 1025, 2500)
    worst = 0.0
    for N in R.grid_sizes(k):
        for ld in (3, 6):
            cloud = PN.knn_cases()[f"k{k}_n{N}_ld{ld}_all"][0]
            assert cloud.shape == (N, ld)
            worst = max(worst, _check(knn_out, f"k{k}_n{N}_ld{ld}", cloud, k, 1 + len(R.uniform_grid_cases(cloud))))
    print(f"k = {k}: mean_dist within {worst:.3g} relative of the float64 restatement")


@pytest.mark.parametrize("name", list(named_cases()))
def test_faces_duplicates_and_strays(knn_out, name):
    cloud, k, grids = named_cases()[name]
    _check(knn_out, name, cloud, k, len(grids))
    if name == "repeated_k32":
        copies = np.flatnonzero(knn_out[name + "_d2"][:, 31] == 0)
        assert copies.shape[0] == 40 and np.array_equal(knn_out[name + "_idx"][copies[-1]], copies[:32].astype(np.int32))
    if name == "noisy_sphere_k16":
        assert cloud.shape[0] == 16384                               # 64 workgroups of queries, the automatic grid fitted to the sphere


def test_lists_alone_a_view_and_the_library_brute_force(knn_out):
    assert knn_out["lists_only_keys"].tolist() == ["d2", "idx"]
    assert bool(knn_out["equals_library_brute_force"])
    assert np.array_equal(knn_out["view_idx"], knn_out["k16_n2500_ld6_idx"])


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
_SOR = f"""
for name in PN.CLOUDS:
    xyz = R.noisy(name, *{NOISY[1:]!r})[0]
    runs = [pc_outliers.remove_statistical_outliers(xyz, 16, 2.0, form=f) for f in (2, 1, 0)]
    out[name + "_keep"], out[name + "_m"], out[name + "_T"] = runs[0][0], runs[0][1], np.array(runs[0][2])
    out[name + "_forms_agree"] = np.array([np.array_equal(runs[0][0], r[0]) and runs[0][1].tobytes() == r[1].tobytes() and runs[0][2] == r[2] for r in runs[1:]])
"""


@pytest.fixture(scope="module")
def sor_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_sor"), _SOR)[0]


@pytest.mark.parametrize("name", list(PN.CLOUDS))
def test_filter_equals_the_restatement(sor_out, name):
    keep, m, T = R.sor_of_noisy(name, *NOISY[1:], 16, 2.0)
    got_keep, got_m, got_T = sor_out[name + "_keep"], sor_out[name + "_m"], float(sor_out[name + "_T"])
    assert got_keep.dtype == np.bool_ and got_keep.shape == keep.shape and got_m.dtype == np.float64
    assert np.array_equal(got_keep, keep)                            # every point compared: the nearest m lies 1e-3 of T from T (host test)
    assert np.abs(got_m - m).max() <= 1e-14 * m.max() and abs(got_T - T) <= 1e-13 * T
    assert sor_out[name + "_forms_agree"].shape == (2,) and sor_out[name + "_forms_agree"].all()   # brute force, grid, automatic: the same bits


# ---- the input side --------------------------------------------------------------------------------------------------------------------
_E2E = f"""
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
xyz, normals, stray = R.noisy(*{NOISY!r})
path = os.path.join(tmp, "scan.npy")
np.save(path, np.concatenate([xyz, normals.astype(np.float32)], 1))
clean = os.path.join(tmp, "clean.npy")
np.save(clean, np.concatenate([xyz[~stray], normals[~stray].astype(np.float32)], 1))
np.random.seed(3)
before = np.random.get_state()[1].copy()
for kind in ("pc_xyz", "pc_normal"):
    ds = Dataset(kind, [path], outlier_k=16, point_sampling="fps")
    out[kind + "_fps_raw"], out[kind + "_fps_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    out[kind + "_fps_unfiltered"] = Dataset(kind, [path], point_sampling="fps").data[0]["pc_normal"]
out["rng_untouched"] = np.array(np.array_equal(np.random.get_state()[1], before))
out["clean_item"] = Dataset("pc_xyz", [clean], point_sampling="fps")[0]["pc_normal"]
for kind in ("pc_xyz", "pc_normal"):
    np.random.seed(9)
    ds = Dataset(kind, [path], outlier_k=16, outlier_std=2.0)
    out[kind + "_random_raw"], out[kind + "_random_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
try:
    Dataset("pc_normal", [path], outlier_k=16, n_points=12100)
    out["too_few"] = np.array("")
except ValueError as e:
    out["too_few"] = np.array(str(e))
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc_outliers_e2e")
    return _gpu(d, _E2E)


def _rows_in(rows, cloud):
    have = {r.tobytes() for r in np.ascontiguousarray(cloud[:, :3], np.float32)}
    return np.array([r.tobytes() in have for r in np.ascontiguousarray(rows[:, :3], np.float32)])


def _half_extent(item, rows=None):
    """the least, over the axes, of how far the rows of a normalised item reach towards either side of the unit box"""
    xyz = item[:, :3].astype(np.float64)[slice(None) if rows is None else rows]
    return float(min(xyz.max(0).min(), -xyz.min(0).max()))


def _least_extent(T):
    """A stray the filter keeps has a mean neighbour distance <= T, itself counted at 0, so another point lies within 16 T / 15 of it:
    the strays next to the unit sphere widen its bounding box to 1 + 16 T / 15 at the most, and the sphere's own points then reach
    0.9995 / (1 + 16 T / 15) of the unit box (T = 0.212: 0.815), less float16 rounding.  Unfiltered, strays in [-2, 2]^3 leave them 0.5."""
    return 0.9995 / (1 + 16 * T / 15) - 2e-3


def test_dataset_filters_before_it_samples(e2e):
    from meshanything_amd import pc_normals
    out, stdout = e2e
    xyz, normals, stray = R.noisy(*NOISY)
    file = np.concatenate([xyz, normals.astype(np.float32)], 1)
    keep, _, T = R.sor_of_noisy(*NOISY, 16, 2.0)
    assert int((~keep).sum()) == 111 and stray[~keep].all()
    surv = file[keep]
    assert stdout.count(f"scan: outlier filter removed 111 of 12120 points (k = 16, threshold {T:.6g})") == 5   # four datasets and the refused one
    assert bool(out["rng_untouched"])                               # the filter and fps draw nothing
    idx = F.fps_ref(surv[:, :3], N_POINTS)[0]
    # pc_normal, fps: the picks among the survivors, rows of the file in pick order
    raw = out["pc_normal_fps_raw"]
    assert raw.dtype == np.float32 and _same(raw, surv[idx])
    assert not _rows_in(raw, xyz[~keep]).any()                       # none of the 111 removed strays
    # pc_xyz, fps: the same rows, normals from the survivors' neighbours, oriented as well as the host reference of the same pipeline
    got = out["pc_xyz_fps_raw"]
    assert got.dtype == np.float32 and got.shape == (N_POINTS, 6) and _same(got[:, :3], surv[idx, :3])
    assert np.abs(np.linalg.norm(got[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6
    on_surface = ~stray[keep][idx]
    nbr, _ = PN.knn_ref(surv[:, :3], idx, 16)
    n, _ = PN.normals_eigh(surv[:, :3], nbr)
    graph, _ = PN.knn_ref(surv[idx, :3], None, 16)
    true = normals[keep][idx]
    want = PN.signed_share(pc_normals.orient_normals(surv[idx, :3], n, graph)[on_surface], true[on_surface])
    share = PN.signed_share(got[on_surface, 3:], true[on_surface])
    print(f"noisy sphere, filtered, fps rows: correctly signed {share:.4f}, host reference {want:.4f}")
    assert want >= 0.99 and share >= want - 0.005
    # after normalize_pc the object fills the box as the clean sphere does; without the filter the strays set the scale
    assert _half_extent(out["clean_item"]) > 0.97 and _least_extent(T) > 0.8
    for kind in ("pc_xyz", "pc_normal"):
        item = out[kind + "_fps_item"]
        assert item.dtype == np.float16 and item.shape == (N_POINTS, 6)
        assert np.abs(item[:, :3].astype(np.float64)).max() <= 0.9995 + 1e-3
        reach = _half_extent(item, on_surface)
        print(f"{kind}, fps, filtered: the sphere's own rows reach {reach:.4f} of the unit box, the clean sphere {_half_extent(out['clean_item']):.4f}")
        assert reach >= _least_extent(T)
        unfiltered = out[kind + "_fps_unfiltered"]
        kept_strays = int(_rows_in(unfiltered, xyz[stray]).sum())
        print(f"{kind}, fps, no filter: {kept_strays} of 120 strays among the {N_POINTS} rows")
        assert kept_strays >= 100                                    # the behaviour being fixed: fps picks strays first


def test_dataset_uniform_draw_runs_over_the_survivors(e2e):
    out, _ = e2e
    xyz, normals, stray = R.noisy(*NOISY)
    file = np.concatenate([xyz, normals.astype(np.float32)], 1)
    keep, _, T = R.sor_of_noisy(*NOISY, 16, 2.0)
    surv = file[keep]
    np.random.seed(9)
    idx = np.random.choice(surv.shape[0], N_POINTS, replace=False)   # the draw of the pc_normal branch, over the survivors
    assert _same(out["pc_normal_random_raw"], surv[idx])
    assert _same(out["pc_xyz_random_raw"][:, :3], surv[idx, :3])
    for kind in ("pc_xyz", "pc_normal"):
        assert not _rows_in(out[kind + "_random_raw"], xyz[~keep]).any()
        assert _half_extent(out[kind + "_random_item"], ~stray[keep][idx]) >= _least_extent(T)
    msg = str(out["too_few"])
    assert "12009" in msg and "12100" in msg                         # fewer survivors than n_points: both counts


def test_cli_outlier_k_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_xyz --outlier_k 16 --input_path scan.npy --synthetic_weights --n_max_triangles 8` end to end (350M
    shape, seeded synthetic checkpoint, 8-face cap): the removal line and one OBJ."""
    src = tmp_path / "scan.npy"
    xyz, _, stray = R.noisy("sphere", 5000, 50, 8)
    np.save(src, xyz)
    keep, _, T = R.sor_ref(xyz, 16, 2.0)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_xyz", "--outlier_k", "16", "--out_dir",
                        str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "scan_gen.obj"
    assert f"scan: outlier filter removed {int((~keep).sum())} of 5050 points (k = 16, threshold {T:.6g})" in r.stdout
    assert int((~keep).sum()) >= 40 and stray[~keep].all()
    assert "dataset total data samples: 1" in r.stdout and "Generation Start!!!" in r.stdout and "Over!!" in r.stdout
