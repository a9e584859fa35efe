"""Farthest-point sampling on the MI355X (csrc/pc_fps.hpp, meshanything_amd/pc_fps.py) against the numpy restatement of
tests/pc_fps_ref.py, through `Dataset(..., point_sampling="fps")`, and through `main.py --point_sampling fps`.  Every GPU step runs in a
fresh interpreter under a time limit; the comparisons run here.

The distance key is float32 arithmetic without contraction and the order (greater distance, then lower index) is total, so indices and
distance bits must EQUAL the restatement's, in the one-workgroup form, in the many-workgroup form, in the automatic choice and on a
second run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_fps_ref as R
import pc_normals_ref as PN

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
E2E_N, E2E_SEED = 6000, 7

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_fps_ref as R
import pc_normals_ref as PN
from meshanything_amd import pc_fps
out = {{}}
"""


def _gpu(tmp_path, body, timeout=300):
    """Run `body` (after _PRELUDE) in a fresh interpreter; it fills the dict `out`, which comes back as a dict of arrays."""
    script = tmp_path / "job.py"
    res = tmp_path / "out.npz"
    script.write_text(_PRELUDE + body + f"\nnp.savez({str(res)!r}, **out)\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(res) as z:
        return {k: z[k] for k in z.files}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
_FPS = """
dev = {}
def same(a, b):
    return bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
for name, (cloud, n, start) in R.fps_cases().items():
    if id(cloud) not in dev:
        dev[id(cloud)] = torch.from_numpy(cloud).cuda()
    p, st, forms = dev[id(cloud)], (None if start < 0 else start), R.forms_for(cloud.shape[0])
    runs = [pc_fps.farthest_point_sample(p, n, st, f) for f in forms]
    out[name + "_idx"], out[name + "_d2"] = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    out[name + "_forms_agree"] = np.array([same(runs[0], r) for r in runs[1:]])
    out[name + "_repeat_agrees"] = np.array([same(r, pc_fps.farthest_point_sample(p, n, st, f)) for r, f in zip(runs, forms)])
# a strided view and a numpy integer are taken as they are
cloud, n, start = R.fps_cases()["n1025_ld6_k64_s-1"]
wide = torch.from_numpy(np.concatenate([cloud, cloud], 1)).cuda()
out["view_idx"] = pc_fps.farthest_point_sample(wide[:, 6:], np.int64(n))[0].cpu().numpy()
"""


@pytest.fixture(scope="module")
def fps_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_fps"), _FPS)


def _names(pred):
    return [n for n, c in R.fps_cases().items() if n.startswith("n") and pred(c[0].shape[0], c[0].shape[1], c[1], c[2])]


@pytest.mark.parametrize("n", R.FPS_PICKS)
def test_picks_equal_the_float32_restatement(fps_out, n):
    names = _names(lambda N, ld, k, s: k == n)
    sizes = {R.fps_cases()[x][0].shape[0] for x in names}
    assert {N for N in R.FPS_N if N >= n} | {n, n + 1} <= sizes and len(names) >= len(sizes) * 2 * 2
    for name in names:
        want_idx, want_d2 = R.reference(name)
        got_idx, got_d2 = fps_out[name + "_idx"], fps_out[name + "_d2"]
        assert got_idx.dtype == np.int32 and got_d2.dtype == np.float32 and got_idx.shape == (n,) and got_d2.shape == (n,), name
        assert np.array_equal(got_idx, want_idx), name
        assert _same(got_d2, want_d2), name
        assert np.isposinf(got_d2[0]) and (np.diff(got_d2[1:]) <= 0).all() and len(set(got_idx.tolist())) == n, name


def test_forms_agree_with_each_other_and_with_a_second_run(fps_out):
    names = list(R.fps_cases())
    one = [x for x in names if R.fps_cases()[x][0].shape[0] <= R.ONE_MAX]
    assert len(one) > 300 and len(names) - len(one) > 40
    for name in names:
        forms = R.forms_for(R.fps_cases()[name][0].shape[0])
        assert fps_out[name + "_forms_agree"].shape == (len(forms) - 1,) and fps_out[name + "_forms_agree"].all(), name
        assert fps_out[name + "_repeat_agrees"].shape == (len(forms),) and fps_out[name + "_repeat_agrees"].all(), name
    assert np.array_equal(fps_out["view_idx"], fps_out["n1025_ld6_k64_s-1_idx"])


@pytest.mark.parametrize("name", ["lattice", "lattice_from_0", "few_positions", "large"])
def test_ties_duplicates_and_many_workgroups(fps_out, name):
    cloud, n, start = R.fps_cases()[name]
    want_idx, want_d2 = R.reference(name)
    got_idx, got_d2 = fps_out[name + "_idx"], fps_out[name + "_d2"]
    assert np.array_equal(got_idx, want_idx) and _same(got_d2, want_d2)
    assert len(set(got_idx.tolist())) == n and np.isposinf(got_d2[0]) and (np.diff(got_d2[1:]) <= 0).all()
    if name == "lattice":
        assert sorted(got_idx.tolist()) == list(range(512)) and got_idx[0] == 0 and got_idx[1] == 511
    if name == "few_positions":
        assert (got_d2[1:7] > 0).all() and (got_d2[7:] == 0).all() and (np.diff(got_idx[7:]) > 0).all()
    if name == "large":
        assert cloud.shape[0] == 70000 and n == 512                 # 137 workgroups in the many-workgroup form, the last one partly filled


# ---- the input side ------------------------------------------------------------------------------------------------------------------
_E2E = f"""
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
p, true = PN.sphere({E2E_N}, seed={E2E_SEED})
path = os.path.join(tmp, "sphere.npy")
np.save(path, np.concatenate([p, true.astype(np.float32)], 1))
np.save(os.path.join(tmp, "sphere64.npy"), np.concatenate([p, true], 1).astype(np.float64))
np.random.seed(3)
before = np.random.get_state()[1].copy()
for kind in ("pc_normal", "pc_xyz"):
    ds = Dataset(kind, [path], point_sampling="fps")
    out[kind + "_raw"], out[kind + "_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
out["pc_normal_f64_raw"] = Dataset("pc_normal", [os.path.join(tmp, "sphere64.npy")], point_sampling="fps").data[0]["pc_normal"]
out["rng_untouched"] = np.array(np.array_equal(np.random.get_state()[1], before))
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc_fps_e2e")
    return d, _gpu(d, _E2E)


def test_dataset_keeps_the_rows_fps_picks_and_draws_nothing(e2e):
    from meshanything_amd import pc_normals
    tmp, out = e2e
    file = np.load(tmp / "sphere.npy")
    file64 = np.load(tmp / "sphere64.npy")
    p, true = PN.sphere(E2E_N, seed=E2E_SEED)
    idx = R.fps_ref(file[:, :3], N_POINTS)[0]
    assert len(set(idx.tolist())) == N_POINTS
    assert bool(out["rng_untouched"])
    # pc_normal: the rows of the file, in pick order, in the file's dtype
    raw = out["pc_normal_raw"]
    assert raw.dtype == np.float32 and _same(raw, file[idx])
    assert out["pc_normal_item"].dtype == np.float16 and out["pc_normal_item"].shape == (N_POINTS, 6)
    raw64 = out["pc_normal_f64_raw"]                                 # a float64 file: sampled on its float32 image, kept as float64
    assert raw64.dtype == np.float64 and _same(raw64, file64[R.fps_ref(file64[:, :3].astype(np.float32), N_POINTS)[0]])
    # pc_xyz: the same rows; normals from the whole cloud, oriented as well as the host reference of the same pipeline orients them
    got = out["pc_xyz_raw"]
    assert got.dtype == np.float32 and got.shape == (N_POINTS, 6) and _same(got[:, :3], file[idx, :3])
    assert np.abs(np.linalg.norm(got[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6
    nbr, _ = PN.knn_ref(file[:, :3], idx, 16)
    n, _ = PN.normals_eigh(file[:, :3], nbr)
    graph, _ = PN.knn_ref(file[idx, :3], None, 16)
    want = PN.signed_share(pc_normals.orient_normals(file[idx, :3], n, graph), true[idx])
    share = PN.signed_share(got[:, 3:], true[idx])
    print(f"sphere, fps rows: correctly signed {share:.4f}, host reference {want:.4f}")
    assert want >= 0.99
    assert share >= want - 0.005
    assert _same(out["pc_xyz_item"][:, :3], out["pc_normal_item"][:, :3])     # the same rows normalise to the same xyz


def test_cli_point_sampling_fps_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_normal --point_sampling fps --input_path sphere.npy --synthetic_weights --n_max_triangles 8` end to
    end (350M shape, seeded synthetic checkpoint, 8-face cap): one OBJ."""
    src = tmp_path / "sphere.npy"
    p, true = PN.sphere(5000, seed=8)
    np.save(src, np.concatenate([p, true.astype(np.float32)], 1))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_normal", "--point_sampling", "fps",
                        "--out_dir", str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "sphere_gen.obj"
    assert "dataset total data samples: 1" in r.stdout and "Generation Start!!!" in r.stdout and "Over!!" in r.stdout
