"""Raw point clouds as input on the MI355X: the neighbour search and the normal estimate (csrc/pc_normals.hpp) against the numpy
restatements of tests/pc_normals_ref.py, `xyz_to_pc_normal` and `Dataset("pc_xyz")` against clouds whose true normals are known, and
`main.py --input_type pc_xyz`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

Neighbours: the distance key is float32 arithmetic without contraction and the order (d, index) is total, so indices and distance bits
must EQUAL the float32 brute force, whatever the number of splits.

Normals: compared where the reference's gap ratio (l1 - l0) / l2 is at least 0.05 (at most 1 % of a cloud may fall below).  The measure
of what float64 resolves is the largest sine between the two float64 restatements (`normals_eigh`, `normals_in_kernel_order`: the
same sums in two orders) on the compared points; the kernel may deviate from `normals_eigh` by 8 times that, with a floor of 1e-12.
"""
# the figure as computed by the `normal_refs` fixture on the clouds below: 2.0e-15, so the floor of 1e-12 is the tolerance
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_normals_ref as R

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
NORMAL_CASES = (("sphere", 16), ("torus", 16), ("cube", 16), ("sphere", 8))
E2E_N, E2E_SEED = 6000, 5

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_normals_ref as R
from meshanything_amd import pc_normals
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


# ---- the neighbour search --------------------------------------------------------------------------------------------------------------
_KNN = """
dev = {}
def same(a, b):
    return bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
for name, (ref, qi, k) in R.knn_cases().items():
    if id(ref) not in dev:
        dev[id(ref)] = torch.from_numpy(ref).cuda()
    q = None if qi is None else torch.from_numpy(qi).cuda()
    runs = [pc_normals.knn(dev[id(ref)], q, k, s) for s in R.SPLITS]
    out[name + "_idx"], out[name + "_d2"] = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    out[name + "_splits_agree"] = np.array([same(runs[0], r) for r in runs[1:]])
    out[name + "_repeat_agrees"] = np.array(same(runs[-1], pc_normals.knn(dev[id(ref)], q, k, 0)))
# int64 indices are taken as they are; an index outside the cloud is refused
ref, qi, k = R.knn_cases()["k16_n1025_ld6_q65"]
out["int64_idx"] = pc_normals.knn(torch.from_numpy(ref).cuda(), torch.from_numpy(qi.astype(np.int64)), k)[0].cpu().numpy()
try:
    pc_normals.knn(torch.from_numpy(ref).cuda(), torch.tensor([0, 1025]), k)
    out["bad_index_refused"] = np.array(False)
except ValueError:
    out["bad_index_refused"] = np.array(True)
"""


@pytest.fixture(scope="module")
def knn_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_knn"), _KNN)


@pytest.fixture(scope="module")
def knn_refs():
    """id(ref array) -> the brute-force neighbours of EVERY point with k = 32, computed once per array; a case takes its rows and its k
    from it (the first k of the 32 nearest by (d, index) are the k nearest)."""
    full = {}

    def ref_for(ref, qi, k):
        if id(ref) not in full:
            full[id(ref)] = R.knn_ref(ref, None, min(32, ref.shape[0]))
        idx, d2 = full[id(ref)]
        rows = slice(None) if qi is None else qi
        return idx[rows, :k], d2[rows, :k]
    return ref_for


@pytest.mark.parametrize("k", R.KNN_K)
def test_neighbours_equal_the_float32_brute_force(knn_out, knn_refs, k):
    cases = {n: c for n, c in R.knn_cases().items() if c[2] == k and n.startswith("k")}
    assert len(cases) == 9 * 2 * 7
    for name, (ref, qi, _) in cases.items():
        want_idx, want_d2 = knn_refs(ref, qi, k)
        got_idx, got_d2 = knn_out[name + "_idx"], knn_out[name + "_d2"]
        assert got_idx.dtype == np.int32 and got_d2.dtype == np.float32, name
        assert np.array_equal(got_idx, want_idx), name
        assert _same(got_d2, want_d2), name
        assert (got_d2[:, 0] == 0).all() and (np.diff(got_d2, axis=1) >= 0).all(), name            # itself first, then ascending


@pytest.mark.parametrize("name", ["tripled_k8", "tripled_k32", "lattice_k8", "lattice_k32"])
def test_equal_distances_are_ordered_by_index(knn_out, knn_refs, name):
    ref, qi, k = R.knn_cases()[name]
    want_idx, want_d2 = knn_refs(ref, qi, k)
    got_idx, got_d2 = knn_out[name + "_idx"], knn_out[name + "_d2"]
    assert np.array_equal(got_idx, want_idx) and _same(got_d2, want_d2)
    ties = (np.diff(got_d2, axis=1) == 0)
    assert ties.mean() > 0.3 and (np.diff(got_idx, axis=1)[ties] > 0).all()
    if name.startswith("tripled"):                                   # a point and its two copies, by index, then the rest
        n = ref.shape[0] // 3
        assert np.array_equal(got_idx[:, :3], (np.arange(3 * n)[:, None] % n) + n * np.arange(3)[None, :]) and (got_d2[:, :3] == 0).all()


def test_result_does_not_depend_on_splits_or_on_the_run(knn_out):
    names = list(R.knn_cases())
    assert len(names) == 4 * 9 * 2 * 7 + 4
    for name in names:
        assert knn_out[name + "_splits_agree"].shape == (len(R.SPLITS) - 1,) and knn_out[name + "_splits_agree"].all(), name
        assert bool(knn_out[name + "_repeat_agrees"]), name
    assert np.array_equal(knn_out["int64_idx"], knn_out["k16_n1025_ld6_q65_idx"])
    assert bool(knn_out["bad_index_refused"])


# ---- the normal estimate ---------------------------------------------------------------------------------------------------------------
_NORMALS = f"""
for name, k in {NORMAL_CASES!r}:
    p = torch.from_numpy(R.CLOUDS[name]({N_POINTS}, seed=1)[0]).cuda()
    nbr, d2 = pc_normals.knn(p, None, k)
    n, w = pc_normals.estimate_normals(p, nbr)
    n2, w2 = pc_normals.estimate_normals(p, nbr)
    tag = f"{{name}}_k{{k}}"
    out[tag + "_nbr"], out[tag + "_n"], out[tag + "_w"] = nbr.cpu().numpy(), n.cpu().numpy(), w.cpu().numpy()
    out[tag + "_again"] = np.array(bool(torch.equal(n.view(torch.int64), n2.view(torch.int64))) and bool(torch.equal(w.view(torch.int64), w2.view(torch.int64))))
# 40 copies of one point inside a cloud: their neighbourhoods coincide; and a (N, 6) cloud gives what its xyz columns give
p, _ = R.sphere(300, seed=6)
p[:40] = p[0]
for k in (3, 16):
    dp = torch.from_numpy(p).cuda()
    nbr, d2 = pc_normals.knn(dp, None, k)
    n, w = pc_normals.estimate_normals(dp, nbr)
    wide = torch.cat([dp, torch.full_like(dp, float("nan"))], 1)
    n6, w6 = pc_normals.estimate_normals(wide, pc_normals.knn(wide, None, k)[0])
    out[f"coincident_k{{k}}_n"], out[f"coincident_k{{k}}_w"], out[f"coincident_k{{k}}_d2"] = n.cpu().numpy(), w.cpu().numpy(), d2.cpu().numpy()
    out[f"coincident_k{{k}}_wide"] = np.array(bool(torch.equal(n, n6)) and bool(torch.equal(w, w6)))
# a line: some unit perpendicular
t = np.linspace(-1, 1, 200)[:, None] * np.array([[1.0, 2.0, -0.5]]) + 0.25
line = torch.from_numpy(t.astype(np.float32)).cuda()
n, w = pc_normals.estimate_normals(line, pc_normals.knn(line, None, 8)[0])
out["line_n"], out["line_w"], out["line_p"] = n.cpu().numpy(), w.cpu().numpy(), line.cpu().numpy()
"""


@pytest.fixture(scope="module")
def normals_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_normals"), _NORMALS)


@pytest.fixture(scope="module")
def normal_refs():
    """(name, k) -> (cloud, reference neighbours, normals_eigh, compared points); and the tolerance derived from the two restatements"""
    ref, figure = {}, 0.0
    for name, k in NORMAL_CASES:
        p, _ = R.CLOUDS[name](N_POINTS, seed=1)
        nbr, _ = R.knn_ref(p, None, k)
        n, w = R.normals_eigh(p, nbr)
        n2, _ = R.normals_in_kernel_order(p, nbr)
        use = R.gap_ratio(w) >= 0.05
        print(f"{name} k={k}: {100 * (1 - use.mean()):.2f} % below the gap ratio")
        assert 1 - use.mean() <= 0.01
        figure = max(figure, float(R.sine(n, n2)[use].max()))
        ref[(name, k)] = (p, nbr, n, w, use)
    tol = max(8 * figure, 1e-12)
    print(f"largest sine between the two float64 restatements: {figure:.3g}; tolerance {tol:.3g}")
    assert figure < 1e-13
    return ref, tol


@pytest.mark.parametrize("name,k", NORMAL_CASES)
def test_normals_match_the_eigh_reference(normals_out, normal_refs, name, k):
    ref, tol = normal_refs
    p, nbr, want_n, want_w, use = ref[(name, k)]
    tag = f"{name}_k{k}"
    got_n, got_w = normals_out[tag + "_n"], normals_out[tag + "_w"]
    assert np.array_equal(normals_out[tag + "_nbr"], nbr)
    assert got_n.dtype == np.float64 and got_n.shape == (N_POINTS, 3) and got_w.dtype == np.float64 and got_w.shape == (N_POINTS, 3)
    # on all points
    assert np.isfinite(got_n).all() and np.isfinite(got_w).all()
    assert np.abs(np.linalg.norm(got_n, axis=1) - 1).max() <= 1e-12
    assert (np.diff(got_w, axis=1) >= 0).all()
    eig_err = float((np.abs(got_w - want_w).max(1) / want_w[:, 2]).max())
    # on the compared points
    sine = float(R.sine(got_n, want_n)[use].max())
    print(f"{tag}: largest sine to the reference {sine:.3g}, eigenvalues relative to l2 {eig_err:.3g}, tolerance {tol:.3g}")
    assert eig_err <= tol
    assert sine <= tol
    a = np.sort(np.abs(got_n), axis=1)
    clear = a[:, 2] - a[:, 1] > tol
    lead = np.take_along_axis(got_n, np.argmax(np.abs(got_n), axis=1)[:, None], 1)[:, 0]
    assert clear.mean() > 0.99
    assert (np.einsum("ij,ij->i", got_n, want_n)[use & clear] > 0).all()                       # the same sign as the reference's rule gives
    assert (lead > 0).all()                                         # exact ties included: argmax takes the lowest axis, as the kernel does
    assert bool(normals_out[tag + "_again"])


def test_degenerate_neighbourhoods(normals_out):
    for k in (3, 16):
        n, w, d2 = (normals_out[f"coincident_k{k}_{x}"] for x in ("n", "w", "d2"))
        same = (d2 == 0).all(1)
        assert same[:40].all() and not same[40:].any()
        assert np.array_equal(n[:40], np.tile([0.0, 0.0, 1.0], (40, 1))) and (w[:40] == 0).all()
        assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12
        assert bool(normals_out[f"coincident_k{k}_wide"])
    n, w = normals_out["line_n"], normals_out["line_w"]
    direction = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12
    assert np.abs(n @ direction).max() < 1e-6                       # float32 points on a line are collinear to about 1e-7
    assert (w[:, 1] <= 1e-9 * w[:, 2]).all() and (w[:, 2] > 0).all()     # float32 rounding off the line, squared


# ---- the whole input side --------------------------------------------------------------------------------------------------------------
def _e2e_cloud(name):
    p, true = R.CLOUDS[name](E2E_N, seed=7)
    return p, true


_E2E = f"""
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
for name in R.CLOUDS:
    p, true = R.CLOUDS[name]({E2E_N}, seed=7)
    np.random.seed({E2E_SEED})
    out[name + "_direct"] = pc_normals.xyz_to_pc_normal(p)
    path = os.path.join(tmp, name + ".npy")
    np.save(path, np.concatenate([p, true.astype(np.float32)], 1))   # an (N, 6) file: pc_xyz reads its first three columns only
    np.random.seed({E2E_SEED})
    ds = Dataset("pc_xyz", [path])
    out[name + "_raw"], out[name + "_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    if name == "sphere":
        np.savetxt(os.path.join(tmp, "scan.xyz"), p.astype(np.float64))
        np.random.seed({E2E_SEED})
        out["sphere_from_text"] = Dataset("pc_xyz", [os.path.join(tmp, "scan.xyz")]).data[0]["pc_normal"]
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc_xyz_e2e")
    return d, _gpu(d, _E2E)


@pytest.mark.parametrize("name", list(R.CLOUDS))
def test_xyz_to_pc_normal_orients_like_the_host_reference(e2e, name):
    from meshanything_amd import pc_normals
    from meshanything_amd.data import Dataset
    tmp, out = e2e
    p, true = _e2e_cloud(name)
    got = out[name + "_direct"]
    np.random.seed(E2E_SEED)
    idx = np.random.choice(E2E_N, N_POINTS, replace=False)
    assert got.dtype == np.float32 and got.shape == (N_POINTS, 6)
    assert _same(got[:, :3], p[idx])                                # the rows the pc_normal branch draws under the same seed
    assert np.abs(np.linalg.norm(got[:, 3:].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert _same(out[name + "_raw"], got)                           # Dataset("pc_xyz") is that call
    # the host reference of the same pipeline: neighbours in the whole cloud, eigh normals, the graph of the chosen points, the propagation
    nbr, _ = R.knn_ref(p, idx, 16)
    n, _ = R.normals_eigh(p, nbr)
    graph, _ = R.knn_ref(p[idx], None, 16)
    want = R.signed_share(pc_normals.orient_normals(p[idx], n, graph), true[idx])
    share = R.signed_share(got[:, 3:], true[idx])
    print(f"{name}: correctly signed {share:.4f}, host reference {want:.4f}")
    assert want >= 0.99
    assert share >= want - 0.005
    # against the pc_normal branch on the same file under the same seed: the same rows, the same normalised xyz, bit for bit
    np.random.seed(E2E_SEED)
    ds = Dataset("pc_normal", [str(tmp / (name + ".npy"))])
    assert _same(ds.data[0]["pc_normal"][:, :3], got[:, :3])
    item = out[name + "_item"]
    assert item.dtype == np.float16 and item.shape == (N_POINTS, 6)
    assert _same(item[:, :3], ds[0]["pc_normal"][:, :3])
    if name == "sphere":                                            # a text file of the same points: float64 rows, the same normals
        text = out["sphere_from_text"]
        assert text.dtype == np.float64 and _same(text[:, :3], p[idx].astype(np.float64))
        assert np.abs(text[:, 3:] - got[:, 3:]).max() < 1e-6


def test_cli_pc_xyz_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_xyz --input_path sphere.npy --synthetic_weights --n_max_triangles 8` end to end (350M shape,
    seeded synthetic checkpoint, 8-face cap): one OBJ."""
    src = tmp_path / "sphere.npy"
    np.save(src, R.sphere(5000, seed=8)[0])
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_xyz", "--out_dir", str(out),
                        "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "sphere_gen.obj"
    assert "dataset total data samples: 1" in r.stdout and "Generation Start!!!" in r.stdout and "Over!!" in r.stdout
