"""Upsampling of sparse input clouds on the MI355X (csrc/pc_upsample.hpp, meshanything_amd/pc_upsample.py): xyz, seed and counts against
the brute-force restatement `pc_upsample_ref.upsample_ref`, over the grids of every case; the sphere's geometry; non-finite input, the
capacity and the pair bound through the raw ABI; `upsample_rows`; through `Dataset(..., upsample_radius=...)` and through
`main.py --upsample_radius`; and, upsampling being the last of them, `Dataset` with every step of the input side on against the public
functions composed by hand.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

Every comparison of the op is EXACT, order included: the normals are an input, every candidate is one float64 expression rounded once,
and the keep test asks which row comes first in a total order, so nothing depends on the grid or on the order the walk visits the rows.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pc_upsample_ref as UR

pytestmark = pytest.mark.gpu

REPO = UR.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import ctypes as C
import numpy as np
import torch
import pc_upsample_ref as UR
import test_gpu_pc_upsample as T
from meshanything_amd import _lib, pc_cluster, pc_smooth, pc_upsample
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


def nonfinite_case():
    """the 300-row sphere with one NaN and one infinite row, one NaN and one infinite normal: through an explicit grid, which
    `upsample_points` does not check for finiteness"""
    p, n = (a.copy() for a in UR.sphere())
    p[5, 1] = np.nan
    p[77, 0] = np.inf
    n[10, 2] = np.nan
    n[11, 0] = -np.inf
    return p, n


NONFINITE_GRID = ((-1.1, -1.1, -1.1), 0.55, (4, 4, 4))
NONFINITE_ROWS = (5, 77, 10, 11)
RADIUS, M = 0.3, 2                                                   # of the raw-ABI cases; radius / 2 * 2 is exact, so fl32(m * step) = fl32(radius)
GUARD = 16

# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
_KERNEL = """
def keep(prefix, got):
    out[prefix + "xyz"], out[prefix + "seed"], out[prefix + "counts"] = got["xyz"].cpu().numpy(), got["seed"].cpu().numpy(), got["counts"].cpu().numpy()
    out[prefix + "total"] = np.array(got["total"])

for name, (cloud, normals, radius, m, active, grids) in UR.cases().items():
    p = torch.from_numpy(cloud).cuda()
    if cloud.shape[1] == 6:                                          # a strided view
        p = torch.cat([torch.full_like(p, 3.0), p], 1)[:, 6:]
        assert not p.is_contiguous()
    n = torch.from_numpy(normals).cuda()
    a = None if active is None else torch.from_numpy(active).cuda()
    for gname, grid in grids.items():
        keep(name + "__" + gname + "__", pc_upsample.upsample_points(p, n, radius, m, a, grid))
    got = pc_upsample.upsample_points(p, n, radius, m, a, count_only=True)
    assert got["xyz"] is None and got["seed"] is None
    out[name + "__count_only"], out[name + "__count_only_total"] = got["counts"].cpu().numpy(), np.array(got["total"])
# non-finite rows and normals through an explicit grid
cloud, normals = T.nonfinite_case()
p, n = torch.from_numpy(cloud).cuda(), torch.from_numpy(normals).cuda()
keep("nonfinite__", pc_upsample.upsample_points(p, n, T.RADIUS, T.M, None, T.NONFINITE_GRID))
# the capacity and the pair bound through the C ABI: nothing is written past a refusal
cloud, normals = UR.sphere()
N = cloud.shape[0]
p, n = torch.from_numpy(cloud).cuda(), torch.from_numpy(normals).cuda()
want = pc_upsample.upsample_points(p, n, T.RADIUS, T.M)
keep("abi_want__", want)
lib = _lib.load()
origin, cell, dims = pc_cluster.choose_cluster_grid(cloud, T.RADIUS)
nbytes = lib.ma_pc_upsample_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

def raw(capacity, max_pairs, rows):
    xyz = torch.full((rows + T.GUARD, 3), -7.0, dtype=torch.float32, device="cuda")
    seed = torch.full((rows + T.GUARD,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    total, bound = C.c_uint64(99), C.c_uint64(99)
    rc = lib.ma_op_pc_upsample(p.data_ptr(), N, 3, n.data_ptr(), None, T.M, T.RADIUS / T.M, (C.c_float * 3)(*origin.tolist()), float(cell),
                               (C.c_int32 * 3)(*dims.tolist()), max_pairs, counts.data_ptr(), xyz.data_ptr(), seed.data_ptr(), capacity, C.byref(total),
                               C.byref(bound), ws.data_ptr(), nbytes, stream)
    torch.cuda.synchronize()
    return rc, total.value, bound.value, lib.ma_last_error(None).decode(), xyz.cpu().numpy(), seed.cpu().numpy(), counts.cpu().numpy()

T_ = want["total"]
for tag, (capacity, max_pairs) in {"exact": (T_, 0), "short": (T_ - 1, 0), "capped": (T_, 1)}.items():
    rc, total, bound, msg, xyz, seed, counts = raw(capacity, max_pairs, T_)
    out["raw_" + tag + "_rc"], out["raw_" + tag + "_total"], out["raw_" + tag + "_bound"] = np.array(rc), np.array(total, np.uint64), np.array(bound, np.uint64)
    out["raw_" + tag + "_msg"], out["raw_" + tag + "_xyz"], out["raw_" + tag + "_seed"], out["raw_" + tag + "_counts"] = np.array(msg), xyz, seed, counts
try:
    pc_upsample.upsample_points(p, n, T.RADIUS, T.M, max_pairs=1)
    out["capped"] = np.array("")
except ValueError as e:
    out["capped"] = np.array(str(e))
try:
    pc_smooth.smooth_points(p, T.RADIUS, max_pairs=1)
    out["smooth_capped"] = np.array("")
except ValueError as e:
    out["smooth_capped"] = np.array(str(e))
try:
    pc_upsample.upsample_points(p, n, T.RADIUS, T.M, capacity=T_ - 1)
    out["short"] = np.array("")
except ValueError as e:
    out["short"] = np.array(str(e))
"""


@pytest.fixture(scope="module")
def kernel_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_upsample"), _KERNEL)[0]


def _equal(out, prefix, want, where):
    for w in ("xyz", "seed", "counts"):
        got = out[prefix + w]
        assert got.dtype == want[w].dtype and got.shape == want[w].shape, (where, w, got.shape, want[w].shape)
        assert got.tobytes() == want[w].tobytes(), (where, w)        # bitwise, order included
    assert int(out[prefix + "total"]) == want["xyz"].shape[0] == int(want["counts"].sum()), where


@pytest.mark.parametrize("name", sorted(UR.cases()))
def test_output_equals_the_brute_force_on_every_grid(kernel_out, name):
    assert {"sphere_ld3", "sphere_ld6", "cube", "sheets", "duplicated", "n1_m1", "n257_m1", "n5000_m1", "n8_m64", "inactive"} == set(UR.cases())
    cloud, normals, radius, m, active, grids = UR.cases()[name]
    assert len(grids) >= 2 and "auto" in grids
    want = UR.reference(name)
    for gname in grids:
        _equal(kernel_out, f"{name}__{gname}__", want, (name, gname))
    assert np.array_equal(kernel_out[name + "__count_only"], want["counts"]) and int(kernel_out[name + "__count_only_total"]) == int(want["counts"].sum())
    T = int(want["counts"].sum())
    print(f"{name}: N = {cloud.shape[0]}, m = {m}, {T} rows kept")
    if name == "inactive":
        assert T == 0
    else:
        assert T > 0
    if name == "n1_m1":
        assert want["counts"].tolist() == [4]                        # nobody to share with
    if name == "n8_m64":
        assert want["counts"].max() > 512                            # several rounds of 256 slots, each with kept candidates
    if name == "duplicated":                                        # of each triple the lowest row alone seeds
        order = np.random.default_rng(6).permutation(300)
        first = np.array([np.flatnonzero(order % 100 == k).min() for k in range(100)])
        rest = np.setdiff1d(np.arange(300), first)
        assert (want["counts"][rest] == 0).all() and (want["counts"][first] > 0).any()
    if name == "sheets":                                            # closer than R: a sheet's candidates stay its own
        z = want["xyz"][:, 2]
        assert set(np.unique(z).tolist()) == {0.0, float(np.float32(0.05))} and np.array_equal(z, cloud[want["seed"], 2])
    if name == "cube":
        assert (want["counts"][~active] == 0).all()


def test_new_rows_on_the_sphere_lie_in_the_tangent_planes(kernel_out):
    cloud, normals, radius, m, _, _ = UR.cases()["sphere_ld3"]
    assert cloud.shape == (300, 3) and radius == 0.3 and m == 8
    xyz = kernel_out["sphere_ld3__auto__xyz"].astype(np.float64)
    seed = kernel_out["sphere_ld3__auto__seed"]
    assert xyz.shape[0] > 3000
    off = np.abs(np.linalg.norm(xyz, axis=1) - 1.0)
    reach = np.linalg.norm(xyz - cloud[seed].astype(np.float64), axis=1)
    print(f"largest distance to the unit sphere {off.max():.6f} (bound {radius * radius / 2 + 1e-6:.6f}), to the seed {reach.max():.6f}")
    assert off.max() <= radius * radius / 2 + 1e-6                   # the tangent-plane offset sqrt(1 + R^2) - 1 <= R^2 / 2
    assert reach.max() <= radius + 4 * 2.0 ** -23 * np.abs(xyz).max()
    d = np.linalg.norm(xyz[:, None, :] - cloud[None].astype(np.float64), axis=2)
    assert (d.min(1) >= reach - 1e-6).all()                          # no row is nearer to a new row than its seed


def test_non_finite_rows_and_normals_seed_nothing(kernel_out):
    cloud, normals = nonfinite_case()
    want = UR.upsample_ref(cloud, normals, RADIUS, M)
    _equal(kernel_out, "nonfinite__", want, "nonfinite")
    assert (kernel_out["nonfinite__counts"][list(NONFINITE_ROWS)] == 0).all() and int(kernel_out["nonfinite__total"]) > 0
    assert np.isfinite(kernel_out["nonfinite__xyz"]).all()


def test_capacity_below_the_total_writes_nothing(kernel_out):
    cloud, normals = UR.sphere()
    want = UR.upsample_ref(cloud, normals, RADIUS, M)
    _equal(kernel_out, "abi_want__", want, "abi")
    T = want["xyz"].shape[0]
    assert int(kernel_out["raw_exact_rc"]) == 0 and int(kernel_out["raw_exact_total"]) == T
    assert np.array_equal(kernel_out["raw_exact_xyz"][:T], want["xyz"]) and np.array_equal(kernel_out["raw_exact_seed"][:T], want["seed"])
    assert np.array_equal(kernel_out["raw_exact_counts"], want["counts"])
    assert (kernel_out["raw_exact_xyz"][T:] == -7).all() and (kernel_out["raw_exact_seed"][T:] == -7).all() and kernel_out["raw_exact_xyz"].shape[0] == T + GUARD
    assert int(kernel_out["raw_short_rc"]) == -1 and int(kernel_out["raw_short_total"]) == T
    assert f"the total {T} exceeds the capacity {T - 1}" in str(kernel_out["raw_short_msg"])
    assert (kernel_out["raw_short_xyz"] == -7).all() and (kernel_out["raw_short_seed"] == -7).all() and (kernel_out["raw_short_counts"] == -7).all()
    assert f"the total {T} exceeds the capacity = {T - 1}" in str(kernel_out["short"])


def test_pair_bound_refuses_before_the_long_kernels(kernel_out):
    msg = str(kernel_out["capped"])
    m = re.search(r"pair bound (\d+) exceeds max_pairs 1\b", msg)
    assert m, msg
    s = re.search(r"pair bound (\d+) exceeds max_pairs 1\b", str(kernel_out["smooth_capped"]))
    assert s and int(m.group(1)) == int(s.group(1)) == int(kernel_out["raw_capped_bound"]) >= 300      # ma_op_pc_smooth's bound on the same grid; every row pairs with itself
    assert int(kernel_out["raw_capped_rc"]) == -1 and "ma_op_pc_upsample: the pair bound" in str(kernel_out["raw_capped_msg"])
    assert int(kernel_out["raw_capped_total"]) == 0
    assert (kernel_out["raw_capped_xyz"] == -7).all() and (kernel_out["raw_capped_seed"] == -7).all() and (kernel_out["raw_capped_counts"] == -7).all()


# ---- upsample_rows and the input side ---------------------------------------------------------------------------------------------------
TARGET = 4096
SPLIT_SMALL = 600


def two_spheres():
    """the 1500-row unit sphere and, far from it, a sphere of 600 rows and radius 0.6: the same point spacing"""
    big = UR.file_rows("float32", 6)
    p, n = UR.fibonacci(SPLIT_SMALL)
    small = np.concatenate([p * np.float32(0.6) + np.float32(5.0), n.astype(np.float32)], 1)
    return np.concatenate([big, small]).astype(np.float32)


_ROWS = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
for dt in ("float16", "float32", "float64"):
    for ld in (3, 6):
        tag = dt + "_" + str(ld)
        rows, fit = pc_upsample.upsample_rows(UR.file_rows(dt, ld), UR.FILE_RADIUS, T.TARGET, tag, return_fit=True)
        out["rows_" + tag], out["normals_" + tag], out["active_" + tag], out["m_" + tag], out["seed_" + tag] = rows, fit["normals"], fit["active"], np.array(fit["m"]), fit["seed"]
dense = UR.file_rows("float32", 6, 5000)
out["dense"] = pc_upsample.upsample_rows(dense, UR.FILE_RADIUS, T.TARGET, "dense")
try:
    pc_upsample.upsample_rows(UR.file_rows("float32", 3), 0.001, T.TARGET, "thin")
    out["thin"] = np.array("")
except ValueError as e:
    out["thin"] = np.array(str(e))
path = os.path.join(tmp, "sparse.npy")
np.save(path, UR.file_rows("float32", 6))
for kind in ("pc_normal", "pc_xyz"):
    for sampling in ("random", "fps"):
        np.random.seed(3)
        ds = Dataset(kind, [path], upsample_radius=UR.FILE_RADIUS, point_sampling=sampling)
        tag = kind + "_" + sampling
        out[tag + "_raw"], out[tag + "_item"], out[tag + "_keys"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"], np.array(sorted(ds[0]))
try:
    Dataset("pc_normal", [path])
    out["plain"] = np.array("")
except AssertionError as e:
    out["plain"] = np.array(str(e))
two = os.path.join(tmp, "two.npy")
np.save(two, T.two_spheres())
ds = Dataset("pc_normal", [two], upsample_radius=UR.FILE_RADIUS, cluster_radius=0.5, cluster_mode="split", cluster_min_points=64, point_sampling="fps")
out["split_len"] = np.array(len(ds))
for j in range(len(ds)):
    out["split_raw_" + str(j)], out["split_item_" + str(j)], out["split_uid_" + str(j)] = ds.data[j]["pc_normal"], ds[j]["pc_normal"], np.array(ds[j]["uid"])
"""


@pytest.fixture(scope="module")
def rows_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_upsample_rows"), _ROWS)


@pytest.mark.parametrize("ld", [3, 6])
@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
def test_upsample_rows_appends_the_restatements_rows(rows_out, dtype, ld):
    out, stdout = rows_out
    tag = f"{dtype}_{ld}"
    rows = UR.file_rows(dtype, ld)
    N = rows.shape[0]
    got, normals, active, m, seed = out["rows_" + tag], out["normals_" + tag], out["active_" + tag], int(out["m_" + tag]), out["seed_" + tag]
    assert N == 1500 and got.dtype == rows.dtype and got.shape[1] == ld and got.shape[0] >= TARGET and m in UR.LADDER
    assert got[:N].tobytes() == rows.tobytes()                       # the input rows first, bit for bit
    # the restatement fed with the normals the same call fitted (a second fit may differ in its last bits and flip a tie)
    want = UR.upsample_ref(rows[:, :3].astype(np.float32), normals, UR.FILE_RADIUS, m, active)
    assert np.array_equal(seed, want["seed"]) and got.shape[0] == N + want["xyz"].shape[0]
    assert got[N:, :3].tobytes() == want["xyz"].astype(rows.dtype).tobytes()
    assert got[N:, 3:].tobytes() == rows[seed][:, 3:].tobytes()      # every other column is the seed's
    if m > 2:                                                        # the ladder stopped at the first m that reaches the target
        fewer = UR.upsample_ref(rows[:, :3].astype(np.float32), normals, UR.FILE_RADIUS, m // 2, active)
        assert N + fewer["xyz"].shape[0] < TARGET
    line = re.search(rf"^{tag}: upsampling \(radius 0\.2, m {m}\) 1500 -> {got.shape[0]} rows, {int((~active).sum())} seeds had no plane$", stdout, re.M)
    assert line, stdout


def test_upsample_rows_leaves_a_dense_cloud_alone_and_refuses_a_radius_too_small(rows_out):
    out, stdout = rows_out
    dense = UR.file_rows("float32", 6, 5000)
    assert out["dense"].tobytes() == dense.tobytes() and out["dense"].shape == dense.shape
    assert "dense: upsampling (radius 0.2) not needed: 5000 rows, at least the 4096 asked for" in stdout
    assert re.search(r"upsampling 1500 rows at radius 0\.001 reaches 1500 rows at m = 64, fewer than the 4096 asked for: use a larger radius", str(out["thin"])), out["thin"]


@pytest.mark.parametrize("sampling", ["random", "fps"])
@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_dataset_takes_a_short_file(rows_out, kind, sampling):
    out, stdout = rows_out
    tag = f"{kind}_{sampling}"
    raw, item = out[tag + "_raw"], out[tag + "_item"]
    assert raw.shape == (N_POINTS, 6) and item.shape == (N_POINTS, 6) and item.dtype == np.float16 and out[tag + "_keys"].tolist() == ["pc_normal", "uid"]
    assert np.abs(np.linalg.norm(item[:, 3:].astype(np.float64), axis=1) - 1.0).max() < 2e-3          # unit normals, in float16
    assert np.abs(np.linalg.norm(raw[:, :3].astype(np.float64), axis=1) - 1.0).max() <= UR.FILE_RADIUS ** 2 / 2 + 1e-6
    cos = np.abs(np.einsum("ij,ij->i", raw[:, 3:6].astype(np.float64), UR.unit(raw[:, :3])))
    assert cos.min() > 0.9                                           # the seed's normal, or the estimate over the upsampled rows
    assert len(re.findall(r"^sparse: upsampling \(radius 0\.2, m \d+\) 1500 -> \d+ rows, 0 seeds had no plane$", stdout, re.M)) == 4
    assert "at least 4096 points" in str(out["plain"])               # the same file without the option is refused


def test_dataset_split_keeps_a_part_of_600_rows(rows_out):
    out, stdout = rows_out
    assert int(out["split_len"]) == 2 and [str(out[f"split_uid_{j}"]) for j in range(2)] == ["two_part0", "two_part1"]
    for j, (centre, radius) in enumerate([(0.0, 1.0), (5.0, 0.6)]):
        raw, item = out[f"split_raw_{j}"], out[f"split_item_{j}"]
        assert raw.shape == (N_POINTS, 6) and item.shape == (N_POINTS, 6) and item.dtype == np.float16
        r = np.linalg.norm(raw[:, :3].astype(np.float64) - centre, axis=1)
        assert np.abs(r - radius).max() <= UR.FILE_RADIUS ** 2 / (2 * radius) + 1e-5
    assert re.search(r"^two_part1: upsampling \(radius 0\.2, m \d+\) 600 -> \d+ rows, 0 seeds had no plane$", stdout, re.M), stdout


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_upsamples_a_sparse_raw_cloud_and_writes_a_mesh(tmp_path):
    """`python main.py --input_type pc_xyz --upsample_radius 0.2 --point_sampling fps --synthetic_weights --n_max_triangles 8` end to end
    (350M shape, seeded synthetic checkpoint, 8-face cap) on a 1500-row .xyz file: the upsampling line is printed and a mesh file is written."""
    np.savetxt(tmp_path / "sparse.xyz", UR.file_rows("float32", 3))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(tmp_path / "sparse.xyz"), "--input_type", "pc_xyz", "--out_dir",
                        str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0", "--upsample_radius", "0.2", "--point_sampling", "fps"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [f for _, _, fs in os.walk(out) for f in fs if f.endswith(".obj")]
    assert objs == ["sparse_gen.obj"]
    assert re.search(r"^sparse: upsampling \(radius 0\.2, m \d+\) 1500 -> \d+ rows, 0 seeds had no plane$", r.stdout, re.M), r.stdout
    assert "dataset total data samples: 1" in r.stdout and r.stdout.count("Over!!") == 1


# ---- every step of the input side at once ------------------------------------------------------------------------------------------------
ALL_STEPS = dict(outlier_k=16, outlier_std=2.0, plane_threshold=0.02, cluster_radius=0.15, cluster_min_points=64, smooth_radius=0.2,
                 upsample_radius=0.13, upsample_points=16384)


def all_steps_scene():
    """(5265, 6) float32: the unit sphere of 3000 rows (spacing 0.065), the table z = -1 under it as a 45 x 45 lattice over [-1.5, 1.5]^2 (spacing
    0.068, touching the sphere), a clump of 200 rows on a sphere of radius 0.15 two units off, and 40 strays in [-4, 4]^3; unit normals"""
    u = np.linspace(-1.5, 1.5, 45)
    table = np.stack([*(g.ravel() for g in np.meshgrid(u, u)), np.full(45 * 45, -1.0)], 1)
    p, n = UR.fibonacci(200)
    clump = np.concatenate([p.astype(np.float64) * 0.15 + np.array([3.0, 0.0, 0.5]), n], 1)
    strays = np.random.default_rng(12).uniform(-4.0, 4.0, (40, 3))
    up = [[0.0, 0.0, 1.0]]
    return np.concatenate([UR.file_rows("float32", 6, 3000), np.concatenate([table, np.repeat(up, 45 * 45, 0)], 1), clump,
                           np.concatenate([strays, np.repeat(up, 40, 0)], 1)]).astype(np.float32)


_ALL_STEPS = """
import contextlib
import io
import os
from meshanything_amd import pc_fps, pc_normals, pc_outliers, pc_plane
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
K = T.ALL_STEPS
np.save(os.path.join(tmp, "scene6.npy"), T.all_steps_scene())
np.save(os.path.join(tmp, "scene3.npy"), T.all_steps_scene()[:, :3])


def by_hand(kind, path, uid, sampling):
    floor = pc_upsample.MIN_ROWS                                    # upsampling is on
    rows = np.load(path)
    rows = pc_outliers.filter_rows(rows, K["outlier_k"], K["outlier_std"], floor, uid)
    rows = rows[pc_plane.remove_planes(rows, K["plane_threshold"], 1024, 1, 0.2, floor, uid)]
    rows = rows[pc_cluster.split_rows(rows, K["cluster_radius"], K["cluster_min_points"], "largest", uid)[0]]
    rows = pc_smooth.smooth_rows(rows, K["smooth_radius"], 1, uid)
    rows = pc_upsample.upsample_rows(rows, K["upsample_radius"], K["upsample_points"], uid)
    if kind == "pc_xyz":
        return pc_normals.xyz_to_pc_normal(rows, T.N_POINTS, 16, sampling=sampling)
    if sampling == "fps":
        return rows[pc_fps.fps_rows(rows, T.N_POINTS)]
    return rows[np.random.choice(rows.shape[0], T.N_POINTS, replace=False)]


for kind, uid in (("pc_normal", "scene6"), ("pc_xyz", "scene3")):
    for sampling in ("random", "fps"):
        tag = kind + "_" + sampling + "_"
        path = os.path.join(tmp, uid + ".npy")
        np.random.seed(7)
        with contextlib.redirect_stdout(io.StringIO()) as lines:
            ds = Dataset(kind, [path], point_sampling=sampling, **K)
        out[tag + "dataset"], out[tag + "dataset_stdout"], out[tag + "keys"] = ds.data[0]["pc_normal"], np.array(lines.getvalue()), np.array(sorted(ds.data[0]))
        out[tag + "len"], out[tag + "dataset_rng"] = np.array(len(ds)), np.random.get_state()[1]
        np.random.seed(7)
        with contextlib.redirect_stdout(io.StringIO()) as lines:
            out[tag + "hand"] = by_hand(kind, path, uid, sampling)
        out[tag + "hand_stdout"], out[tag + "hand_rng"] = np.array(lines.getvalue()), np.random.get_state()[1]
"""


@pytest.fixture(scope="module")
def all_steps_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_all_steps"), _ALL_STEPS)[0]


@pytest.mark.parametrize("sampling", ["random", "fps"])
@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_dataset_with_every_step_on_is_the_public_functions_composed_in_order(all_steps_out, kind, sampling):
    """outliers, plane, cluster, smooth, upsample, pick: the arrays bit for bit, the printed lines one for one and in order, the same draws
    from the numpy RNG; and on this scene every step does something, so that no other order would give these lines"""
    out, tag = all_steps_out, f"{kind}_{sampling}_"
    got, want = out[tag + "dataset"], out[tag + "hand"]
    assert int(out[tag + "len"]) == 1 and out[tag + "keys"].tolist() == ["pc_normal", "uid"]
    assert got.shape == want.shape == (N_POINTS, 6) and got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes()
    lines = str(out[tag + "hand_stdout"]).splitlines()
    assert str(out[tag + "dataset_stdout"]).splitlines() == lines + ["dataset total data samples: 1"]
    assert np.array_equal(out[tag + "dataset_rng"], out[tag + "hand_rng"])
    uid = "scene6" if kind == "pc_normal" else "scene3"
    assert len(lines) == 5, lines
    m = re.fullmatch(rf"{uid}: outlier filter removed (\d+) of 5265 points \(k = 16, threshold \S+\)", lines[0])
    assert m and 0 < int(m.group(1)) <= 40, lines[0]
    left = 5265 - int(m.group(1))
    m = re.fullmatch(rf"{uid}: plane removal \(threshold 0\.02\) removed 1 plane: (\d+) inliers, normal \(\S+ \S+ \S+\), dropped (\d+) of {left} points", lines[1])
    assert m and int(m.group(1)) == int(m.group(2)) >= 45 * 45, lines[1]
    left -= int(m.group(2))
    m = re.fullmatch(rf"{uid}: clustering \(radius 0\.15\) found (\d+) components, kept 1 \(sizes (\d+)\), dropped (\d+) of {left} points", lines[2])
    assert m and int(m.group(1)) > 1 and int(m.group(3)) >= 200 and int(m.group(2)) == left - int(m.group(3)), lines[2]
    left = int(m.group(2))
    assert re.fullmatch(rf"{uid}: smoothing \(radius 0\.2, 1 pass\) left \d+ of {left} rows in place .*", lines[3]), lines[3]
    m = re.fullmatch(rf"{uid}: upsampling \(radius 0\.13, m \d+\) {left} -> (\d+) rows, \d+ seeds had no plane", lines[4])
    assert m and int(m.group(1)) >= 16384 > left, lines[4]
