"""Smoothing of input clouds on the MI355X (csrc/pc_smooth.hpp, meshanything_amd/pc_smooth.py): `count` against the brute force, the
float outputs against the eigh restatement `pc_smooth_ref.smooth_ref`, over four grids; the pair bound's cap; `smooth_rows`; through
`Dataset(..., smooth_radius=...)` and through `main.py --smooth_radius`.  Every GPU step runs in a fresh interpreter under a time limit;
the comparisons run here.

count[i] is an integer function of the cloud and the radius alone and must EQUAL the restatement's on every grid.  The float outputs are
sums whose order the walk decides; every term is the restatement's bit for bit, so they must agree with it to what float64 resolves:
max(1e-12, 100 x the spread between the restatement's two summation orders), on the rows with count >= min_count and a gap ratio
(l1 - l0) / l2 >= 0.05.  Measured on an MI355X, the largest deviation over the four grids (moved / R, sine, eigenvalues): see DESIGN.md
section 17.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pc_normals_ref as PN
import pc_smooth_ref as SR

pytestmark = pytest.mark.gpu

REPO = SR.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
EPS32 = float(np.finfo(np.float32).eps)

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import ctypes as C
import numpy as np
import torch
import pc_smooth_ref as SR
from meshanything_amd import _lib, pc_smooth
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


def nonfinite_cloud():
    """300 sphere points, one row NaN and one infinite: through an explicit grid, which `smooth_points` does not check for finiteness"""
    p = SR.noisy_sphere()[0][:300].copy()
    p[5, 1] = np.nan
    p[77, 0] = np.inf
    return p


NONFINITE_GRID = ((-1.1, -1.1, -1.1), 0.55, (4, 4, 4))
NONFINITE_RADIUS = 0.6
CAP_CASE = "n1025_ld3"

# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
_KERNEL = """
sys.path.insert(0, {tests!r})
import test_gpu_pc_smooth as T
for name, (cloud, radius, grids) in SR.count_cases().items():
    p = torch.from_numpy(cloud).cuda()
    for gname, grid in grids.items():
        got = pc_smooth.smooth_points(p, radius, SR.MIN_COUNT, grid, want=pc_smooth.WANT)
        for w in got:
            out[name + "__" + gname + "__" + w] = got[w].cpu().numpy()
# a strided view, the keys of the default call, count alone, another min_count
cloud, radius, _ = SR.count_cases()["n1025_ld6"]
p = torch.from_numpy(cloud).cuda()
wide = torch.cat([p, p], 1)
out["view_count"] = pc_smooth.smooth_points(wide[:, 6:], radius, want="count")["count"].cpu().numpy()
out["default_keys"] = np.array(sorted(pc_smooth.smooth_points(p, radius)))
got = pc_smooth.smooth_points(p, radius, min_count=30, want=pc_smooth.WANT)
for w in got:
    out["min30__" + w] = got[w].cpu().numpy()
# non-finite rows through an explicit grid
p = torch.from_numpy(T.nonfinite_cloud()).cuda()
got = pc_smooth.smooth_points(p, T.NONFINITE_RADIUS, SR.MIN_COUNT, T.NONFINITE_GRID, want=pc_smooth.WANT)
for w in got:
    out["nonfinite__" + w] = got[w].cpu().numpy()
# the cap: the ValueError of the Python call, and through the C ABI that nothing is written
cloud, radius, _ = SR.count_cases()[T.CAP_CASE]
p = torch.from_numpy(cloud).cuda()
try:
    pc_smooth.smooth_points(p, radius, max_pairs=1)
    out["capped"] = np.array("")
except ValueError as e:
    out["capped"] = np.array(str(e))
lib = _lib.load()
N = cloud.shape[0]
origin, cell, dims = pc_smooth.choose_cluster_grid(cloud, radius)
nbytes = lib.ma_pc_smooth_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
f = [torch.full((N, 3), -7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
cnt = torch.full((N,), -7, dtype=torch.int32, device="cuda")
bound = C.c_uint64(0)
rc = lib.ma_op_pc_smooth(p.data_ptr(), N, 3, radius, (C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist()), 6, 1, f[0].data_ptr(),
                         f[1].data_ptr(), f[2].data_ptr(), cnt.data_ptr(), C.byref(bound), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
torch.cuda.synchronize()
out["cap_rc"], out["cap_bound"], out["cap_message"] = np.array(rc), np.array(bound.value, np.uint64), np.array(lib.ma_last_error(None).decode())
out["cap_untouched"] = np.array(all(bool((t == -7).all()) for t in f + [cnt]))
""".format(tests=TESTS)


@pytest.fixture(scope="module")
def kernel_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_smooth"), _KERNEL)[0]


def _got(out, name, gname):
    return {w: out[f"{name}__{gname}__{w}"] for w in ("moved", "normals", "eigvals", "count")}


def _check_every_row(got, cloud, radius, min_count, name):
    """what holds on every row, the ill-posed ones included"""
    N = cloud.shape[0]
    q = cloud[:, :3].astype(np.float64)
    assert got["moved"].shape == (N, 3) and got["normals"].shape == (N, 3) and got["eigvals"].shape == (N, 3) and got["count"].shape == (N,), name
    assert got["moved"].dtype == got["normals"].dtype == got["eigvals"].dtype == np.float64 and got["count"].dtype == np.int32, name
    assert all(np.isfinite(got[w]).all() for w in ("moved", "normals", "eigvals")), name
    assert np.abs(np.linalg.norm(got["normals"], axis=1) - 1.0).max() <= 1e-14, name
    assert (np.linalg.norm(got["moved"] - q, axis=1) <= radius * (1 + 1e-6)).all(), name
    assert (np.diff(got["eigvals"], axis=1) >= 0).all(), name                         # ascending
    few = got["count"] < min_count
    assert np.array_equal(got["moved"][few], q[few]) and (got["normals"][few] == (0.0, 0.0, 1.0)).all() and (got["eigvals"][few] == 0).all(), name
    lead = np.take_along_axis(got["normals"], np.argmax(np.abs(got["normals"]), axis=1)[:, None], 1)[:, 0]
    assert (lead > 0).all(), name                                                     # the sign rule


def _check_floats(got, name, left_out_cap=None):
    """the float outputs against the eigh restatement on the well-posed rows -> the largest deviations"""
    radius = SR.count_cases()[name][1]
    want = SR.reference(name)
    rows = SR.well_posed(want)
    if left_out_cap is not None:
        assert (~rows).mean() <= left_out_cap, name
    if not rows.any():
        return (0.0, 0.0, 0.0)
    worst = tuple(float(v[rows].max()) for v in SR.deviations(got, want, radius))
    tol = SR.tolerance(name)
    assert all(w <= t for w, t in zip(worst, tol)), (name, worst, tol)
    return worst


@pytest.mark.parametrize("name", sorted(SR.count_cases()))
def test_count_equals_the_brute_force_and_every_row_is_sane_on_every_grid(kernel_out, name):
    assert SR.COUNT_N == (1, 2, 6, 255, 256, 257, 1025, 3000) and {f"n{N}_ld{ld}" for N in SR.COUNT_N for ld in (3, 6)} <= set(SR.count_cases())
    cloud, radius, grids = SR.count_cases()[name]
    assert {"auto", "one", "ratio8", "odd"} <= set(grids) and grids["odd"][2] == (5, 1, 17) and 7.99 < radius / grids["ratio8"][1] <= 8
    want = SR.count_ref(cloud, radius)
    first = None
    for gname in grids:
        got = _got(kernel_out, name, gname)
        assert np.array_equal(got["count"], want), (name, gname)
        _check_every_row(got, cloud, radius, SR.MIN_COUNT, (name, gname))
        worst = _check_floats(got, name)
        if first is None:
            first = got
        else:                                                        # the result does not depend on the grid
            assert np.array_equal(got["count"], first["count"])
            rows = SR.well_posed(SR.reference(name))
            if rows.any():
                between = tuple(float(v[rows].max()) for v in SR.deviations(got, first, radius))
                assert all(b <= t for b, t in zip(between, SR.tolerance(name))), (name, gname, between)
        print(f"{name} {gname}: largest deviation from the restatement {worst[0]:.2e} (moved / R), {worst[1]:.2e} (sine), {worst[2]:.2e} (eigenvalues)")
    if name == "whole" or cloud.shape[0] <= 6:
        assert (want == cloud.shape[0]).all()                        # a radius beyond the whole cloud
    if name == "lattice_1":
        assert want.max() == 7 and np.array_equal(first["moved"], cloud.astype(np.float64))   # keys EQUAL to r2 count and weigh nothing
    if name == "tripled":
        assert (want % 3 == 0).all()


@pytest.mark.parametrize("name", ["n3000_ld3", "cube"])
def test_floats_agree_with_the_eigh_restatement_on_the_sphere_and_the_cube(kernel_out, name):
    cloud, radius, grids = SR.count_cases()[name]
    assert cloud.shape == (3000, 3) and radius == {"n3000_ld3": 0.2, "cube": 0.25}[name]
    spread, tol = SR.spread(name), SR.tolerance(name)
    worst = np.max([_check_floats(_got(kernel_out, name, gname), name, left_out_cap=0.01) for gname in grids], axis=0)
    print(f"{name}: spread between the two CPU orders {spread[0]:.2e} / {spread[1]:.2e} / {spread[2]:.2e}, tolerance {tol[0]:.0e}, "
          f"largest GPU deviation {worst[0]:.2e} (moved / R), {worst[1]:.2e} (sine), {worst[2]:.2e} (eigenvalues)")


def test_a_view_the_default_call_and_min_count(kernel_out):
    cloud, radius, _ = SR.count_cases()["n1025_ld6"]
    assert kernel_out["default_keys"].tolist() == ["moved"]
    assert np.array_equal(kernel_out["view_count"], SR.count_ref(cloud, radius))
    got = {w: kernel_out["min30__" + w] for w in ("moved", "normals", "eigvals", "count")}
    few = got["count"] < 30
    assert 0.1 < few.mean() < 0.9                                    # both kinds of row
    _check_every_row(got, cloud, radius, 30, "min30")
    base = _got(kernel_out, "n1025_ld6", "auto")
    assert np.array_equal(got["count"], base["count"])
    assert np.abs(got["moved"][~few] - base["moved"][~few]).max() <= 1e-12 * radius   # min_count decides who stays, nothing else


def test_non_finite_rows_have_no_neighbours_and_stay(kernel_out):
    cloud = nonfinite_cloud()
    got = {w: kernel_out["nonfinite__" + w] for w in ("moved", "normals", "eigvals", "count")}
    want = SR.smooth_ref(cloud, NONFINITE_RADIUS)
    assert np.array_equal(got["count"], want["count"]) and got["count"][5] == 0 and got["count"][77] == 0
    for row in (5, 77):
        assert np.array_equal(got["moved"][row], cloud[row].astype(np.float64), equal_nan=True)
        assert got["normals"][row].tolist() == [0, 0, 1] and got["eigvals"][row].tolist() == [0, 0, 0]
    ok = np.ones(300, bool)
    ok[[5, 77]] = False
    rows = ok & SR.well_posed(want)
    dev = SR.deviations({w: got[w][rows] for w in got}, {w: want[w][rows] for w in want}, NONFINITE_RADIUS)
    assert rows.sum() > 200 and max(float(v.max()) for v in dev) <= 1e-12


def test_pair_bound_refuses_before_the_long_kernel(kernel_out):
    import pc_cluster_ref as CR
    from meshanything_amd import pc_cluster
    cloud, radius, _ = SR.count_cases()[CAP_CASE]
    msg = str(kernel_out["capped"])
    m = re.search(r"pair bound (\d+) exceeds max_pairs 1\b", msg)
    assert m, msg
    origin, cell, dims = pc_cluster.choose_cluster_grid(cloud, radius)
    assert int(m.group(1)) == CR.bound_ref(cloud, radius, origin, cell, dims) == int(kernel_out["cap_bound"])   # ma_op_pc_cluster's bound
    assert int(kernel_out["cap_rc"]) == -1 and "ma_op_pc_smooth: the pair bound" in str(kernel_out["cap_message"])
    assert bool(kernel_out["cap_untouched"])                         # no output is written past the refusal


# ---- smooth_rows and the input side -----------------------------------------------------------------------------------------------------
def file_rows(dtype, ld, n=3000):
    """the noisy sphere as a file of that dtype; with 6 columns the true normals, those of the odd rows negated"""
    p, true = SR.noisy_sphere(n)
    if ld == 3:
        return p.astype(dtype)
    side = np.where(np.arange(n) % 2 == 1, -1.0, 1.0)[:, None]
    return np.concatenate([p.astype(np.float64), true * side], 1).astype(dtype)


_ROWS = """
import os
sys.path.insert(0, {tests!r})
import test_gpu_pc_smooth as T
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
for dt in ("float16", "float32", "float64"):
    for ld in (3, 6):
        out["rows_" + dt + "_" + str(ld)] = pc_smooth.smooth_rows(T.file_rows(dt, ld), SR.SPHERE_RADIUS, 1, dt + str(ld))
rows = T.file_rows("float32", 6)
out["two"] = pc_smooth.smooth_rows(rows, SR.SPHERE_RADIUS, 2, "two")
once = pc_smooth.smooth_rows(rows, SR.SPHERE_RADIUS, 1, "once")
out["chained"] = pc_smooth.smooth_rows(once, SR.SPHERE_RADIUS, 1, "chained")
big = T.file_rows("float32", 6, 6000)
path = os.path.join(tmp, "noisy.npy")
np.save(path, big)
out["smoothed"] = pc_smooth.smooth_rows(big, SR.SPHERE_RADIUS, 1, "whole")
for kind in ("pc_normal", "pc_xyz"):
    np.random.seed(3)
    ds = Dataset(kind, [path], smooth_radius=SR.SPHERE_RADIUS)
    out[kind + "_raw"], out[kind + "_item"], out[kind + "_keys"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"], np.array(sorted(ds[0]))
np.random.seed(3)
out["pc_xyz_plain_raw"] = Dataset("pc_xyz", [path]).data[0]["pc_normal"]
np.random.seed(3)
ds = Dataset("pc_normal", [path], smooth_radius=SR.SPHERE_RADIUS, smooth_iters=2)
out["pc_normal_two_raw"] = ds.data[0]["pc_normal"]
""".format(tests=TESTS)


@pytest.fixture(scope="module")
def rows_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_smooth_rows"), _ROWS)


@pytest.mark.parametrize("ld", [3, 6])
@pytest.mark.parametrize("dtype", ["float16", "float32", "float64"])
def test_smooth_rows_keeps_dtype_and_shape_and_the_files_side(rows_out, dtype, ld):
    out, stdout = rows_out
    rows = file_rows(dtype, ld)
    got = out[f"rows_{dtype}_{ld}"]
    assert got.shape == rows.shape and got.dtype == rows.dtype
    want = SR.reference("n3000_ld3") if dtype != "float16" else SR.smooth_ref(rows[:, :3].astype(np.float32), SR.SPHERE_RADIUS)
    assert want["count"].min() >= SR.MIN_COUNT and SR.well_posed(want).all()
    # the float64 result within the kernel's tolerance, then one rounding to the file's dtype: half an ulp of a coordinate below 1.1
    cast = 0.0 if dtype == "float64" else float(np.finfo(dtype).eps) * 1.1
    assert np.abs(got[:, :3].astype(np.float64) - want["moved"]).max() <= 1e-12 * SR.SPHERE_RADIUS + cast
    m = re.search(rf"^{dtype}{ld}: smoothing \(radius 0\.2, 1 pass\) left 0 of 3000 rows in place for lack of neighbours, mean displacement (\S+), largest (\S+)$", stdout, re.M)
    assert m, stdout
    step = np.linalg.norm(want["moved"] - rows[:, :3].astype(np.float32).astype(np.float64), axis=1)
    assert abs(float(m.group(1).rstrip(",")) - step.mean()) <= 1e-5 * step.mean() and abs(float(m.group(2)) - step.max()) <= 1e-5 * step.max()
    if ld == 6:
        theirs, mine = rows[:, 3:6].astype(np.float64), got[:, 3:6].astype(np.float64)
        assert (np.einsum("ij,ij->i", theirs, mine) > 0).all()       # on the file's side, the negated rows too
        unit = mine / np.linalg.norm(mine, axis=1, keepdims=True)
        assert PN.sine(unit, want["normals"]).max() <= 1e-12 + 4 * cast
        assert np.abs(np.linalg.norm(mine, axis=1) - 1).max() <= 4 * cast + 1e-14


def test_two_passes_are_two_single_passes(rows_out):
    out, stdout = rows_out
    rows = file_rows("float32", 6)
    assert out["two"].shape == rows.shape and out["two"].dtype == np.float32
    # the second pass runs on the float32 cast of the first either way; a last-bit difference of the first pass's float64 result can move a
    # float32 input of the second by one ulp, which moves its output by about as much, and the file's dtype rounds once more
    assert np.abs(out["two"].astype(np.float64) - out["chained"].astype(np.float64)).max() <= 4 * EPS32 * 1.1
    assert "two: smoothing (radius 0.2, 2 passes) left 0 of 3000 rows" in stdout
    p, _ = SR.noisy_sphere()
    r1 = np.linalg.norm(SR.reference("n3000_ld3")["moved"], axis=1)
    r2 = np.linalg.norm(out["two"][:, :3].astype(np.float64), axis=1)
    assert np.std(r2) < np.std(r1) < np.std(np.linalg.norm(p.astype(np.float64), axis=1))   # a second pass smooths further


@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_dataset_items_are_rows_of_the_smoothed_cloud(rows_out, kind):
    out, stdout = rows_out
    _, true = SR.noisy_sphere(6000)
    np.random.seed(3)
    idx = np.random.choice(6000, N_POINTS, replace=False)            # the draw of both input types under this seed
    raw, smoothed = out[kind + "_raw"], out["smoothed"]
    assert raw.shape == (N_POINTS, 6) and out[kind + "_keys"].tolist() == ["pc_normal", "uid"] and out[kind + "_item"].dtype == np.float16
    # two runs of the kernel differ in the last bits of float64; the float32 file rounds that away except at a rounding boundary
    assert np.abs(raw[:, :3].astype(np.float64) - smoothed[idx, :3].astype(np.float64)).max() <= 2 * EPS32 * 1.1
    assert stdout.count("noisy: smoothing (radius 0.2, 1 pass) left 0 of 6000 rows in place for lack of neighbours") == 2
    cos = np.abs(np.einsum("ij,ij->i", raw[:, 3:6].astype(np.float64), true[idx]))
    if kind == "pc_normal":
        assert np.abs(raw[:, 3:6] - smoothed[idx, 3:6]).max() <= 2 * EPS32 and cos.min() > 0.95
        two = out["pc_normal_two_raw"]
        assert np.std(np.linalg.norm(two[:, :3].astype(np.float64), axis=1)) < np.std(np.linalg.norm(raw[:, :3].astype(np.float64), axis=1))
    else:
        plain = out["pc_xyz_plain_raw"]
        big = file_rows("float32", 6, 6000)
        assert np.array_equal(plain[:, :3], big[idx, :3])            # the same rows, unsmoothed
        cos_plain = np.abs(np.einsum("ij,ij->i", plain[:, 3:6].astype(np.float64), true[idx]))
        print(f"pc_xyz normals, mean |cos| against the true normals: {cos_plain.mean():.5f} without smoothing, {cos.mean():.5f} with")
        assert cos.mean() >= cos_plain.mean()


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_smooths_a_raw_cloud_and_writes_a_mesh(tmp_path):
    """`python main.py --input_type pc_xyz --smooth_radius 0.2 --synthetic_weights --n_max_triangles 8` end to end (350M shape, seeded
    synthetic checkpoint, 8-face cap): the smoothing line is printed and a mesh file is written."""
    np.save(tmp_path / "noisy.npy", SR.noisy_sphere(6000)[0])
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(tmp_path / "noisy.npy"), "--input_type", "pc_xyz", "--out_dir",
                        str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0", "--smooth_radius", "0.2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [f for _, _, fs in os.walk(out) for f in fs if f.endswith(".obj")]
    assert objs == ["noisy_gen.obj"]
    assert re.search(r"^noisy: smoothing \(radius 0\.2, 1 pass\) left 0 of 6000 rows in place for lack of neighbours, mean displacement \S+, largest \S+$", r.stdout, re.M)
    assert "dataset total data samples: 1" in r.stdout and r.stdout.count("Over!!") == 1
