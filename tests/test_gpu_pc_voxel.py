"""Voxel thinning on the MI355X: the hash-table kernels (csrc/pc_voxel.hpp, meshanything_amd/pc_voxel.py) against the numpy restatement
`pc_voxel_ref.voxel_ref`, through `Dataset(..., voxel_size=...)` and through `main.py --voxel_size` on a .ply file.  Every GPU step runs in
a fresh interpreter under a time limit; the comparisons run here.

The rule is float32 arithmetic without contraction and the order (d, row index) is total, so the survivor of a voxel is unique: the keep
mask must EQUAL the restatement's byte for byte, on a second run, at the smallest capacity that holds the voxels and at 8 times that, and
with the cloud fed in chunks of 1 000 rows: there is no tolerance anywhere in this file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_fps_ref as F
import pc_voxel_ref as R

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
N_POINTS = 4096
E2E_LEAF = 0.04

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import pc_voxel_ref as R
from meshanything_amd import pc_voxel
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


def least_capacity(voxels):
    """the smallest table that holds `voxels` at half load"""
    return 1 << max(1, (2 * voxels - 1).bit_length())


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
_KERNELS = """
sys.path.insert(0, {tests!r})
import test_gpu_pc_voxel as T
for name, (cloud, leaf) in R.cases().items():
    keep, voxels = pc_voxel.voxel_keep(cloud, leaf)
    out[name + "_keep"], out[name + "_voxels"] = keep, np.array(voxels)
    least = T.least_capacity(R.reference(name)[1])
    runs = {{"twice": {{}}, "least": {{"capacity": least}}, "eightfold": {{"capacity": 8 * least}}, "chunks": {{"chunk_rows": 1000}},
            "chunks_least": {{"chunk_rows": 1000, "capacity": least}}}}
    for run, kw in runs.items():
        k2, v2 = pc_voxel.voxel_keep(cloud, leaf, **kw)
        out[name + "_" + run] = np.array(k2.tobytes() == keep.tobytes() and v2 == voxels and k2.dtype == np.bool_)
# ld 6 on the device: the (N, 6) tensor itself, in two inserts, against the origin voxel_keep would pass
cloud, leaf = R.cases()["sphere_ld6"]
origin = cloud[:, :3].min(0)
table = pc_voxel.new_table(16384, "cuda")
p = torch.from_numpy(cloud).cuda()
pc_voxel.insert(table, 16384, p[:7001], 0, origin, leaf)
pc_voxel.insert(table, 16384, p[7001:], 7001, origin, leaf)
keep, state = pc_voxel.mark(table, 16384, cloud.shape[0])
out["ld6_keep"], out["ld6_state"] = keep.cpu().numpy(), np.array([state[k] for k in ("used", "overflow", "out_of_range", "voxels")])
# the table at its load limit: 8 voxels in 16 slots
cloud, leaf = R.cases()["load_limit"]
keep, voxels = pc_voxel.voxel_keep(cloud, leaf, capacity=16, max_voxels=8)
out["limit_keep"], out["limit_voxels"] = keep, np.array(voxels)
# one voxel too many, then a table with no free slot at all: an error in time, and the next call in this process is right
nine = R.occupied(9)
for name, kw in (("overflow", {{"max_voxels": 8}}), ("full", {{"capacity": 8}}), ("tiny", {{"capacity": 2}})):
    try:
        pc_voxel.voxel_keep(nine, 1.0, **kw)
        out[name] = np.array("")
    except ValueError as e:
        out[name] = np.array(str(e))
    keep, voxels = pc_voxel.voxel_keep(nine, 1.0)
    out[name + "_then_keep"], out[name + "_then_voxels"] = keep, np.array(voxels)
try:
    pc_voxel.voxel_keep(np.array([[0, 0, 0], [1, 0, 0]], np.float32), 1.0 / (1 << 21))
    out["too_fine"] = np.array("")
except ValueError as e:
    out["too_fine"] = np.array(str(e))
""".format(tests=TESTS)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_voxel"), _KERNELS, timeout=240)[0]


@pytest.mark.parametrize("name", list(R.cases()))
def test_mask_equals_the_restatement(kernels, name):
    want, voxels = R.reference(name)
    got = kernels[name + "_keep"]
    assert got.dtype == np.bool_ and _same(got, want), (name, int(got.sum()), voxels)
    assert int(kernels[name + "_voxels"]) == voxels == int(got.sum())
    for run in ("twice", "least", "eightfold", "chunks", "chunks_least"):
        assert bool(kernels[name + "_" + run]), (name, run)
    if name == "one_voxel":
        assert R.cases()[name][0].shape[0] == 5000 and voxels == 1 and int(np.flatnonzero(got)[0]) == int(np.flatnonzero(want)[0])
    if name == "one_per_row_257":
        assert got.all() and got.shape == (257,)
    if name == "one_row":
        assert got.tolist() == [True]
    if name == "hand":
        assert got.tolist() == R.hand_cloud()[2].tolist()
    if name == "face_lattice":
        assert voxels == 729
    if name in ("sphere_ld3", "shifted"):
        assert got.shape == (20000,) and 2000 <= voxels <= 8000


def test_the_device_reads_rows_of_six_floats(kernels):
    want, voxels = R.reference("sphere_ld6")
    assert kernels["ld6_keep"].dtype == np.uint8 and _same(kernels["ld6_keep"].astype(bool), want)
    assert kernels["ld6_state"].tolist() == [voxels, 0, 0, voxels]


def test_a_table_at_its_load_limit(kernels):
    want, voxels = R.reference("load_limit")
    assert voxels == 8 and _same(kernels["limit_keep"], want) and int(kernels["limit_voxels"]) == 8


def test_a_full_table_ends_in_an_error_not_in_a_spin(kernels):
    nine = R.occupied(9)
    want, voxels, _ = R.voxel_ref(nine, 1.0)
    assert voxels == 9
    assert str(kernels["overflow"]) == "more than 8 voxels are occupied at voxel_size = 1: choose a larger one"
    assert str(kernels["full"]) == "more than 4 voxels are occupied at voxel_size = 1: choose a larger one"
    assert str(kernels["tiny"]) == "more than 1 voxels are occupied at voxel_size = 1: choose a larger one"
    for name in ("overflow", "full", "tiny"):
        assert _same(kernels[name + "_then_keep"], want) and int(kernels[name + "_then_voxels"]) == 9, name
    assert "too small" in str(kernels["too_fine"])


# ---- the input side ------------------------------------------------------------------------------------------------------------------------------
_E2E = f"""
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
rows = R.sphere_cloud(ld=6)
keep = R.voxel_ref(rows, {E2E_LEAF})[0]
dense, thinned = os.path.join(tmp, "scan.npy"), os.path.join(tmp, "thinned.npy")
np.save(dense, rows)
np.save(thinned, rows[keep])
np.random.seed(3)
before = np.random.get_state()[1].copy()
for kind in ("pc_normal", "pc_xyz"):
    ds = Dataset(kind, [dense], voxel_size={E2E_LEAF}, point_sampling="fps")
    out[kind + "_raw"], out[kind + "_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
    ds = Dataset(kind, [thinned], point_sampling="fps")
    out[kind + "_want_raw"], out[kind + "_want_item"] = ds.data[0]["pc_normal"], ds[0]["pc_normal"]
out["rng_untouched"] = np.array(np.array_equal(np.random.get_state()[1], before))
try:
    Dataset("pc_normal", [dense], voxel_size=0.2)
    out["too_few"] = np.array("")
except ValueError as e:
    out["too_few"] = np.array(str(e))
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_voxel_e2e"), _E2E, timeout=240)


def test_dataset_thins_before_it_samples(e2e):
    out, stdout = e2e
    rows = R.sphere_cloud(ld=6)
    keep, voxels, _ = R.voxel_ref(rows, E2E_LEAF)
    assert N_POINTS < voxels < 20000
    assert stdout.count(f"scan: voxel grid kept {voxels} of 20000 points (voxel_size {E2E_LEAF:g})") == 2
    assert bool(out["rng_untouched"])
    idx = F.fps_ref(rows[keep, :3], N_POINTS)[0]
    assert _same(out["pc_normal_raw"], rows[keep][idx])               # rows of the file, normals with them, in pick order
    assert _same(out["pc_xyz_raw"][:, :3], rows[keep][idx, :3])
    for kind in ("pc_normal", "pc_xyz"):                              # the rest of the pipeline on the reference-thinned rows
        assert _same(out[kind + "_raw"], out[kind + "_want_raw"]), kind
        assert out[kind + "_item"].dtype == np.float16 and _same(out[kind + "_item"], out[kind + "_want_item"]), kind
    few = R.voxel_ref(rows, 0.2)[1]
    assert few < N_POINTS and str(out["too_few"]) == f"scan: only {few} of 20000 points survive the voxel grid, fewer than the {N_POINTS} the encoder takes"


def test_cli_voxel_size_on_a_ply_file_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_normal --voxel_size 0.04 --input_path scan.ply --synthetic_weights --n_max_triangles 8` end to end (350M
    shape, seeded synthetic checkpoint, 8-face cap): the report line and one OBJ."""
    rows = R.sphere_cloud(ld=6)
    src = tmp_path / "scan.ply"
    R.write_ply(str(src), "binary_little_endian", rows[:, :3], rows[:, 3:], colours=True)
    voxels = R.voxel_ref(rows, E2E_LEAF)[1]
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_normal", "--voxel_size", str(E2E_LEAF),
                        "--out_dir", str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "scan_gen.obj"
    assert f"scan: voxel grid kept {voxels} of 20000 points (voxel_size {E2E_LEAF:g})" in r.stdout
    assert "dataset total data samples: 1" in r.stdout and "Generation Start!!!" in r.stdout and "Over!!" in r.stdout
