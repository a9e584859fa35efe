"""Registration on the MI355X (csrc/pc_register.hpp, meshanything_amd/pc_register.py): pairs and sums of one ICP step against the numpy
restatement `pc_register_ref`, three scans of the test solid through `Dataset(..., register_dist=0.1)`, and `main.py --register_dist` on a
directory.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

The pair of a source row is the least of a total order over float32 keys formed without contraction: nn_idx and nn_d2 must EQUAL the
restatement's byte for byte, whatever the grid.  The 32 sums are formed in a fixed order without floating-point atomics: they must be the
same BYTES on a second run, on another grid and on a workspace that held 0xFF; against the exactly rounded restatement they may differ by
depth * 2^-52 * sum |term| per slot, depth = the longest chain of additions of that order (pc_register_ref.depth, from the header's
constants): the worst case of any summation of that depth, every term being the same float64 on both sides.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_register_ref as R

from meshanything_amd import pc_register                          # noqa: E402
from test_pc_register_host import BOUNDS                          # noqa: E402  twice the worst the restatement's ICP showed over eight seeds

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
D_SMALL, D_LARGE = 0.05, 0.5625                                    # below one cell of the 16^3 grid (9/128) and at exactly eight of them
RUNS = tuple((D_SMALL, g) for g in ("one", "flat", "fine")) + ((D_LARGE, "one"), (D_LARGE, "fine"))

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import ctypes as C
import numpy as np
import torch
import pc_register_ref as R
import test_gpu_pc_register as T
from meshanything_amd import _lib, pc_register
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


def grid_of(name, table=R.GRIDS):
    o, c, d = table[name]
    return np.array(o, np.float32), np.float32(c), np.array(d, np.int32)


def test_the_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    Ms, Ns = {s[0] for s in R.SHAPES}, {s[1] for s in R.SHAPES}
    assert Ms >= {1, 255, 256, 257, R.GROUP_ROWS - 1, R.GROUP_ROWS, R.GROUP_ROWS + 1} and Ns == {1, 257, 4099}
    assert {(s[2], s[3]) for s in R.SHAPES} == {(3, 3), (3, 6), (6, 3), (6, 6)}
    assert [tuple(g[2]) for g in R.GRIDS.values()] == [(1, 1, 1), (3, 2, 1), (16, 16, 16)]
    assert D_SMALL < R.GRIDS["fine"][1] and float(np.float32(D_LARGE)) / float(np.float32(R.GRIDS["fine"][1])) == 8.0
    assert R.depth(R.GROUP_ROWS + 1) == R.ROWS_PER_THREAD + 8 + 2


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
_KERNEL = """
lib = _lib.load()
def raw(tgt, src, grid, pose, centre, dist, normals, fill, max_pairs=0, want=("idx", "d2", "sums"), build=True):
    # normals: None or (device pointer, ld).  The C ABI itself on a workspace filled with `fill`, outputs filled with sentinels -> (rc, message, bound, outputs)
    N, M = tgt.shape[0], src.shape[0]
    o, c, d = grid
    need = lib.ma_pc_register_workspace_bytes(N, M, int(d[0]), int(d[1]), int(d[2]))
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    ga = ((C.c_float * 3)(*o.tolist()), float(c), (C.c_int32 * 3)(*d.tolist()))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if build:
        assert lib.ma_op_pc_register_build(tgt.data_ptr(), N, tgt.shape[1], src.data_ptr(), M, src.shape[1], *ga, ws.data_ptr(), need, s) == 0
    outs = {"idx": torch.full((M,), -7, dtype=torch.int32, device="cuda"), "d2": torch.full((M,), -7.0, dtype=torch.float32, device="cuda"),
            "sums": torch.full((32,), -7.0, dtype=torch.float64, device="cuda")}
    ptr = lambda w: outs[w].data_ptr() if w in want else None
    bound = C.c_uint64(0)
    rc = lib.ma_op_pc_register_step(tgt.data_ptr(), N, tgt.shape[1], src.data_ptr(), M, src.shape[1], *ga, (C.c_float * 12)(*pose.tolist()), (C.c_float * 3)(*centre.tolist()),
                                    dist, None if normals is None else normals[0], 0 if normals is None else normals[1], max_pairs, ptr("idx"), ptr("d2"),
                                    C.byref(bound), ptr("sums"), ws.data_ptr(), need, s)
    torch.cuda.synchronize()
    return rc, (lib.ma_last_error(None) or b"").decode(), bound.value, {w: t.cpu().numpy() for w, t in outs.items()}
same = lambda a, b: all(a[w].tobytes() == b[w].tobytes() for w in a)
def run(name, tgt_h, src_h, grids, pose, dist, plane):
    tgt, src = torch.from_numpy(tgt_h).cuda(), torch.from_numpy(src_h).cuda()
    for gname, grid in grids.items():
        built = pc_register.build(tgt, src, dist, grid)
        normals = None
        if plane:
            normals = "target" if tgt.shape[1] == 6 else torch.from_numpy(T.normals_for(tgt_h)).cuda()
        got = {w: t.cpu().numpy() for w, t in pc_register.icp_step(built, pose, R.CENTRE, dist, normals, want=pc_register.WANT).items()}
        again = {w: t.cpu().numpy() for w, t in pc_register.icp_step(built, pose, R.CENTRE, dist, normals, want=pc_register.WANT).items()}
        nt = None if not plane else ((tgt.data_ptr() + 12, 6) if tgt.shape[1] == 6 else (normals.data_ptr(), normals.shape[1]))   # (pointer, ld)
        rc, msg, bound, filled = raw(tgt, src, grid, pose, R.CENTRE, dist, nt, 0xFF)
        alone = pc_register.icp_step(built, pose, R.CENTRE, dist, normals)
        key = f"{name}_{'plane' if plane else 'point'}_{gname}"
        out[key + "_flags"] = np.array([same(got, again), rc == 0 and same(got, filled), list(alone) == ["sums"] and alone["sums"].cpu().numpy().tobytes() == got["sums"].tobytes()])
        out[key + "_bound"] = np.array(bound, np.uint64)
        for w in got:
            out[key + "_" + w] = got[w]
for M, N, sld, tld in R.SHAPES:
    tgt_h, src_h = R.uniform_case(M, N, sld, tld)
    for dist, gname in T.RUNS:
        for plane in (True, False):
            run(f"m{M}_n{N}_d{dist}", tgt_h, src_h, {gname: T.grid_of(gname)}, R.CASE_POSE, dist, plane)
tgt_h, src_h, pose, dist = R.content_case()
for plane in (True, False):
    run("content", tgt_h, src_h, {g: T.grid_of(g, R.CONTENT_GRIDS) for g in R.CONTENT_GRIDS}, pose, dist, plane)
# the guard: 300 target rows in one cell, 50 source rows on them: the bound is 15 000 whatever the rings, above a cap of 1 000
tgt = torch.full((300, 3), 0.5, device="cuda") + torch.arange(300, device="cuda")[:, None] * 1e-4
src = tgt[:50].clone()
eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32)
rc, msg, bound, outs = raw(tgt, src, T.grid_of("one"), eye, R.CENTRE, 0.05, None, 0, max_pairs=1000)
out["guard"] = np.array([f"{rc}|{bound}|{int((outs['idx'] == -7).all() and (outs['d2'] == -7).all() and (outs['sums'] == -7).all())}|{msg}"])
rc, msg, bound, outs = raw(tgt, src, T.grid_of("one"), eye, R.CENTRE, 0.05, None, 0, max_pairs=15000)
out["guard_at_cap"] = np.array([rc, bound, int((outs["idx"] == np.arange(50)).all())])
try:
    pc_register.icp_step(pc_register.build(tgt, src, 0.05, T.grid_of("one")), eye, R.CENTRE, 0.05, None, max_pairs=1000)
    out["guard_py"] = np.array([""])
except ValueError as e:
    out["guard_py"] = np.array([str(e)])
# refusals of the C ABI: non-zero, a message, nothing written
abi = []
for kw in (dict(want=()), dict(dist=0.0), dict(dist=float("inf")), dict(dist=17.0), dict(pose=np.full(12, np.nan, np.float32))):
    args = dict(tgt=tgt, src=src, grid=T.grid_of("one"), pose=eye, centre=R.CENTRE, dist=0.05, normals=None, fill=0)
    args.update(kw)
    rc, msg, bound, outs = raw(**args)
    abi.append(f"{rc}|{int((outs['idx'] == -7).all() and (outs['sums'] == -7).all())}|{msg}")
out["abi"] = np.array(abi)
"""


def normals_for(tgt):
    """The normals of a three-column target: a fixed random vector per row, of any length."""
    return np.random.default_rng(tgt.shape[0]).standard_normal((tgt.shape[0], 4)).astype(np.float32)


@pytest.fixture(scope="module")
def kernel_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_register"), _KERNEL)[0]


_REF = {}


def _ref(tgt, src, pose, dist, plane):
    """The restatement of one case, computed once."""
    key = (tgt.shape, src.shape, float(dist), plane, tgt.tobytes()[:64])
    if key not in _REF:
        normals = None if not plane else (tgt[:, 3:6] if tgt.shape[1] == 6 else normals_for(tgt)[:, :3])
        _REF[key] = R.sums_ref(tgt, src, pose, R.CENTRE, dist, normals)
    return _REF[key]


def _check(out, key, tgt, src, pose, dist, plane):
    sums, absum, idx, d2 = _ref(tgt, src, pose, dist, plane)
    got_i, got_d, got_s = out[key + "_idx"], out[key + "_d2"], out[key + "_sums"]
    assert got_i.dtype == np.int32 and got_d.dtype == np.float32 and got_s.dtype == np.float64 and got_s.shape == (32,), key
    assert got_i.tobytes() == idx.tobytes(), (key, np.flatnonzero(got_i != idx)[:8])
    assert got_d.tobytes() == d2.tobytes(), key
    assert out[key + "_flags"].all(), (key, out[key + "_flags"])
    tol = R.depth(src.shape[0]) * 2.0 ** -52 * absum
    err = np.abs(got_s - sums)
    print(f"{key}: pairs {int(sums[0])} skipped {int(sums[30])}, worst |sum - ref| / tolerance {float(np.max(err / np.where(tol > 0, tol, 1.0))):.3g}")
    assert (err <= tol).all(), (key, err, tol)
    assert got_s[0] == sums[0] and got_s[30] == sums[30] and got_s[31] == 0.0, key
    pairs = int(((got_i >= 0)).sum())
    assert int(out[key + "_bound"]) >= pairs, key
    return got_s


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "m%d_n%d_ld%d%d" % s)
def test_pairs_equal_the_restatement_and_the_sums_do_not_depend_on_grid_or_run(kernel_out, shape):
    M, N, sld, tld = shape
    tgt, src = R.uniform_case(M, N, sld, tld)
    for plane in (True, False):
        by_dist = {}
        for dist, gname in RUNS:
            key = f"m{M}_n{N}_d{dist}_{'plane' if plane else 'point'}_{gname}"
            by_dist.setdefault(dist, []).append(_check(kernel_out, key, tgt, src, R.CASE_POSE, dist, plane))
        for dist, all_sums in by_dist.items():
            assert len(all_sums) >= 2 and all(s.tobytes() == all_sums[0].tobytes() for s in all_sums), (shape, dist)


def test_some_rows_lie_outside_the_box_and_some_pairs_exist():
    tgt, src = R.uniform_case(257, 4099, 3, 6)
    p = R.transform_ref(src, R.CASE_POSE)
    o, c, d = grid_of("fine")
    assert ((p < o).any(1) | (p > o + c * d).any(1)).sum() > 20
    for dist in (D_SMALL, D_LARGE):
        idx = _ref(tgt, src, R.CASE_POSE, dist, True)[2]
        assert 10 < (idx >= 0).sum() and ((idx < 0).sum() > 10 or dist == D_LARGE)


@pytest.mark.parametrize("plane", [True, False], ids=["plane", "point"])
def test_duplicates_ties_the_rim_bad_rows_and_zero_normals(kernel_out, plane):
    tgt, src, pose, dist = R.content_case()
    sums = [_check(kernel_out, f"content_{'plane' if plane else 'point'}_{g}", tgt, src, pose, dist, plane) for g in R.CONTENT_GRIDS]
    assert sums[0].tobytes() == sums[1].tobytes()
    idx, d2 = kernel_out["content_plane_one_idx"], kernel_out["content_plane_one_d2"]
    assert idx.tolist() == [0, 2, 4, 5, -1, -1, 7]                   # the lower of duplicates, the lower of a tie, the rim, no pair twice
    assert d2[2] == np.float32(0.0625) and np.isinf(d2[4]) and np.isinf(d2[5]) and np.isfinite(sums[0]).all()
    assert (sums[0][0], sums[0][30]) == ((3.0, 2.0) if plane else (5.0, 0.0))


def test_the_guard_refuses_before_the_search(kernel_out):
    rc, bound, untouched, msg = str(kernel_out["guard"][0]).split("|", 3)
    assert int(rc) != 0 and int(bound) == 15000 and untouched == "1"
    assert msg.startswith("ma_op_pc_register_step: the pair bound 15000 exceeds max_pairs 1000")
    assert kernel_out["guard_at_cap"].tolist() == [0, 15000, 1]
    assert "the pair bound 15000 exceeds max_pairs 1000" in str(kernel_out["guard_py"][0])
    abi = [e.split("|", 2) for e in kernel_out["abi"].tolist()]
    for (rc, untouched, msg), word in zip(abi, ["no output", "max_dist", "max_dist", "max_dist / cell", "pose"]):
        assert int(rc) != 0 and untouched == "1" and msg.startswith("ma_op_pc_register_step:") and word in msg, (rc, untouched, msg)


# ---- the input side ------------------------------------------------------------------------------------------------------------------------
E2E_SEED = 11


def write_scans(folder, kind):
    """Three scans of the solid as files in sorted order: c_first, b_second and a_third would sort wrongly, so the names carry the order."""
    os.makedirs(folder, exist_ok=True)
    scans = R.solid_scans(E2E_SEED)
    for j, s in enumerate(scans):
        np.save(os.path.join(folder, f"scan{j}.npy"), s if kind == "pc_normal" else s[:, :3])
    return scans


_E2E = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
for kind in ("pc_normal", "pc_xyz"):
    folder = os.path.join(tmp, kind, "solid")
    T.write_scans(folder, kind)
    np.random.seed(3)
    ds = Dataset(kind, [folder], register_dist=R.DIST)
    item = ds[0]
    out[kind + "_n"], out[kind + "_keys"], out[kind + "_uid"], out[kind + "_item"] = np.array(len(ds)), np.array(sorted(item)), np.array(item["uid"]), item["pc_normal"]
    out[kind + "_R"], out[kind + "_t"] = np.stack([p[0] for p in item["scan_poses"]]), np.stack([p[1] for p in item["scan_poses"]])
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_register_e2e"), _E2E)


@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_dataset_registers_three_scans_of_the_solid(e2e, kind):
    out, stdout = e2e
    assert int(out[kind + "_n"]) == 1 and out[kind + "_keys"].tolist() == ["pc_normal", "scan_poses", "uid"] and str(out[kind + "_uid"]) == "solid"
    assert out[kind + "_item"].shape == (4096, 6) and out[kind + "_item"].dtype == np.float16
    Rs, ts = out[kind + "_R"], out[kind + "_t"]
    assert Rs.shape == (3, 3, 3) and Rs.dtype == np.float64 and ts.shape == (3, 3) and np.array_equal(Rs[0], np.eye(3)) and not ts[0].any()
    scans = R.solid_scans(E2E_SEED)
    angle_bound, move_bound = BOUNDS[kind]
    for j in (1, 2):
        assert np.abs(Rs[j] @ Rs[j].T - np.eye(3)).max() < 1e-14
        angle, move = R.pose_errors((Rs[j], ts[j]), R.TRUE_POSES[j], scans[j][:, :3])
        print(f"{kind} scan {j}: rotation error {angle:.3e} rad (bound {angle_bound:.3e}), largest displacement {move:.3e} (bound {move_bound:.3e})")
        assert angle <= angle_bound and move <= move_bound
    assert stdout.count("solid: registration (distance 0.1, plane metric): scan scan0 is the frame") == 2 and stdout.count("solid: scan scan1: ") == 2


def test_cli_register_dist_on_a_directory_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_normal --register_dist 0.1 --input_path solid/ --synthetic_weights --n_max_triangles 8` end to end."""
    folder = tmp_path / "solid"
    write_scans(str(folder), "pc_normal")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(folder), "--input_type", "pc_normal", "--register_dist", str(R.DIST),
                        "--out_dir", str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "solid_gen.obj"
    assert "solid: scan scan2: " in r.stdout and "dataset total data samples: 1" in r.stdout and "Over!!" in r.stdout
