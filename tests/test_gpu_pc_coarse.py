"""Coarse registration on the MI355X (csrc/pc_coarse.hpp, meshanything_amd/pc_coarse.py): the four ops against the numpy restatement
`pc_coarse_ref` byte for byte, `register_rows(coarse=...)` on seed 3 of the fixture (a turn of 120 degrees), and the same directory through
`Dataset` and `main.py --coarse_radius`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

Histograms, descriptors, matches and counts are integers formed from float32 operations without contraction and with IEEE sqrt and /:
they must EQUAL the restatement's, whatever the grid and whatever the workspace held.  The matched distance is a sequential float32
sum: equal bytes too.  End to end the device's ops are bit-equal to the restatement's and only numpy's host arithmetic (and, for pc_xyz,
the device's own normal estimate) may differ, so the pose after ICP is held to twice the worst the restatement showed over six seeds
(test_pc_coarse_host.BOUNDS).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pc_coarse_ref as CR
import pc_register_ref as RR

from test_pc_coarse_host import BOUNDS                            # noqa: E402  twice the worst the restatement showed over six seeds

pytestmark = pytest.mark.gpu

REPO = CR.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
F_SMALL, F_LARGE = 0.05, 0.5625                                    # below one cell of the 16^3 grid (9/128) and at exactly eight of them
RUNS = tuple((F_SMALL, g) for g in ("one", "flat", "fine")) + ((F_LARGE, "one"), (F_LARGE, "fine"))

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import ctypes as C
import numpy as np
import torch
import pc_coarse_ref as CR
import pc_register_ref as RR
import test_gpu_pc_coarse as T
from meshanything_amd import _lib, pc_coarse, pc_register
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


def grid_of(name, table=RR.GRIDS):
    o, c, d = table[name]
    return np.array(o, np.float32), np.float32(c), np.array(d, np.int32)


def test_the_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    assert CR.SPFH_N == (1, 2, 63, 64, 65, 257, 4099) and CR.GATHER_Q == (1, 257)
    assert {s[0] for s in CR.MATCH_SHAPES} == {s[1] for s in CR.MATCH_SHAPES} == {1, 63, 64, 65, 257, 4096}
    assert {s[0] for s in CR.SCORE_SHAPES} == {1, 255, 256, 257, 4096} and {s[1] for s in CR.SCORE_SHAPES} == {1, 3, 257, 4096}
    assert [tuple(g[2]) for g in RR.GRIDS.values()] == [(1, 1, 1), (3, 2, 1), (16, 16, 16)]
    assert F_SMALL < RR.GRIDS["fine"][1] and float(np.float32(F_LARGE)) / float(np.float32(RR.GRIDS["fine"][1])) == 8.0


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
_KERNEL = """
lib = _lib.load()
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
def raw(cloud, normals, radius, grid, query, fill, max_pairs=0):
    # the C ABI itself on workspaces filled with `fill`, outputs filled with a sentinel -> (rc, message, bound, hist, rc of the gather, its message, desc)
    N = cloud.shape[0]
    o, c, d = grid
    need = lib.ma_pc_spfh_workspace_bytes(N, int(d[0]), int(d[1]), int(d[2]))
    ga = ((C.c_float * 3)(*o.tolist()), float(c), (C.c_int32 * 3)(*d.tolist()))
    nptr, nld = (cloud.data_ptr() + 12, 6) if normals is None else (normals.data_ptr(), normals.shape[1])
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    hist = torch.full((N, 34), -7, dtype=torch.int32, device="cuda")
    bound, most = C.c_uint64(0), C.c_uint32(0)
    rc = lib.ma_op_pc_spfh(cloud.data_ptr(), N, cloud.shape[1], nptr, nld, radius, *ga, max_pairs, hist.data_ptr(), C.byref(bound), C.byref(most), ws.data_ptr(), need, stream())
    msg = (lib.ma_last_error(None) or b"").decode()
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    desc = torch.full((query.shape[0], 33), -7, dtype=torch.int32, device="cuda")
    rc2 = lib.ma_op_pc_spfh_gather(cloud.data_ptr(), N, cloud.shape[1], radius, *ga, max_pairs, hist.data_ptr(), query.data_ptr(), query.shape[0], desc.data_ptr(), None,
                                   ws.data_ptr(), need, stream())
    msg2 = (lib.ma_last_error(None) or b"").decode()
    torch.cuda.synchronize()
    return rc, msg, bound.value, hist.cpu().numpy(), rc2, msg2, desc.cpu().numpy()
u32 = lambda t: t.cpu().numpy().astype(np.uint32)
def run(name, cloud_h, normals_h, radius, gname, grid, queries):
    cloud = torch.from_numpy(cloud_h).cuda()
    normals = None if normals_h is None else torch.from_numpy(normals_h).cuda()
    hist = pc_coarse.spfh(cloud, radius, "cloud" if normals is None else normals, grid)
    key = f"{name}_{gname}"
    out[key + "_hist"] = u32(hist)
    flags = []
    for Q, query_h in queries.items():
        query = torch.from_numpy(query_h).cuda()
        desc = pc_coarse.spfh_gather(cloud, hist, radius, query, grid)
        out[f"{key}_desc{Q}"] = u32(desc)
        rc, msg, bound, h_raw, rc2, msg2, d_raw = raw(cloud, normals, radius, grid, query, 0xFF)
        flags += [rc == 0 and rc2 == 0, h_raw.view(np.uint32).tobytes() == out[key + "_hist"].tobytes(), d_raw.view(np.uint32).tobytes() == out[f"{key}_desc{Q}"].tobytes()]
        out[key + "_bound"] = np.array(bound, np.uint64)
    out[key + "_flags"] = np.array(flags)
for N in CR.SPFH_N:
    for ld in (3, 6):
        cloud_h, normals_h = CR.cloud_case(N, ld)
        for radius, gname in T.RUNS:
            run(f"n{N}_ld{ld}_f{radius}", cloud_h, normals_h, radius, gname, T.grid_of(gname), {Q: CR.query_case(N, Q) for Q in CR.GATHER_Q})
content = CR.content_case()
for gname in CR.CONTENT_GRIDS:
    run("content", content, None, CR.CONTENT_RADIUS, gname, T.grid_of(gname, CR.CONTENT_GRIDS), {12: np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 2, 2, 0], np.int32)})
# the guard: 300 rows in one cell: the bound is 90 000 whatever the rings, above a cap of 1 000
cloud = torch.full((300, 6), 0.5, device="cuda") + torch.arange(300, device="cuda")[:, None] * 1e-4
query = torch.arange(4, dtype=torch.int32, device="cuda")
rc, msg, bound, hist, rc2, msg2, desc = raw(cloud, None, 0.05, T.grid_of("one"), query, 0, max_pairs=1000)
out["guard"] = np.array([f"{rc}|{bound}|{int((hist == -7).all())}|{msg}", f"{rc2}|0|{int((desc == -7).all())}|{msg2}"])
rc, msg, bound, hist, rc2, msg2, desc = raw(cloud, None, 0.05, T.grid_of("one"), query, 0, max_pairs=90000)
out["guard_at_cap"] = np.array([rc, rc2, bound, int((hist != -7).all() and (desc != -7).all())])
for fn, call in (("spfh", lambda: pc_coarse.spfh(cloud, 0.05, grid=T.grid_of("one"), max_pairs=1000)),
                 ("gather", lambda: pc_coarse.spfh_gather(cloud, torch.zeros((300, 34), dtype=torch.int64, device="cuda"), 0.05, query, T.grid_of("one"), max_pairs=1000))):
    try:
        call()
        out["guard_py_" + fn] = np.array([""])
    except ValueError as e:
        out["guard_py_" + fn] = np.array([str(e)])
for Ka, Kb in CR.MATCH_SHAPES:
    A, B = CR.match_case(Ka, Kb)
    idx, dist = pc_coarse.desc_match(torch.from_numpy(A.astype(np.int64)).cuda(), torch.from_numpy(B.astype(np.int64)).cuda())
    out[f"match_{Ka}_{Kb}_idx"], out[f"match_{Ka}_{Kb}_dist"] = idx.cpu().numpy(), dist.cpu().numpy()
for H, Cn in CR.SCORE_SHAPES:
    poses, P, Q, dist = CR.score_case(H, Cn)
    counts, best = pc_coarse.pose_score(torch.from_numpy(poses).cuda(), torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), dist)
    out[f"score_{H}_{Cn}_counts"], out[f"score_{H}_{Cn}_best"] = counts.cpu().numpy(), best.cpu().numpy()
"""


@pytest.fixture(scope="module")
def kernel_out(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_coarse"), _KERNEL)[0]


def _check(out, name, cloud, normals, radius, grids, queries):
    hist = CR.spfh_ref(cloud, normals, radius)
    for gname in grids:
        key = f"{name}_{gname}"
        got = out[key + "_hist"]
        assert got.dtype == np.uint32 and got.shape == hist.shape and got.tobytes() == hist.tobytes(), (key, np.argwhere(got != hist)[:8])
        for Q, query in queries.items():
            desc = CR.gather_ref(cloud, hist, radius, query)
            assert out[f"{key}_desc{Q}"].tobytes() == desc.tobytes(), (key, Q)
        assert out[key + "_flags"].all(), (key, out[key + "_flags"])                   # the raw ABI on a workspace of 0xFF: the same bytes
        assert int(out[key + "_bound"]) >= int(hist[:, 33].astype(np.int64).sum()), key
    return hist


@pytest.mark.parametrize("N", CR.SPFH_N)
def test_histograms_and_descriptors_equal_the_restatement_on_every_grid(kernel_out, N):
    for ld in (3, 6):
        cloud, normals = CR.cloud_case(N, ld)
        queries = {Q: CR.query_case(N, Q) for Q in CR.GATHER_Q}
        for radius in (F_SMALL, F_LARGE):
            hist = _check(kernel_out, f"n{N}_ld{ld}_f{radius}", cloud, CR.normals_of(cloud, normals), radius, [g for f, g in RUNS if f == radius], queries)
            print(f"N {N} ld {ld} F {radius}: used pairs {int(hist[:, 33].sum())}, most in a row {int(hist[:, 33].max())}")
            if N == 4099:
                assert hist[:, 33].max() > (4 if radius == F_SMALL else 1000) and (radius == F_LARGE or (hist[:, 33] == 0).any())


def test_some_rows_lie_outside_the_box_and_queries_repeat():
    cloud, _ = CR.cloud_case(4099, 3)
    o, c, d = grid_of("fine")
    assert ((cloud < o).any(1) | (cloud > o + c * d).any(1)).sum() > 100
    q = CR.query_case(4099, 257)
    assert len(set(q.tolist())) < 257 and CR.query_case(257, 1).tolist() == [256]


def test_duplicates_the_rim_a_lone_row_and_bad_normals(kernel_out):
    cloud = CR.content_case()
    queries = {12: np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 2, 2, 0], np.int32)}
    hist = _check(kernel_out, "content", cloud, cloud[:, 3:6], CR.CONTENT_RADIUS, list(CR.CONTENT_GRIDS), queries)
    got = kernel_out["content_one_hist"]
    assert not got[4].any() and not got[5].any() and not got[6].any()              # alone; a zero normal; a NaN normal
    assert got[0].tobytes() == got[1].tobytes() and got[0, 33] == 3                 # rows 2 (on the rim), 3 and 8; not the duplicate, not 5, 6 and 7
    assert got[2, 33] >= 2 and got[8, 10] + got[8, 9] > 0                          # the rim counts both ways; a normal of length 3 fills the last bins
    desc = kernel_out["content_one_desc12"]
    assert desc[9].tobytes() == desc[10].tobytes() == desc[2].tobytes() and not desc[4].any() and desc[5].any()   # a zero-normal row still gathers its neighbours
    assert np.array_equal(hist, got)


def test_the_guard_refuses_before_the_search(kernel_out):
    for entry, op in zip(kernel_out["guard"].tolist(), ("ma_op_pc_spfh", "ma_op_pc_spfh_gather")):
        rc, bound, untouched, msg = entry.split("|", 3)
        assert int(rc) != 0 and untouched == "1" and msg.startswith(f"{op}: the pair bound 90000 exceeds max_pairs 1000"), entry
    assert kernel_out["guard"][0].split("|")[1] == "90000"
    assert kernel_out["guard_at_cap"].tolist() == [0, 0, 90000, 1]
    assert "spfh: the pair bound 90000 exceeds max_pairs 1000" in str(kernel_out["guard_py_spfh"][0])
    assert "spfh_gather: the pair bound 90000 exceeds max_pairs 1000" in str(kernel_out["guard_py_gather"][0])


@pytest.mark.parametrize("shape", CR.MATCH_SHAPES, ids=lambda s: "%dx%d" % s)
def test_matches_equal_the_restatement_and_ties_go_to_the_lowest_index(kernel_out, shape):
    Ka, Kb = shape
    A, B = CR.match_case(Ka, Kb)
    idx, dist = CR.match_ref(A, B)
    got_i, got_d = kernel_out[f"match_{Ka}_{Kb}_idx"], kernel_out[f"match_{Ka}_{Kb}_dist"]
    assert got_i.dtype == np.int32 and got_d.dtype == np.float32
    assert got_i.tobytes() == idx.tobytes(), np.flatnonzero(got_i != idx)[:8]
    assert got_d.tobytes() == dist.tobytes()
    if Ka >= 63 and Kb >= 63:
        assert got_i[20:40].tolist() == list(range(20)) and not got_d[20:40].any()       # copies of rows that B holds twice: the first
        assert got_i[5] == 7 and got_d[5] == 0                                         # the all-zero descriptor finds the all-zero descriptor


@pytest.mark.parametrize("shape", CR.SCORE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_counts_equal_the_restatement_and_the_lowest_of_equal_counts_wins(kernel_out, shape):
    H, C = shape
    poses, P, Q, dist = CR.score_case(H, C)
    counts, best = CR.score_ref(poses, P, Q, dist)
    got = kernel_out[f"score_{H}_{C}_counts"]
    assert got.dtype == np.int32 and got.tobytes() == counts.tobytes(), np.flatnonzero(got != counts)[:8]
    assert kernel_out[f"score_{H}_{C}_best"].tolist() == [best]
    if (H, C) == (1, 1):
        assert counts.tolist() == [1]                                                  # a key equal to T^2 agrees
    else:
        assert counts[H // 2] == counts[H - 1] and counts[best] == counts.max() and not (counts[:best] == counts[best]).any()


# ---- the input side ------------------------------------------------------------------------------------------------------------------------
E2E_SEED = 3
COARSE = (CR.RADIUS, CR.POINTS, CR.ITERS, CR.DIST)


def write_scans(folder, kind):
    os.makedirs(folder, exist_ok=True)
    scans = CR.scans(E2E_SEED)
    for j, s in enumerate(scans):
        np.save(os.path.join(folder, f"scan{j}.npy"), s if kind == "pc_normal" else s[:, :3])
    return scans


_E2E = """
import os
from meshanything_amd.data import Dataset
tmp = os.path.dirname(os.path.abspath(__file__))
scans = CR.scans(T.E2E_SEED)
for kind in ("pc_normal", "pc_xyz"):
    rows, poses = pc_register.register_rows([s if kind == "pc_normal" else s[:, :3] for s in scans], CR.ICP_DIST, normal_k=None if kind == "pc_normal" else 16,
                                            uid=kind, coarse=T.COARSE)
    out[kind + "_rows"], out[kind + "_R"], out[kind + "_t"] = np.array(rows.shape), poses[1][0], poses[1][1]
folder = os.path.join(tmp, "ellipsoid")
T.write_scans(folder, "pc_normal")
np.random.seed(3)
ds = Dataset("pc_normal", [folder], register_dist=CR.ICP_DIST, coarse_radius=CR.RADIUS, coarse_points=CR.POINTS, coarse_iters=CR.ITERS, coarse_dist=CR.DIST)
item = ds[0]
out["ds_n"], out["ds_keys"], out["ds_uid"], out["ds_item"] = np.array(len(ds)), np.array(sorted(item)), np.array(item["uid"]), item["pc_normal"]
out["ds_R"], out["ds_t"] = np.stack([p[0] for p in item["scan_poses"]]), np.stack([p[1] for p in item["scan_poses"]])
try:
    Dataset("pc_normal", [folder], register_dist=CR.ICP_DIST)
    out["ds_without"] = np.array([""])
except ValueError as e:
    out["ds_without"] = np.array([str(e)])
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("pc_coarse_e2e"), _E2E)


def _within(label, pose):
    scans = CR.scans(E2E_SEED)
    R, t = pose
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    angle, move = RR.pose_errors(pose, CR.true_pose(E2E_SEED), scans[1][:, :3])
    print(f"{label}: rotation error {angle:.3e} rad (bound {BOUNDS['icp'][0]:.3e}), largest displacement {move:.3e} (bound {BOUNDS['icp'][1]:.3e})")
    assert angle <= BOUNDS["icp"][0] and move <= BOUNDS["icp"][1]


@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_register_rows_finds_a_turn_of_120_degrees(e2e, kind):
    out, stdout = e2e
    scans = CR.scans(E2E_SEED)
    assert out[kind + "_rows"].tolist() == [scans[0].shape[0] + scans[1].shape[0], 6 if kind == "pc_normal" else 3]
    _within(kind, (out[kind + "_R"], out[kind + "_t"]))
    assert stdout.count(f"{kind}: scan 1: coarse pose from ") == 1 and stdout.count(f"{kind}: scan 1: ") == 2


def test_dataset_carries_the_scan_poses_and_refuses_without_the_coarse_stage(e2e):
    out, stdout = e2e
    assert int(out["ds_n"]) == 1 and out["ds_keys"].tolist() == ["pc_normal", "scan_poses", "uid"] and str(out["ds_uid"]) == "ellipsoid"
    assert out["ds_item"].shape == (4096, 6) and out["ds_item"].dtype == np.float16
    assert out["ds_R"].shape == (2, 3, 3) and np.array_equal(out["ds_R"][0], np.eye(3)) and not out["ds_t"][0].any()
    _within("Dataset", (out["ds_R"][1], out["ds_t"][1]))
    assert "ellipsoid: scan scan1: coarse pose from " in stdout
    assert "ellipsoid: registration of scan scan1" in str(out["ds_without"][0]) and "do the scans start within --register_dist of each other?" in str(out["ds_without"][0])


def _cli(tmp_path, flags):
    folder = tmp_path / "ellipsoid"
    write_scans(str(folder), "pc_normal")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(folder), "--input_type", "pc_normal", "--register_dist", str(CR.ICP_DIST),
                        "--out_dir", str(out), "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"] + flags, capture_output=True, text=True, timeout=600)
    return r, [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]


def test_cli_coarse_radius_on_a_directory_writes_one_obj(tmp_path):
    """`python main.py --input_type pc_normal --register_dist 0.1 --coarse_radius 0.15 ... --input_path ellipsoid/` end to end."""
    r, objs = _cli(tmp_path, ["--coarse_radius", str(CR.RADIUS), "--coarse_points", str(CR.POINTS), "--coarse_dist", str(CR.DIST)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "ellipsoid_gen.obj"
    assert "ellipsoid: scan scan1: coarse pose from " in r.stdout and "dataset total data samples: 1" in r.stdout and "Over!!" in r.stdout


def test_cli_without_coarse_radius_the_same_directory_is_refused(tmp_path):
    r, objs = _cli(tmp_path, [])
    assert r.returncode != 0 and objs == [] and "do the scans start within --register_dist of each other?" in r.stderr and "coarse pose" not in r.stdout
