"""GPU surface sampling (meshanything_amd/surface_sample.py, csrc/surface_sample.hpp) on the MI355X: the kernels on hand-made draws
against the host sampler restated with the same draws (tests/surface_sample_ref.py), `mesh_to_pc_normal(..., device="cuda")` and
`process_mesh_to_pc(..., device="cuda")` against the host functions on the same RNG state, and `main.py --gpu_sampling` end to end.
Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_sample_ref as S
import watertight_ref as W

pytestmark = pytest.mark.gpu

REPO = W.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1, 2)
BOUNDARY_U = [0.0, 0.25, 0.75, 0.875, 1 - 2.0 ** -53, 1.0]        # first positive face, picks on cum boundaries, the top, the clamp

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import surface_sample_ref as S
import watertight_ref as W
from meshanything_amd import surface_sample, watertight
from meshanything_amd.mesh_input import mesh_to_pc_normal
out = {{}}

def on_device(v, f, u, uv):
    dv = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
    df = torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()
    normals, cum = surface_sample.surface_cdf(dv, df)
    draws = torch.from_numpy(np.concatenate([u, np.asarray(uv).reshape(-1)])).cuda()
    pc, idx = surface_sample.sample_draws(dv, df, normals, cum, draws, len(u), return_index=True)
    return pc.cpu().numpy(), idx.cpu().numpy(), normals.cpu().numpy(), cum.cpu().numpy()


def put(key, res):
    for part, a in zip(("pc", "idx", "normals", "cum"), res):
        out[key + "_" + part] = a
"""


def _gpu(tmp_path, body, timeout=600):
    """Run `body` (after _PRELUDE) in a fresh interpreter; it fills the dict `out`, which comes back as a dict of arrays."""
    script = tmp_path / "job.py"
    res = tmp_path / "out.npz"
    script.write_text(_PRELUDE + body + f"\nnp.savez({str(res)!r}, **out)\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(res) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ops(tmp_path_factory):
    body = f"""
v, f = S.boundary_mesh()
u = np.array({BOUNDARY_U!r})
uv = np.array([[0.25, 0.75], [0.5, 0.5000000000000001], [0.75, 0.25], [0.1, 0.2], [0.9, 0.3], [1 - 2.0 ** -53, 2.0 ** -53]])
put("boundary", on_device(v, f, u, uv))
# a vertex whose float16 needs one rounding from float64: 1 + 2^-11 + 2^-40 -> 1.000977, not 1.0
x = 1 + 2.0 ** -11 + 2.0 ** -40
v1 = np.array([[x, -x, 0.5], [x + 1, -x, 0.5], [x, 1 - x, 0.5]])
put("round", on_device(v1, [[0, 1, 2]], np.zeros(2), np.zeros((2, 2))))
rng = np.random.default_rng(4)
for name in ("torus", "sliver_soup", "open_box_degenerate", "dyadic"):
    v, f = S.MESHES[name]()
    u, uv = rng.random(8192), rng.random((8192, 2))
    out[name + "_u"], out[name + "_uv"] = u, uv
    put(name, on_device(v, f, u, uv))
"""
    return _gpu(tmp_path_factory.mktemp("ss_ops"), body)


def _res(ops, key):
    """(cloud, face index, normals, cum) of one on_device() call."""
    return tuple(ops[f"{key}_{part}"] for part in ("pc", "idx", "normals", "cum"))


def _check_against_host(got, v, f, u, uv, exact_cum):
    pc, idx, normals, cum = got
    ref_pc, ref_idx, ref_normals, ref_cum = S.host_sample(v, f, u, uv)
    assert pc.dtype == np.float16 and pc.shape == (len(u), 6) and idx.dtype == np.int64
    assert np.array_equal(normals.view(np.uint64), ref_normals.view(np.uint64))          # per face: bitwise numpy's
    if exact_cum:
        assert np.array_equal(cum, ref_cum)
    else:
        assert np.abs(cum - ref_cum).max() <= 1e-12 * ref_cum[-1]
    assert np.all(np.diff(cum) >= 0)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(pc.view(np.uint16), ref_pc.view(np.uint16))


def test_picks_follow_searchsorted_right_and_the_clamp(ops):
    v, f = S.boundary_mesh()
    pc, idx, normals, cum = _res(ops, "boundary")
    assert np.array_equal(cum, [0, 0.5, 0.5, 1.5, 1.75, 1.75, 2, 2])
    # u = 0: the first face with area; a pick on a boundary goes right, past the zero-area face; 1 - 2^-53 stays on the last face
    # with area; only u = 1 (pick = total, which no draw in [0, 1) reaches) is clamped to F - 1
    assert idx.tolist() == [1, 3, 4, 6, 6, 7]
    u = np.array(BOUNDARY_U)
    uv = np.array([[0.25, 0.75], [0.5, 0.5000000000000001], [0.75, 0.25], [0.1, 0.2], [0.9, 0.3], [1 - 2.0 ** -53, 2.0 ** -53]])
    _check_against_host(_res(ops, "boundary"), v, f, u, uv, exact_cum=True)


def test_uv_fold_is_strict(ops):
    v, f = S.boundary_mesh()
    pc = ops["boundary_pc"].astype(np.float64)
    t = v[f[1]]                                                    # u = 0 -> face 1; u + v == 1.0 exactly: not folded
    assert np.array_equal(pc[0, :3], (t[0] + 0.25 * (t[1] - t[0]) + 0.75 * (t[2] - t[0])).astype(np.float16))
    t = v[f[3]]                                                    # u + v > 1: folded to (0.5, 0.4999999999999999)
    assert np.array_equal(pc[1, :3], (t[0] + 0.5 * (t[1] - t[0]) + (1 - 0.5000000000000001) * (t[2] - t[0])).astype(np.float16))


def test_zero_area_faces_are_never_drawn(ops):
    for name in ("open_box_degenerate", "dyadic", "sliver_soup"):
        v, f = S.MESHES[name]()
        _, areas = S.face_normals_and_areas(v, f)
        idx = ops[name + "_idx"]
        assert (areas[idx] > 0).all(), name


def test_float16_is_rounded_once(ops):
    pc = ops["round_pc"]
    assert pc[0, 0] == np.float16(1.001) and pc[0, 0].view(np.uint16) == 0x3C01
    assert pc[0, 1].view(np.uint16) == 0xBC01


@pytest.mark.parametrize("name", ["torus", "sliver_soup", "open_box_degenerate", "dyadic"])
def test_kernels_match_numpy_on_the_same_draws(ops, name):
    v, f = S.MESHES[name]()
    _check_against_host(_res(ops, name), v, f, ops[name + "_u"], ops[name + "_uv"], exact_cum=name == "dyadic")


@pytest.fixture(scope="module")
def clouds(tmp_path_factory):
    body = f"""
for name, fn in S.MESHES.items():
    v, f = fn()
    for s in {SEEDS!r}:
        np.random.seed(s)
        out[f"{{name}}_{{s}}_host"] = mesh_to_pc_normal(v, f)
        out[f"{{name}}_{{s}}_host_next"] = np.random.random(4)
        np.random.seed(s)
        out[f"{{name}}_{{s}}_gpu"] = mesh_to_pc_normal(v, f, device="cuda")
        out[f"{{name}}_{{s}}_gpu_next"] = np.random.random(4)
v, f = S.no_area()
np.random.seed(9)
for dev in (None, "cuda"):
    try:
        mesh_to_pc_normal(v, f, device=dev)
        out[f"no_area_{{dev}}"] = np.array("no error")
    except ValueError as e:
        out[f"no_area_{{dev}}"] = np.array(str(e))
out["no_area_next"] = np.random.random(4)
"""
    return _gpu(tmp_path_factory.mktemp("ss_clouds"), body, timeout=900)


@pytest.mark.parametrize("name", list(S.MESHES))
def test_gpu_cloud_is_the_host_cloud(clouds, name):
    for s in SEEDS:
        host, gpu = clouds[f"{name}_{s}_host"], clouds[f"{name}_{s}_gpu"]
        assert gpu.dtype == np.float16 and gpu.shape == (4096, 6)
        assert np.array_equal(gpu.view(np.uint16), host.view(np.uint16)), (name, s)
        assert np.array_equal(clouds[f"{name}_{s}_gpu_next"], clouds[f"{name}_{s}_host_next"])   # the RNG moved on alike


def test_no_area_is_the_host_error_and_draws_nothing(clouds):
    assert str(clouds["no_area_None"]) == str(clouds["no_area_cuda"]) == "the mesh has no surface area"
    np.random.seed(9)
    assert np.array_equal(clouds["no_area_next"], np.random.random(4))


def test_process_mesh_to_pc_on_the_device_is_the_host_result(tmp_path):
    out = _gpu(tmp_path, """
meshes = [W.MESHES["open_box"](), W.MESHES["torus"](), W.MESHES["collinear"]()]
for dev in (None, "cuda"):
    np.random.seed(0)
    pcs, ms = watertight.process_mesh_to_pc(meshes, marching_cubes=True, device=dev)
    for i, (pc, (mv, mf)) in enumerate(zip(pcs, ms)):
        out[f"{dev}_pc{i}"], out[f"{dev}_v{i}"], out[f"{dev}_f{i}"] = pc, mv, mf
    out[f"{dev}_next"] = np.random.random(4)
    np.random.seed(1)
    pcs, _ = watertight.process_mesh_to_pc(meshes[:1], device=dev)
    out[f"{dev}_plain"] = pcs[0]
""", timeout=900)
    for i in range(3):
        assert out[f"cuda_v{i}"].dtype == np.float64 and out[f"cuda_f{i}"].dtype == np.int64
        assert np.array_equal(out[f"cuda_v{i}"].view(np.uint64), out[f"None_v{i}"].view(np.uint64))
        assert np.array_equal(out[f"cuda_f{i}"], out[f"None_f{i}"])
        assert np.array_equal(out[f"cuda_pc{i}"].view(np.uint16), out[f"None_pc{i}"].view(np.uint16))
    assert np.array_equal(out["cuda_next"], out["None_next"])
    assert np.array_equal(out["cuda_plain"].view(np.uint16), out["None_plain"].view(np.uint16))


@pytest.mark.parametrize("mc", [False, True], ids=["mesh", "mesh-mc"])
def test_cli_gpu_sampling_writes_the_same_obj_files(tmp_path, mc):
    """`main.py --input_dir DIR --input_type mesh [--mc] --synthetic_weights --n_max_triangles 8`, with and without --gpu_sampling:
    byte-identical OBJ files."""
    src = tmp_path / "in"
    src.mkdir()
    W.write_obj(src / "open_box.obj", *W.open_box())
    W.write_obj(src / "torus.obj", *W.torus())
    files = {}
    for gpu in (False, True):
        out = tmp_path / f"out_{int(gpu)}"
        cmd = [sys.executable, os.path.join(REPO, "main.py"), "--input_dir", str(src), "--input_type", "mesh", "--out_dir", str(out),
               "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"] + (["--mc"] if mc else []) + (["--gpu_sampling"] if gpu else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        objs = {fn: open(os.path.join(dp, fn), "rb").read() for dp, _, fs in os.walk(out) for fn in fs if fn.endswith("_gen.obj")}
        assert sorted(objs) == ["open_box_gen.obj", "torus_gen.obj"]
        files[gpu] = objs
    assert files[True] == files[False]
