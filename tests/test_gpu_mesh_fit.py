"""The mesh fit on the MI355X (csrc/mesh_fit.hpp, meshanything_amd/mesh_fit.py): the pairing and the per-face sums
against the float32 restatement of tests/mesh_fit_ref.py, bit for bit, and against the float64 definition; `fit_mesh` end to end on
crafted meshes; `main.py --fit_iters 2`.  Every GPU step runs in a fresh interpreter under a time limit; the comparisons run here.

Tolerance.  The yardstick is the restatement against float64, never the kernel against itself: `mesh_fit_ref.figures()` measures the
largest deviation of (b) from (a) on the very inputs of `kernel_cases()`, per point (s, |p - c|^2 and the nearest point c) and per face
(a sum divided by the face's count), and the `refs` fixture prints it; the kernel may deviate from (a) by at most 8 times those figures,
and the end-to-end results from (a)'s by 8 times the per-point one.  A point may be paired with another face than (a)'s only where
(a)'s two best faces are within float32 resolution of each other (RESOLUTION below).
"""
# the figures as computed by `mesh_fit_ref.figures()`: per point 9.87e-06, per face 3.55e-03 -- both set by the slivers of "m600_p4096",
# whose weights (not the point they name) are ill-conditioned across their width of 2e-4; the cube alone gives 1.8e-07 and 2.4e-08
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_fit_ref as R

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))
# squared distances here are below 0.01 and carry about ten float32 roundings each: two faces whose squared distances differ by less
# than 16 ulp of 0.01 cannot be told apart in float32
RESOLUTION = 16 * 0.01 * 2.0 ** -23

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import mesh_fit_ref as R
from meshanything_amd import _lib, mesh_fit
out = {{}}

def run(v, f, cl, d, mc, ws=None):
    o = mesh_fit.fit_pairs(torch.from_numpy(np.asarray(v)).cuda(), f, torch.from_numpy(np.asarray(cl)), d, mc, mesh_scale=1.0, workspace=ws)
    torch.cuda.synchronize()
    return {{k: t.cpu().numpy().copy() for k, t in o.items()}}

def keep(name, o):
    for k, t in o.items():
        out[name + "_" + k] = t
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


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    body = """
cases = R.kernel_cases()
for name, c in cases.items():
    keep(name, run(*c))
v, f, cl, d, mc = cases["m257_p257_cos"]
keep("again", run(v, f, cl, d, mc))
need = _lib.load().ma_mesh_fit_workspace_bytes(len(v), len(f), len(cl))
big = torch.full((need + 8192,), 0xA5, dtype=torch.uint8, device="cuda")          # another placement, and not zeroed
keep("moved", run(v, f, cl, d, mc, big[4096 + 256:]))
# a float16 cloud is the float32 cloud of the same values
v, f, cl, d, mc = cases["m256_p257_f16"]
keep("f16_as_f32", run(v, f, cl.astype(np.float32), d, mc))
# what the kernels find in the arrays themselves comes back as an error of the call (the Python checks are bypassed here)
v, f, cl, d, mc = cases["m2_p64_cos"]
x = torch.from_numpy(v).cuda()
c32 = torch.from_numpy(cl).cuda()
bad_f = torch.tensor([[0, 1, 2], [3, 4, 6]], dtype=torch.int32, device="cuda")
bad_x = x.clone(); bad_x[4, 1] = float("nan")
bad_c = c32.clone(); bad_c[7, 5] = float("inf")
good_f = torch.from_numpy(f).to(torch.int32).cuda()
for name, args in (("bad_index", (x, bad_f, c32)), ("bad_vertex", (bad_x, good_f, c32)), ("bad_cloud", (x, good_f, bad_c))):
    try:
        mesh_fit._pairs(*args, d, 0.0)
        out[name] = np.array("")
    except _lib.MAError as e:
        out[name] = np.array(str(e))
torch.cuda.synchronize()
try:
    mesh_fit.fit_pairs(x, f, bad_c, d)
    out["py_bad_cloud"] = np.array(False)
except ValueError:
    out["py_bad_cloud"] = np.array(True)
"""
    return _gpu(tmp_path_factory.mktemp("fit_kernels"), body)


@pytest.fixture(scope="module")
def refs():
    """name -> ((b), (a)) of every kernel case, computed once, and the figures"""
    pt, fc, mism = R.figures()
    print(f"restatement (b) against float64 (a): per point {pt:.3e}, per face {fc:.3e}; tolerances 8 x; differently paired: "
          f"{ {k: v for k, v in mism.items() if v} }")
    both = {}
    for name, (v, f, cl, d, mc) in R.kernel_cases().items():
        both[name] = (R.pairs_f32(v, f, cl, d, mc), R.pairs_ref(v, f, np.asarray(cl).astype(np.float32), d, mc))
    return both, pt, fc


def _got(kernels, name):
    return {"face": kernels[name + "_face"], "w": kernels[name + "_weights"], "s": kernels[name + "_s"], "r2": kernels[name + "_r2"],
            "sums": kernels[name + "_sums"]}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("name", list(R.kernel_cases()))
def test_kernel_equals_the_float32_restatement_bit_for_bit(kernels, refs, name):
    got, (b, _) = _got(kernels, name), refs[0][name]
    assert got["face"].dtype == np.int32 and got["sums"].dtype == np.int64
    assert np.array_equal(got["face"], b["face"])
    for k in ("w", "s", "r2"):
        assert np.array_equal(_bits(got[k]), _bits(b[k])), k
    assert np.array_equal(got["sums"], b["sums"])
    assert np.array_equal(got["sums"][:, 0].sum(), (b["face"] >= 0).sum())


def test_the_crafted_points_pair_as_worked_out_by_hand(kernels):
    g = _got(kernels, "quad_p63")
    assert g["face"][:5].tolist() == [0, 0, 0, -1, -1]               # shared edge and shared vertex: the lowest index; inside; outside; zero normal
    assert g["w"][0].tolist() == [0.5, 0.0, 0.5] and g["w"][1].tolist() == [1.0, 0.0, 0.0]
    assert g["r2"][2] == np.float32(0.0625) ** 2 and g["s"][2] == np.float32(0.0625)
    assert not g["w"][3:5].any() and not g["s"][3:5].any()
    u = _got(kernels, "unpaired")
    assert (u["face"] == -1).all() and not u["sums"].any() and not u["w"].any()
    assert (_got(kernels, "m1_p1")["face"] >= -1).all()


def test_same_bits_twice_elsewhere_and_for_a_float16_cloud(kernels):
    for other, base in (("again", "m257_p257_cos"), ("moved", "m257_p257_cos"), ("f16_as_f32", "m256_p257_f16")):
        a, b = _got(kernels, other), _got(kernels, base)
        assert np.array_equal(a["face"], b["face"]) and np.array_equal(a["sums"], b["sums"])
        for k in ("w", "s", "r2"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (other, k)


def test_bad_arrays_are_returned_errors(kernels):
    assert "face index" in str(kernels["bad_index"]) and "MA_ERR_INVALID" in str(kernels["bad_index"])
    assert "non-finite" in str(kernels["bad_vertex"]) and "vertex" in str(kernels["bad_vertex"])
    assert "non-finite" in str(kernels["bad_cloud"]) and "cloud" in str(kernels["bad_cloud"])
    assert bool(kernels["py_bad_cloud"])


@pytest.mark.parametrize("name", list(R.kernel_cases()))
def test_kernel_against_the_float64_definition(kernels, refs, name):
    both, pt, fc = refs
    got, (_, a) = _got(kernels, name), both[name]
    v, f, cl, _, _ = R.kernel_cases()[name]
    dp, df, diff = R.compare(got, a, v, f, np.asarray(cl).astype(np.float32))
    print(f"{name}: kernel against (a): per point {dp:.3e} (allowed {8 * pt:.3e}), per face {df:.3e} (allowed {8 * fc:.3e}), differently paired {len(diff)}")
    assert dp <= 8 * pt and df <= 8 * fc
    for q in diff:                                                       # only where float32 cannot tell (a)'s two best faces apart
        assert a["gap"][q] <= RESOLUTION, (q, a["face"][q], got["face"][q], a["gap"][q])


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    body = """
def fit(name, v, f, cl, iters, **kw):
    vv, rep = mesh_fit.fit_mesh(v, f, cl, iters, **kw)
    out[name + "_verts"] = np.asarray(vv)
    out[name + "_same_object"] = np.array(vv is v)
    out[name + "_kept"] = np.array(rep["kept"])
    out[name + "_scores"] = np.array([rep["score_before"], rep["score_after"]], np.float64)
    out[name + "_its"] = np.array([[i["paired"], i["rms"], i["move"]] for i in rep["iterations"]], np.float64)
    out[name + "_max_move"] = np.array(rep["max_move"])
    out[name + "_line"] = np.array(mesh_fit.report_line(name, rep))

v, f = R.jittered_cube()
fit("cube", v, f, R.cube_cloud(), 4)
fit("cube_f16", v, f, R.cube_cloud(dtype=np.float16), 4)
fit("shifted", v, f, R.shifted_cloud(10.0), 4)
v, f = R.pulled_cube(6.0)
fit("pulled", v, f, R.cube_cloud(), 4, max_move=2.0)
v, f = R.fin_cube()
fit("fin", v, f, R.cube_cloud(), 4)
v, f = R.open_cube()
fit("open", v, f, R.cube_cloud(), 4)
# tensors in, tensor out
v, f = R.jittered_cube()
vv, rep = mesh_fit.fit_mesh(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(R.cube_cloud()).cuda(), 4)
out["cube_cuda_verts"] = vv.cpu().numpy()
out["cube_cuda_is_cuda"] = np.array(vv.is_cuda and vv.dtype == torch.float32)
"""
    return _gpu(tmp_path_factory.mktemp("fit_e2e"), body)


def _cube_error(verts):
    return float(np.abs(np.asarray(verts, np.float64) * 2.0 - R.cube_mesh()[0]).max())


def test_jittered_cube_is_pulled_onto_the_cloud(fits, refs):
    _, pt, _ = refs
    v, f = R.jittered_cube()
    want, _ = R.fit_ref(v, f, R.cube_cloud(), 4)
    got = fits["cube_verts"]
    start, end = _cube_error(v), _cube_error(got)
    print(f"jittered cube: largest vertex error {start:.3e} -> {end:.3e} ({start / end:.0f} x), against (a) {np.abs(got * 2.0 - want * 2.0).max():.3e}")
    assert got.dtype == np.float32 and bool(fits["cube_kept"])
    assert np.abs(got.astype(np.float64) * 2.0 - want * 2.0).max() <= 8 * pt        # in cloud units, as the figure is
    assert end * 100 <= start
    assert np.array_equal(fits["cube_cuda_verts"], got) and bool(fits["cube_cuda_is_cuda"])
    # the float16 rows the CLI fits against: the rounding of 0.4 to float16 (2^-12 at most) is all that is left
    assert _cube_error(fits["cube_f16_verts"]) <= 2.0 ** -12 and bool(fits["cube_f16_kept"])
    s = fits["cube_scores"]
    assert s[1].sum() < s[0].sum()
    assert re.fullmatch(r"cube: fit \d iterations, 4096 of 4096 points paired, RMS \S+ -> \S+, largest move \S+ steps, total \S+ -> \S+, kept", str(fits["cube_line"]))


def test_a_cloud_out_of_reach_changes_nothing(fits):
    v, _ = R.jittered_cube()
    assert bool(fits["shifted_same_object"]) and not bool(fits["shifted_kept"])
    assert np.array_equal(_bits(fits["shifted_verts"]), _bits(v))
    assert fits["shifted_its"].tolist() == [[0.0, 0.0, 0.0]] and float(fits["shifted_max_move"]) == 0.0
    assert str(fits["shifted_line"]).endswith("not kept: the decoder's vertices are written") and " 0 of 4096 points paired" in str(fits["shifted_line"])


def test_a_pulled_vertex_moves_the_cap_and_no_further(fits):
    v, _ = R.pulled_cube(6.0)
    got = fits["pulled_verts"]
    d = (got.astype(np.float64) - v.astype(np.float64)) * 2.0            # cloud units
    cap = 2.0 * R.STEP
    ln = np.linalg.norm(d, axis=1)
    # float32 rounding of the written vertex (coordinates below 0.25 in mesh units: 2^-25 each, doubled, three axes)
    eps = 3 * 2.0 ** -24
    assert bool(fits["pulled_kept"])
    assert abs(ln[7] - cap) <= eps and (ln <= cap + eps).all()
    toward = -np.ones(3) / np.sqrt(3.0)
    assert d[7] @ toward >= cap * (1 - 1e-6)                             # along the diagonal, back toward the corner
    assert abs(float(fits["pulled_max_move"]) - cap) <= 1e-12


def test_unsupported_vertices_do_not_move(fits):
    v, _ = R.fin_cube()
    got = fits["fin_verts"]
    assert bool(fits["fin_kept"])
    assert np.array_equal(_bits(got[8]), _bits(v[8]))                   # the fin's apex: no paired point carries weight on it
    assert _cube_error(got[:8]) * 100 <= _cube_error(v[:8])


def test_the_guard_decides_on_an_unmeshed_side(fits):
    v, _ = R.open_cube()
    s = fits["open_scores"]
    assert s.shape == (2, 2) and np.isfinite(s).all() and (s > 0).all()
    kept = bool(fits["open_kept"])
    assert kept == bool(0.5 * s[1].sum() < 0.5 * s[0].sum())
    assert kept or np.array_equal(_bits(fits["open_verts"]), _bits(v))
    assert (kept and str(fits["open_line"]).endswith(", kept")) or str(fits["open_line"]).endswith("not kept: the decoder's vertices are written")
    assert 0 < fits["open_its"][0, 0] <= 1.0


def _read_obj(path):
    vs, fs = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            vs.append([float(x) for x in t[1:4]])
        elif t and t[0] == "f":
            fs.append([int(x) for x in t[1:4]])
    return np.array(vs), np.array(fs)


def test_cli_fit_iters_writes_the_same_faces_and_close_vertices(tmp_path):
    """`python main.py --input_path mouse.npy --input_type pc_normal --fit_iters 2 ...` (350M shape, seeded synthetic checkpoint, 8-face
    cap) against the same run without the flag: the line, the same face list, vertices at most --fit_max_move (2 steps = 1/64) apart."""
    g = np.load(os.path.join(REPO, "tests", "golden", "dataset.npz"))
    src = tmp_path / "mouse.npy"
    np.save(src, g["mouse_raw"])
    meshes = {}
    for name, extra in (("plain", []), ("fit", ["--fit_iters", "2"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_normal", "--out_dir", str(out),
                            "--synthetic_weights", "--n_max_triangles", "8", "--seed", "0"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
        assert len(objs) == 1
        meshes[name] = _read_obj(objs[0])
        line = re.search(r"^mouse: fit \d+ iterations?, \d+ of 4096 points paired, RMS \S+ -> \S+, largest move \S+ steps, total \S+ -> \S+, "
                         r"(kept|not kept: the decoder's vertices are written)$", r.stdout, flags=re.M)
        assert bool(line) == (name == "fit"), r.stdout[-2000:]
    (v0, f0), (v1, f1) = meshes["plain"], meshes["fit"]
    assert np.array_equal(f0, f1) and v0.shape == v1.shape
    assert np.linalg.norm(v1 - v0, axis=1).max() <= 2.0 / 128.0 + 1e-7          # (the OBJ holds 8 decimals)
