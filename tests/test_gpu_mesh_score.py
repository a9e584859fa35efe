"""Best-of-N sampling on the MI355X: the score kernels (csrc/mesh_score.hpp) against the float64 reference of tests/mesh_score_ref.py,
their bitwise reproducibility, the ranking of crafted candidates, `forward_detailed(..., num_candidates=4)` end to end on the tiny
configuration and `main.py --sampling --num_candidates 4`.  Every GPU step runs in a fresh interpreter under a time limit; the
comparisons run here.

Tolerance.  fp32 cannot do better than its own rounding, so the measure is the largest deviation, per cloud point and per face, of the
float32 numpy restatement of the kernel's arithmetic (`mesh_score_ref.score_f32`) from the float64 reference on the very inputs of
`mesh_score_ref.cases()`; the `refs` fixture computes it at run time and prints it.  The kernel may deviate from the float64
reference by at most 8 times that figure, per point, per face and in the two means (8: FMA contraction and the other summation
order).  Area: relative 1e-6; the face count: exact.
"""
# the figure as computed by the `refs` fixture on the cases below: 2.34e-07 (tolerance 1.87e-06), set by the far single points of "five_faces"; the
# 200- to 800-face soups alone give 8e-08 .. 1.3e-07
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_score_ref as R

pytestmark = pytest.mark.gpu

REPO = R.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import mesh_score_ref as R
from meshanything_amd import mesh_score
out = {{}}

def run(c, cl, n, s):
    cl = cl if torch.is_tensor(cl) else torch.from_numpy(cl)
    sc, t = mesh_score.score_meshes(torch.from_numpy(c).cuda(), cl.cuda(), n, s, return_terms=True)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), {{k: v.cpu().numpy() for k, v in t.items()}}
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
for name, (c, cl, n, s) in R.cases().items():
    sc, t = run(c, cl, n, s)
    out[name + "_scores"] = sc
    for k, v in t.items():
        out[name + "_" + k] = v
c, cl, n, s = R.cases()["groups"]
out["groups_again"] = run(c, cl, n, s)[0]
out["row7_alone"] = run(c[7:8], cl[1:2], 1, s)[0]
# a float16 cloud is the float32 cloud of the same values
half = torch.from_numpy(cl).half()
out["groups_f16"] = run(c, half, n, s)[0]
out["groups_f16_as_f32"] = run(c, half.float(), n, s)[0]
bad = cl.copy()
bad[1, 5, 2] = np.inf
try:
    run(c, bad, n, s)
    out["nonfinite_refused"] = np.array(False)
except ValueError:
    out["nonfinite_refused"] = np.array(True)
c, cl = R.ranking()
sc = run(c, cl, 4, 2.0)[0]
chosen, total = mesh_score.select(torch.from_numpy(sc), 4)
out["rank_scores"], out["rank_chosen"], out["rank_total"] = sc, chosen.numpy(), total.numpy()
"""
    return _gpu(tmp_path_factory.mktemp("score_kernels"), body)


@pytest.fixture(scope="module")
def refs():
    """name -> the float64 reference of every case, computed once; and the tolerance derived from the fp32 restatement on them"""
    ref, figure = {}, 0.0
    for name, (c, cl, n, s) in R.cases().items():
        ref[name] = R.batch(R.score_ref, c, cl, n, s)
        f32 = R.batch(R.score_f32, c, cl, n, s)
        for k in ("pt_dist", "face_nn"):
            a, b = ref[name][k], f32[k]
            assert np.array_equal(np.isfinite(a), np.isfinite(b))
            fin = np.isfinite(a)
            if fin.any():
                figure = max(figure, float(np.abs(a[fin] - b[fin]).max()))
    print(f"largest per-point deviation of the fp32 restatement from the fp64 reference: {figure:.3g}; tolerance {8 * figure:.3g}")
    assert 0 < figure < 1e-6
    return ref, 8 * figure


def _close(got, want, tol):
    """finite where the reference is, within tol there; the same infinities elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin]) and (not fin.any() or float(np.abs(got[fin] - want[fin]).max()) <= tol)


@pytest.mark.parametrize("name", list(R.cases()))
def test_kernel_matches_the_fp64_reference(kernels, refs, name):
    ref, tol = refs
    want = ref[name]
    sc = kernels[name + "_scores"]
    assert sc.dtype == np.float32 and sc.shape == want["scores"].shape and not np.isnan(sc).any()
    with np.errstate(invalid="ignore"):                              # inf - inf where both are +inf
        err = {k: float(np.abs(np.where(np.isfinite(want[k]), kernels[name + "_" + k] - want[k], 0)).max()) for k in ("pt_dist", "face_nn")}
        err["means"] = float(np.abs(np.where(np.isfinite(want["scores"][:, :2]), sc[:, :2] - want["scores"][:, :2], 0)).max())
    print(f"{name}: per point {err['pt_dist']:.3g}, per face {err['face_nn']:.3g}, means {err['means']:.3g}, tolerance {tol:.3g}")
    assert _close(kernels[name + "_pt_dist"], want["pt_dist"], tol)                      # per cloud point
    assert _close(kernels[name + "_face_nn"], want["face_nn"], tol)                      # per face: the mean over its 7 quadrature points
    assert np.array_equal(kernels[name + "_face_area"] < 0, want["face_area"] < 0)       # the same faces are invalid
    assert _close(sc[:, 0], want["scores"][:, 0], tol) and _close(sc[:, 1], want["scores"][:, 1], tol)
    assert np.abs(sc[:, 2] - want["scores"][:, 2]).max() <= 1e-6 * np.abs(want["scores"][:, 2]).max()
    assert np.array_equal(sc[:, 3], want["scores"][:, 3])


def test_edge_cases(kernels):
    sc = kernels["degenerate_scores"]
    assert np.isposinf(sc[0, 0]) and np.isposinf(sc[0, 1]) and sc[0, 2] == 0 and sc[0, 3] == 0       # all NaN
    assert np.isfinite(sc[1, 0]) and np.isposinf(sc[1, 1]) and sc[1, 2] == 0 and sc[1, 3] == 3         # zero-area faces only
    assert np.isfinite(sc[2]).all() and sc[2, 3] == 5
    cube = kernels["cube_scores"][0]
    assert cube[0] == 0.0 and cube[2] == 13.5 and cube[3] == 12                               # its own surface cloud, on the 1/128 grid: exact
    on_plane = kernels["voronoi_pt_dist"][0, 1]
    assert on_plane == 0.0
    assert bool(kernels["nonfinite_refused"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_nan_rows_between_valid_faces_change_no_bit(kernels):
    assert np.array_equal(_bits(kernels["nan_interleaved_scores"]), _bits(kernels["nan_compacted_scores"]))
    assert np.array_equal(_bits(kernels["nan_interleaved_pt_dist"]), _bits(kernels["nan_compacted_pt_dist"]))
    assert 300 < kernels["nan_compacted_scores"][0, 3] < 800


def test_scores_are_bitwise_reproducible_and_independent_of_the_batch(kernels):
    assert np.array_equal(_bits(kernels["groups_scores"]), _bits(kernels["groups_again"]))
    assert np.array_equal(_bits(kernels["groups_scores"][7:8]), _bits(kernels["row7_alone"]))          # row 7 of 12 = scored alone
    assert np.array_equal(_bits(kernels["groups_f16"]), _bits(kernels["groups_f16_as_f32"]))


def test_ranking_of_crafted_candidates(kernels, refs):
    """The cube's cloud against the cube, the cube shifted by 0.1, the cube with half its faces NaN, the cube scaled by 0.5."""
    _, tol = refs
    c, cl = R.ranking()
    ref = R.batch(R.score_ref, c, cl, 4)["scores"]
    total = np.sort(0.5 * (ref[:, 0] + ref[:, 1]))
    assert np.argmin(0.5 * (ref[:, 0] + ref[:, 1])) == 0
    assert total[1] - total[0] >= 100 * tol                        # on the reference: the decision is far above the kernel's error
    assert kernels["rank_chosen"].tolist() == [0]
    assert _close(kernels["rank_total"][0], 0.5 * (ref[:, 0] + ref[:, 1]), tol)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
_E2E = """
import types
from meshanything_amd.config import MAConfig, DTYPE_BF16, DTYPE_F32
from meshanything_amd.checkpoint import synthetic_state_dict
from meshanything_amd.data import normalize_pc
from meshanything_amd.model import MeshAnything

def clouds(cfg, seeds):
    rows = []
    for s in seeds:
        g = torch.Generator().manual_seed(s)
        d = torch.randn(cfg.n_points, 3, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        r = 0.3 + 0.7 * torch.rand(cfg.n_points, 1, generator=g)
        rows.append(normalize_pc(torch.cat([d * r, d], dim=-1).numpy().astype(np.float32)))
    return torch.from_numpy(np.stack(rows))

def message(fn):
    try:
        fn()
    except ValueError as e:
        return str(e)
    return ""

for tag, dt in (("bf16", DTYPE_BF16), ("fp32", DTYPE_F32)):
    cfg = MAConfig.tiny(dtype=dt, max_batch=8)
    args = types.SimpleNamespace(llm="facebook/opt-350m", codebook_size=cfg.codebook_size, codebook_dim=cfg.codebook_dim,
                                 n_max_triangles=cfg.n_max_faces, ma_config=cfg)
    m = MeshAnything(args)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, include_unused=True).items()}, strict=True)
    pc = clouds(cfg, [23, 24]).cuda()
    d = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11)
    d2 = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11)
    cand = d["candidates"]
    out[tag + "_pc"] = pc.cpu().numpy()
    for k in ("coords", "candidates", "scores", "chosen", "total", "tokens"):
        out[tag + "_" + k] = d[k].cpu().numpy()
        out[tag + "_again_" + k] = d2[k].cpu().numpy()
    out[tag + "_lengths"] = np.asarray(d["lengths"])
    out[tag + "_alone"] = mesh_score.score_meshes(cand.reshape(8, *cand.shape[2:]).contiguous(), pc, 4).cpu().numpy()
    out[tag + "_forward"] = m(pc, sampling=True, num_candidates=4, seed=11).cpu().numpy()
    out[tag + "_one"] = m.forward_detailed(pc, sampling=True, seed=11, num_candidates=1)["coords"].cpu().numpy()
    out[tag + "_plain"] = m.forward_detailed(pc, sampling=True, seed=11)["coords"].cpu().numpy()
    out[tag + "_too_many"] = np.array(message(lambda: m(clouds(cfg, [1, 2, 3]).cuda(), sampling=True, num_candidates=4)))
    out[tag + "_greedy"] = np.array(message(lambda: m(pc, sampling=False, num_candidates=4)))
    m.engine.close()
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("score_e2e"), _E2E)


def _same(a, b):
    """bitwise, NaN rows included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tag", ["bf16", "fp32"])
def test_forward_returns_the_best_of_four_candidates(e2e, tag):
    g = lambda k: e2e[tag + "_" + k]                                # noqa: E731
    cand, chosen, scores, pc = g("candidates"), g("chosen"), g("scores"), g("pc")
    G, N, F = 2, 4, 8
    assert cand.shape == (G, N, F, 3, 3) and scores.shape == (G, N, 4) and chosen.shape == (G,) and chosen.dtype == np.int64
    assert g("coords").shape == (G, F, 3, 3) and g("tokens").shape[0] == G * N and g("lengths").shape == (G * N,)
    for i in range(G):
        assert _same(g("coords")[i], cand[i, chosen[i]])
    assert _same(g("forward"), g("coords"))
    assert _same(scores.reshape(G * N, 4), g("alone"))             # the scores are those of a stand-alone call on the returned candidates
    assert not np.isnan(scores).any()
    # against the float64 reference: the chosen candidate is the best of its group, within the tolerance worked out for these inputs
    flat = cand.reshape(G * N, F, 3, 3)
    cloud = pc.astype(np.float32)
    ref = R.batch(R.score_ref, flat, cloud, N)
    f32 = R.batch(R.score_f32, flat, cloud, N)
    figure = 0.0
    for k in ("pt_dist", "face_nn"):
        fin = np.isfinite(ref[k])
        if fin.any():
            figure = max(figure, float(np.abs(ref[k][fin] - f32[k][fin]).max()))
    tol = 8 * figure
    total = (0.5 * (ref["scores"][:, 0] + ref["scores"][:, 1])).reshape(G, N)
    print(f"{tag}: chosen {chosen.tolist()}, reference totals {total.tolist()}, kernel totals {g('total').tolist()}, tolerance {tol:.3g}")
    for i in range(G):
        assert total[i, chosen[i]] <= total[i].min() + tol
    # the same seed twice: the same everything
    for k in ("coords", "candidates", "scores", "chosen", "tokens"):
        assert _same(g(k), g("again_" + k)), k
    # the rows of a group come from different sampler streams
    for i in range(G):
        assert any(not _same(cand[i, 0], cand[i, j]) for j in range(1, N))
    # one candidate is today's path
    assert _same(g("one"), g("plain"))
    assert "batchsize_per_gpu" in str(g("too_many")) and "num_candidates" in str(g("too_many"))
    assert "sampling" in str(g("greedy"))


def test_cli_num_candidates_writes_one_obj(tmp_path):
    """`python main.py --input_path mouse.npy --input_type pc_normal --sampling --num_candidates 4 ...` end to end (350M shape, seeded
    synthetic checkpoint, 8-face cap): one OBJ, and one line with the chosen index and the four totals."""
    import re
    g = np.load(os.path.join(REPO, "tests", "golden", "dataset.npz"))
    src = tmp_path / "mouse.npy"
    np.save(src, g["mouse_raw"])
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_normal", "--out_dir", str(out),
                        "--synthetic_weights", "--sampling", "--num_candidates", "4", "--n_max_triangles", "8", "--seed", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "mouse_gen.obj"
    m = re.search(r"^mouse: candidate (\d) of 4 chosen, totals ((?:\S+ ?){4})$", r.stdout, flags=re.M)
    assert m, r.stdout[-2000:]
    totals = [float(t) for t in m.group(2).split()]
    assert len(totals) == 4 and 0 <= int(m.group(1)) < 4
    assert totals[int(m.group(1))] == min(totals)
    assert "Generation Start!!!" in r.stdout and "Over!!" in r.stdout
