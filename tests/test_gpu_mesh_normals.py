"""Normal agreement between candidate meshes and their cloud on the MI355X (csrc/mesh_normals.hpp): the nearest
indices against the float32 restatement of tests/mesh_normals_ref.py, the values against its float64 restatement, bitwise
reproducibility, the edge cases, the ranking with the normal term, the orientation of faces, `forward_detailed(..., normal_weight=w,
orient="cloud")` end to end on the tiny configuration and `main.py --normal_weight 0.1 --orient cloud`.  Every GPU step runs in a fresh
interpreter under a time limit; the comparisons run here.

Tolerance.  Measured, not chosen: the `refs` fixture computes the largest deviation, per face (a_f, u_f) and in NC and the flipped
share, of the float32 restatement from the float64 one evaluated on the same nearest indices, on the inputs of
`mesh_normals_ref.cases()` (the overflow case apart), and prints it.  The kernel may deviate from the float64 restatement by at most 8
times that figure (8: the margin DESIGN.md section 9 uses for the distances; it bounds a reordering or contraction inside one fp32
expression).  The flipped share compares only because every sign is decided far above that: the fixture asserts that the smallest
|a_f| of a measurable face is at least 10 tolerances.
"""
# the figure as computed by the `refs` fixture on the cases below: 1.93e-07 (tolerance 1.54e-06); the smallest |a_f|: 1.73e-04
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_normals_ref as N
import mesh_score_ref as S

pytestmark = pytest.mark.gpu

REPO = N.REPO
TESTS = os.path.dirname(os.path.abspath(__file__))

_PRELUDE = f"""
import sys
sys.path[:0] = [{REPO!r}, {TESTS!r}]
import numpy as np
import torch
import mesh_normals_ref as N
import mesh_score_ref as S
from meshanything_amd import mesh_score
out = {{}}

def run(c, cl, n=1, s=2.0):
    c = c if torch.is_tensor(c) else torch.from_numpy(c)
    cl = cl if torch.is_tensor(cl) else torch.from_numpy(cl)
    ns, fa, t = mesh_score.normal_agreement(c.cuda(), cl.cuda(), n, s, return_terms=True)
    torch.cuda.synchronize()
    r = {{k: v.cpu().numpy() for k, v in t.items()}}
    r["nscores"], r["face_agree"] = ns.cpu().numpy(), fa.cpu().numpy()
    return r

def put(name, r):
    for k, v in r.items():
        out[name + "_" + k] = v
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
cases = N.cases()
for name, (c, cl, n, s) in cases.items():
    put(name, run(c, cl, n, s))
c, cl, n, s = cases["batch_6_3"]
put("again", run(c, cl, n, s))
for row in range(6):
    put(f"row{row}_alone", run(c[row:row + 1], cl[row // n:row // n + 1], 1, s))
bad = cl.copy()
bad[1, 5, 4] = np.nan                                        # a normal, not a coordinate
refused = {}
for key, fn in (("nonfinite", lambda: run(c, bad, n, s)), ("no_normals", lambda: run(c, cl[:, :, :3].copy(), n, s))):
    try:
        fn()
        refused[key] = False
    except ValueError:
        refused[key] = True
    out["refused_" + key] = np.array(refused[key])
# the same faces through the score op: the area of a measurable face is the score kernel's
sc, t = mesh_score.score_meshes(torch.from_numpy(cases["soup_800"][0]).cuda(), torch.from_numpy(cases["soup_800"][1]).cuda(), 1, 2.0, return_terms=True)
out["soup_800_score_area"] = t["face_area"].cpu().numpy()
# ranking: the flat mesh against the accordion, the weight derived from the float64 restatement
c, cl = N.ranking()
sc = mesh_score.score_meshes(torch.from_numpy(c).cuda(), torch.from_numpy(cl).cuda(), 2).cpu()
r = run(c, cl, 2)
ref_d = S.batch(S.score_ref, c, cl, 2)["scores"]
ref_n = N.batch(N.agree_f64, c, cl, 2)["nscores"]
tot = 0.5 * (ref_d[:, 0] + ref_d[:, 1])
w = 2.0 * (tot[0] - tot[1]) / (ref_n[0, 0] - ref_n[1, 0])
ch0, t0 = mesh_score.select(sc, 2)
ch1, t1 = mesh_score.select(sc, 2, torch.from_numpy(r["nscores"]), w)
out["rank_scores"], out["rank_nscores"], out["rank_w"] = sc.numpy(), r["nscores"], np.array(w)
out["rank_chosen0"], out["rank_chosen1"], out["rank_total0"], out["rank_total1"] = ch0.numpy(), ch1.numpy(), t0.numpy(), t1.numpy()
# orientation: flipped cube and open box
c, cl = N.orientation()
r = run(c, cl, 2)
fixed = mesh_score.orient_faces(torch.from_numpy(c).cuda(), torch.from_numpy(r["face_agree"]).cuda())
put("orient", r)
out["orient_fixed"] = fixed.cpu().numpy()
put("orient_after", run(fixed, cl, 2))
"""
    return _gpu(tmp_path_factory.mktemp("normals_kernels"), body)


@pytest.fixture(scope="module")
def refs():
    """name -> (float32 restatement, float64 restatement on the float32 indices) of every case, computed once; and the tolerance"""
    ref, figure, smallest = {}, 0.0, np.inf
    for name, (c, cl, n, s) in N.cases().items():
        f32 = N.batch(N.agree_f32, c, cl, n, s)
        f64 = N.batch(N.agree_f64, c, cl, n, s, idx=f32["nn_idx"])
        ref[name] = (f32, f64)
        if name == "degenerate":                                  # overflow: fp64 does not overflow where fp32 does; checked on its own
            continue
        for k in ("face_agree", "face_abs"):
            figure = max(figure, float(np.abs(f32[k] - f64[k]).max()))
        figure = max(figure, float(np.abs(f32["nscores"][:, :2] - f64["nscores"][:, :2]).max()))
        meas = np.stack([N.agree_measurable(x, s) for x in c])
        smallest = min(smallest, float(np.abs(f64["face_agree"][meas]).min()))
    tol = 8 * figure
    print(f"largest deviation of the fp32 restatement from the fp64 one: {figure:.3g}; tolerance {tol:.3g}; smallest |a_f| {smallest:.3g}")
    assert 0 < figure < 1e-6
    assert smallest >= 10 * tol                                   # every sign, hence the flipped share, is decided
    return ref, tol


@pytest.mark.parametrize("name", list(N.cases()))
def test_nearest_indices_equal_the_fp32_restatement(kernels, refs, name):
    want = refs[0][name][0]["nn_idx"]
    got = kernels[name + "_nn_idx"]
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} indices differ"
    P = N.cases()[name][1].shape[1]
    assert ((got >= -1) & (got < P)).all()


def test_ties_are_decided_by_the_lowest_index(kernels, refs):
    c, cl, _, s = N.cases()["cube"]
    share = N.tie_share(c[0], cl[0], s)
    print(f"cube against its cloud: {share:.1%} of the queries have an exact tie")
    assert share > 0.05                                            # the case does test the tie-break (nn_idx equality: the test above)
    idx = kernels["tripled_nn_idx"]
    assert idx.min() >= 0 and idx.max() < 400                      # of three coincident points the first copy wins, in every LDS tile
    cloud = N.cases()["tripled"][1][0]
    assert not np.array_equal(cloud[:400, 3:], cloud[400:800, 3:]) and np.array_equal(cloud[:400, :3], cloud[800:, :3])


@pytest.mark.parametrize("name", [n for n in N.cases() if n != "degenerate"])
def test_values_match_the_fp64_restatement(kernels, refs, name):
    ref, tol = refs
    f32, f64 = ref[name]
    err = {k: float(np.abs(kernels[name + "_" + k] - f64[k]).max()) for k in ("face_agree", "face_abs")}
    ns = kernels[name + "_nscores"]
    err["NC"] = float(np.abs(ns[:, 0] - f64["nscores"][:, 0]).max())
    err["flipped"] = float(np.abs(ns[:, 1] - f64["nscores"][:, 1]).max())
    print(f"{name}: " + ", ".join(f"{k} {v:.3g}" for k, v in err.items()) + f", tolerance {tol:.3g}")
    assert ns.dtype == np.float32 and np.isfinite(ns).all()
    assert all(v <= tol for v in err.values()), err
    assert np.array_equal(kernels[name + "_face_area"] < 0, f64["face_area"] < 0)      # the same faces are invalid
    assert np.abs(kernels[name + "_face_area"] - f64["face_area"]).max() <= 1e-6 * max(1.0, np.abs(f64["face_area"]).max())
    assert np.abs(ns[:, 2] - f64["nscores"][:, 2]).max() <= 1e-6 * np.abs(f64["nscores"][:, 2]).max()
    assert np.array_equal(ns[:, 3], f64["nscores"][:, 3])


@pytest.mark.parametrize("name", list(N.NAMED))
def test_fp64_argmin_equals_the_kernels_indices(kernels, name):
    """On these three inputs fp32 resolves every nearest point: no query left out."""
    c, cl, n, s = N.cases()[name]
    want = N.batch(N.agree_f64, c, cl, n, s)["nn_idx"]
    assert np.array_equal(kernels[name + "_nn_idx"], want)
    assert want.size == 7 * c.shape[1] and (want >= 0).all()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bitwise_reproducible_and_independent_of_the_batch(kernels):
    for k in ("nscores", "face_agree", "face_abs", "face_area"):
        assert np.array_equal(_bits(kernels["batch_6_3_" + k]), _bits(kernels["again_" + k])), k
        for row in range(6):                                        # every row of the batch = that candidate scored alone
            assert np.array_equal(_bits(kernels["batch_6_3_" + k][row:row + 1]), _bits(kernels[f"row{row}_alone_" + k])), (k, row)
    for row in range(6):
        assert np.array_equal(kernels["batch_6_3_nn_idx"][row:row + 1], kernels[f"row{row}_alone_nn_idx"]), row
    # the two groups of batch_6_3 were scored against different clouds
    assert not np.array_equal(kernels["batch_6_3_nscores"][0], kernels["batch_6_3_nscores"][3])


def test_nan_rows_between_valid_faces_change_no_bit_of_the_scores(kernels):
    assert np.array_equal(_bits(kernels["nan_interleaved_nscores"]), _bits(kernels["nan_compacted_nscores"]))
    keep = S.valid_rows(N.cases()["nan_interleaved"][0][0])
    assert np.array_equal(_bits(kernels["nan_interleaved_face_agree"][0][keep]), _bits(kernels["nan_compacted_face_agree"][0]))
    assert 50 < kernels["nan_compacted_nscores"][0, 3] < 130


def test_area_is_the_score_kernels(kernels):
    """The same expression, 0.5 * sqrtf(n . n), in two kernels, this one compiled without FMA contraction and the score kernel with the
    default.  On these lattice inputs n is exact (products of multiples of 1/64 below 2 fit 24 bits), so the two can differ only in how
    the three squares of n . n are rounded or fused: at most 3 roundings of 2^-24 each way in
    l2, halved by the root, plus the root's own: within 4 float32 epsilons."""
    a, b = kernels["soup_800_face_area"].astype(np.float64), kernels["soup_800_score_area"].astype(np.float64)
    print(f"largest relative difference of the two kernels' areas: {float((np.abs(a - b) / b).max()):.3g}")
    assert (b > 0).all() and (np.abs(a - b) <= 4 * np.finfo(np.float32).eps * b).all()


def test_edge_cases(kernels, refs):
    f32 = refs[0]["degenerate"][0]
    for k in ("nscores", "face_agree", "face_abs", "face_area"):
        assert np.isfinite(kernels["degenerate_" + k]).all(), k              # no NaN, no infinity, coordinates near FLT_MAX included
    idx = kernels["degenerate_nn_idx"]
    assert ((idx >= -1) & (idx < 67)).all() and np.array_equal(idx, f32["nn_idx"])
    coords = N.cases()["degenerate"][0]
    valid = np.stack([S.valid_rows(c) for c in coords])
    assert np.array_equal(idx[..., 0] == -1, ~valid) and np.array_equal(kernels["degenerate_face_area"] == -1, ~valid)
    ns = kernels["degenerate_nscores"]
    assert ns[0].tolist() == [0, 0, 0, 0]                                     # all NaN
    assert ns[1].tolist() == [0, 0, 0, 3]                                     # zero-area faces only
    assert ns[2, 3] == 5 and ns[2, 2] > 0 and 0 < ns[2, 0] <= 1 and 0 <= ns[2, 1] <= 1
    assert ns[3].tolist() == [0, 0, 0, 4]                                     # near FLT_MAX: every normal overflows, nothing is measurable
    meas = np.stack([N.agree_measurable(c) for c in coords])
    assert meas[2].sum() == 3 and not meas[[0, 1, 3]].any()
    for k in ("face_agree", "face_abs"):
        assert (kernels["degenerate_" + k][~meas] == 0).all()
    assert bool(kernels["refused_nonfinite"]) and bool(kernels["refused_no_normals"])


def test_ranking_with_the_normal_term(kernels, refs):
    """A flat cloud with normals +z; the flat mesh lifted by DELTA against an accordion that is closer but folded by 45 degrees."""
    _, tol = refs
    tol_d = 1.87e-6                                                 # the distances' tolerance (test_gpu_mesh_score.py)
    c, cl = N.ranking()
    ref_d = S.batch(S.score_ref, c, cl, 2)["scores"]
    ref_n = N.batch(N.agree_f64, c, cl, 2)["nscores"]
    tot = 0.5 * (ref_d[:, 0] + ref_d[:, 1])
    w = float(kernels["rank_w"])
    print(f"distance totals {tot.tolist()}, NC {ref_n[:, 0].tolist()}, weight {w:.4f}")
    assert tot[0] - tot[1] >= 100 * tol_d                          # the accordion is closer ...
    assert ref_n[0, 0] - ref_n[1, 0] >= 100 * tol                  # ... and less consistent, both far above the kernels' error
    assert w == 2.0 * (tot[0] - tot[1]) / (ref_n[0, 0] - ref_n[1, 0])
    with_n = tot + w * (1.0 - ref_n[:, 0])
    assert with_n[1] - with_n[0] >= 100 * (tol_d + w * tol)
    assert kernels["rank_chosen0"].tolist() == [1] and kernels["rank_chosen1"].tolist() == [0]
    assert np.abs(kernels["rank_total0"][0] - tot).max() <= tol_d
    assert np.abs(kernels["rank_total1"][0] - with_n).max() <= tol_d + w * tol
    assert np.abs(kernels["rank_nscores"][:, 0] - ref_n[:, 0]).max() <= tol


def test_orientation_by_the_cloud(kernels):
    c, _ = N.orientation()
    assert (N.outward(S.cube()) == 1).all() and (N.outward(c[0]) == -1).sum() == 6      # the inputs are what they claim
    share = kernels["orient_nscores"][:, 1]
    assert 0.3 < share[0] < 0.7 and 0.2 < share[1] < 0.8
    fixed = kernels["orient_fixed"]
    assert (N.outward(fixed[0]) == 1).all() and len(N.outward(fixed[0])) == 12
    assert (N.outward(fixed[1]) == 1).all() and len(N.outward(fixed[1])) == 10          # the open box: its NaN rows stay
    assert np.isnan(fixed[1, 2:4]).all()
    flipped = kernels["orient_face_agree"] < 0
    assert np.array_equal(fixed[flipped], c[flipped][:, [0, 2, 1]]) and np.array_equal(fixed[~flipped], c[~flipped], equal_nan=True)
    assert (kernels["orient_after_nscores"][:, 1] == 0).all() and (kernels["orient_after_face_agree"] >= 0).all()
    assert np.array_equal(kernels["orient_after_nscores"][:, 0], kernels["orient_nscores"][:, 0]) or \
        np.abs(kernels["orient_after_nscores"][:, 0] - kernels["orient_nscores"][:, 0]).max() < 1e-6   # NC does not depend on the winding


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

W = 0.1
for tag, dt in (("bf16", DTYPE_BF16), ("fp32", DTYPE_F32)):
    cfg = MAConfig.tiny(dtype=dt, max_batch=8)
    args = types.SimpleNamespace(llm="facebook/opt-350m", codebook_size=cfg.codebook_size, codebook_dim=cfg.codebook_dim,
                                 n_max_triangles=cfg.n_max_faces, ma_config=cfg)
    m = MeshAnything(args)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, include_unused=True).items()}, strict=True)
    pc = clouds(cfg, [23, 24]).cuda()
    plain = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11)
    zero = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11, normal_weight=0, orient=None)
    full = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11, normal_weight=W, orient="cloud")
    out[tag + "_plain_keys"] = np.array(sorted(plain))
    out[tag + "_zero_keys"] = np.array(sorted(zero))
    for k in ("coords", "chosen", "total", "candidates", "scores"):
        out[tag + "_plain_" + k] = plain[k].cpu().numpy()
        out[tag + "_zero_" + k] = zero[k].cpu().numpy()
    for k in ("coords", "chosen", "total", "candidates", "scores", "normal_scores", "face_agree"):
        out[tag + "_full_" + k] = full[k].cpu().numpy()
    cand = full["candidates"]
    flat = cand.reshape(8, *cand.shape[2:]).contiguous()
    ns, fa = mesh_score.normal_agreement(flat, pc, 4)
    ch, tot = mesh_score.select(full["scores"].reshape(8, 4), 4, ns, W)
    out[tag + "_alone_nscores"], out[tag + "_alone_agree"] = ns.cpu().numpy(), fa.cpu().numpy()
    out[tag + "_select_chosen"], out[tag + "_select_total"] = ch.cpu().numpy(), tot.cpu().numpy()
    out[tag + "_forward"] = m(pc, sampling=True, num_candidates=4, seed=11, normal_weight=W, orient="cloud").cpu().numpy()
    # orientation alone: best-of-4 by distance, and a single candidate
    o4 = m.forward_detailed(pc, sampling=True, num_candidates=4, seed=11, orient="cloud")
    out[tag + "_o4_coords"], out[tag + "_o4_agree"], out[tag + "_o4_chosen"] = o4["coords"].cpu().numpy(), o4["face_agree"].cpu().numpy(), o4["chosen"].cpu().numpy()
    one = m.forward_detailed(pc, sampling=True, seed=11)
    one_o = m.forward_detailed(pc, sampling=True, seed=11, orient="cloud")
    out[tag + "_one"], out[tag + "_one_o"], out[tag + "_one_agree"] = one["coords"].cpu().numpy(), one_o["coords"].cpu().numpy(), one_o["face_agree"].cpu().numpy()
    out[tag + "_one_agree_alone"] = mesh_score.normal_agreement(one["coords"], pc, 1)[1].cpu().numpy()
    out[tag + "_weight_alone"] = np.array(message(lambda: m(pc, sampling=True, normal_weight=W)))
    out[tag + "_weight_negative"] = np.array(message(lambda: m(pc, sampling=True, num_candidates=4, normal_weight=-1.0)))
    out[tag + "_bad_orient"] = np.array(message(lambda: m(pc, sampling=True, orient="volume")))
    m.engine.close()
"""


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return _gpu(tmp_path_factory.mktemp("normals_e2e"), _E2E)


def _same(a, b):
    """bitwise, NaN rows included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _oriented(coords, agree):
    c = np.array(coords, copy=True)
    flip = agree < 0
    c[flip] = c[flip][:, [0, 2, 1]]
    return c


@pytest.mark.parametrize("tag", ["bf16", "fp32"])
def test_forward_with_normal_weight_and_orientation(e2e, tag):
    g = lambda k: e2e[tag + "_" + k]                                # noqa: E731
    G, n, F = 2, 4, 8
    # the defaults, spelled out, are today's call: bit for bit, and no new key
    for k in ("coords", "chosen", "total", "candidates", "scores"):
        assert _same(g("plain_" + k), g("zero_" + k)), k
    assert g("plain_keys").tolist() == g("zero_keys").tolist() and "normal_scores" not in g("plain_keys").tolist() and "face_agree" not in g("plain_keys").tolist()
    # with the weight: the same candidates and distance scores, the op's own numbers, and select's choice
    assert _same(g("full_candidates"), g("plain_candidates")) and _same(g("full_scores"), g("plain_scores"))
    ns = g("full_normal_scores")
    assert ns.shape == (G, n, 4) and np.isfinite(ns).all() and _same(ns.reshape(G * n, 4), g("alone_nscores"))
    assert (ns[..., 0] >= 0).all() and (ns[..., 0] <= 1.001).all()   # the cloud's normals are float16: unit within 5e-4
    chosen = g("full_chosen")
    assert chosen.tolist() == g("select_chosen").tolist() and _same(g("full_total"), g("select_total"))
    want_total = g("plain_total") + np.float32(0.1) * (np.float32(1.0) - ns[..., 0])
    fin = np.isfinite(want_total)                                   # a candidate without a valid face has a total of +inf
    assert np.array_equal(np.isfinite(g("full_total")), fin) and np.allclose(g("full_total")[fin], want_total[fin], rtol=0, atol=1e-6)
    for i in range(G):
        assert chosen[i] == int(np.argmin(np.nan_to_num(g("full_total")[i], nan=np.inf)))
        agree = g("alone_agree").reshape(G, n, F)[i, chosen[i]]
        assert _same(g("full_face_agree")[i], agree)
        assert _same(g("full_coords")[i], _oriented(g("full_candidates")[i, chosen[i]], agree))
    assert _same(g("forward"), g("full_coords"))
    # orientation alone keeps the distance ranking
    assert g("o4_chosen").tolist() == g("plain_chosen").tolist()
    for i in range(G):
        assert _same(g("o4_coords")[i], _oriented(g("plain_coords")[i], g("o4_agree")[i]))
    assert _same(g("one_o"), np.stack([_oriented(g("one")[i], g("one_agree")[i]) for i in range(G)])) and _same(g("one_agree"), g("one_agree_alone"))
    assert "num_candidates" in str(g("weight_alone")) and "normal_weight" in str(g("weight_negative")) and "orient" in str(g("bad_orient"))


def _read_obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                f.append([int(x) - 1 for x in p[1:4]])
    return np.array(v, np.float32), np.array(f, np.int64)


def test_cli_normal_weight_and_orient_cloud(tmp_path):
    """`python main.py ... --sampling --num_candidates 4 --normal_weight 0.1 --orient cloud` end to end (350M shape, seeded synthetic
    checkpoint, 8-face cap): one OBJ, the candidate line with the four NC values, and no written face wound against its cloud."""
    g = np.load(os.path.join(REPO, "tests", "golden", "dataset.npz"))
    src = tmp_path / "mouse.npy"
    np.save(src, g["mouse_raw"])
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--input_path", str(src), "--input_type", "pc_normal", "--out_dir", str(out),
                        "--synthetic_weights", "--sampling", "--num_candidates", "4", "--normal_weight", "0.1", "--orient", "cloud",
                        "--n_max_triangles", "8", "--seed", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    objs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith("_gen.obj")]
    assert len(objs) == 1 and os.path.basename(objs[0]) == "mouse_gen.obj"
    m = re.search(r"^mouse: candidate (\d) of 4 chosen, totals ((?:\S+ ){3}\S+), NC ((?:\S+ ){3}\S+)$", r.stdout, flags=re.M)
    assert m, r.stdout[-2000:]
    totals, ncs = [float(t) for t in m.group(2).split()], [float(t) for t in m.group(3).split()]
    assert totals[int(m.group(1))] == min(totals) and all(0 <= v <= 1.001 for v in ncs)
    verts, faces = _read_obj(objs[0])
    assert len(faces) >= 1
    np.save(tmp_path / "written.npy", verts[faces])
    body = f"""
from meshanything_amd.data import Dataset
np.random.seed(0)                                            # main.py seeds numpy before it builds the dataset
cloud = Dataset("pc_normal", [{str(src)!r}])[0]["pc_normal"]
put("obj", run(np.load({str(tmp_path / "written.npy")!r})[None], np.asarray(cloud)[None]))
"""
    back = _gpu(tmp_path, body)
    assert back["obj_face_agree"].shape == (1, len(faces)) and (back["obj_face_agree"] >= 0).all() and back["obj_nscores"][0, 1] == 0
