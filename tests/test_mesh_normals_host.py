"""Normal agreement without a GPU: the argument checks of ma_op_mesh_normals / ma_mesh_normals_workspace_bytes (they run before the first
HIP call), `mesh_score.select` with the normal term on hand-made tables, every refusal of `normal_agreement` that precedes a device
call, `orient_faces` on CPU tensors, the restatement of tests/mesh_normals_ref.py on inputs with a known answer, and main.py's flags."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import mesh_normals_ref as N
import mesh_score_ref as S

REPO = N.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build                           # noqa: E402
from meshanything_amd import mesh_score                            # noqa: E402

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


def _call(lib, B=4, F=8, cloud_ld=6, P=16, n=2, scale=2.0, ws_bytes=None, coords=1, cloud=1, agree=1, nscores=1, ws=1):
    """ma_op_mesh_normals with dummy non-null pointers: every case here is refused before anything is read or launched"""
    buf = (C.c_float * 4)()
    p = lambda on: C.addressof(buf) if on else None                  # noqa: E731
    nb = lib.ma_mesh_normals_workspace_bytes(B, F) if ws_bytes is None else ws_bytes
    return lib.ma_op_mesh_normals(p(coords), B, F, p(cloud), cloud_ld, P, n, scale, p(agree), p(nscores), p(ws), nb, None)


@pytest.mark.parametrize("kw,word", [
    (dict(coords=0), "null"), (dict(cloud=0), "null"), (dict(agree=0), "null"), (dict(nscores=0), "null"), (dict(ws=0), "null"),
    (dict(B=0, ws_bytes=1 << 20), "B >= 1"), (dict(F=0, ws_bytes=1 << 20), "F"), (dict(F=(1 << 20) + 1, ws_bytes=1 << 40), "F"),
    (dict(P=0), "P"), (dict(P=(1 << 20) + 1), "P"),
    (dict(n=0), "n_per_cloud"), (dict(n=3), "n_per_cloud"), (dict(n=-2), "n_per_cloud"),
    (dict(cloud_ld=3), "cloud_ld"), (dict(cloud_ld=4), "cloud_ld"), (dict(cloud_ld=0), "cloud_ld"),
    (dict(scale=0.0), "mesh_scale"), (dict(scale=-1.0), "mesh_scale"), (dict(scale=INF), "mesh_scale"), (dict(scale=float("nan")), "mesh_scale"),
    (dict(ws_bytes=0), "workspace"), (dict(ws_bytes=2 * 256 + 1024 - 1), "workspace"),
])
def test_bad_arguments_are_refused_without_a_gpu(lib, kw, word):
    assert _call(lib, **kw) == -1                                    # MA_ERR_INVALID
    msg = lib.ma_last_error(None).decode()
    assert msg.startswith("ma_op_mesh_normals:") and word in msg, msg


def test_workspace_bytes(lib):
    a256 = lambda b: (b + 255) & ~255                                # noqa: E731
    for B, F in [(1, 1), (4, 8), (12, 130), (64, 800), (1, 1 << 20)]:
        assert lib.ma_mesh_normals_workspace_bytes(B, F) == 2 * a256(B * F * 4) + a256(B * F * 28)
    for B, F in [(0, 8), (-1, 8), (1, 0), (1, (1 << 20) + 1)]:
        assert lib.ma_mesh_normals_workspace_bytes(B, F) == 0
    assert lib.ma_mesh_normals_workspace_bytes(65536, 1 << 20) == 36 * 65536 * (1 << 20)      # the size does not wrap


def test_symbols_are_declared_and_bound(lib):
    with open(os.path.join(REPO, "include", "meshanything_amd.h")) as f:
        header = f.read()
    for name, nargs in (("ma_op_mesh_normals", 13), ("ma_mesh_normals_workspace_bytes", 2)):
        assert f" {name}(" in header and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "no reference counterpart" in header[header.index("csrc/mesh_normals.hpp"):header.index("ma_op_mesh_normals(")].lower()


# ---- select ------------------------------------------------------------------------------------------------------------------------
def _table(rows):
    return torch.tensor([[a, b, 1.0, 5.0] for a, b in rows], dtype=torch.float32)


def _nc(values):
    return torch.tensor([[v, 0.0, 1.0, 5.0] for v in values], dtype=torch.float32)


def test_select_with_the_normal_term_by_hand():
    scores = _table([(0.25, 0.25), (0.125, 0.125), (0.5, 0.5), (INF, INF)])          # distance totals 0.25, 0.125, 0.5, inf
    nc = _nc([1.0, 0.5, 0.75, 1.0])
    chosen, total = mesh_score.select(scores, 4)
    assert chosen.tolist() == [1] and total.tolist() == [[0.25, 0.125, 0.5, INF]]
    chosen, total = mesh_score.select(scores, 4, nc, 0.5)                               # + 0.5 * (0, 0.5, 0.25, 0)
    assert chosen.tolist() == [0] and total.tolist() == [[0.25, 0.375, 0.625, INF]]
    chosen, total = mesh_score.select(scores, 4, nc, 0.25)                              # 0.25 against 0.125 + 0.125: a tie, the lowest index
    assert chosen.tolist() == [0] and total.tolist() == [[0.25, 0.25, 0.5625, INF]]
    chosen, total = mesh_score.select(scores, 2, nc, 0.5)                               # two groups of two
    assert chosen.tolist() == [0, 0] and total.tolist() == [[0.25, 0.375], [0.625, INF]]
    # +inf still loses, whatever its NC; a group that is all +inf gives index 0
    chosen, _ = mesh_score.select(_table([(INF, INF), (3.0, 3.0)]), 2, _nc([1.0, 0.0]), 100.0)
    assert chosen.tolist() == [1]
    chosen, total = mesh_score.select(_table([(INF, INF), (INF, 1.0)]), 2, _nc([0.0, 1.0]), 1.0)
    assert chosen.tolist() == [0] and torch.isinf(total).all()
    # a weight of 0 ignores the normal scores, given or not
    assert mesh_score.select(scores, 4, nc, 0.0)[0].tolist() == [1] and torch.equal(mesh_score.select(scores, 4, nc, 0.0)[1], mesh_score.select(scores, 4)[1])


def test_select_default_path_is_unchanged():
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 4, 8):
        s = torch.rand(6 * n, 4, generator=g)
        s[torch.rand(6 * n, generator=g) < 0.2, :2] = INF
        chosen, total = mesh_score.select(s, n)
        want = (0.5 * (s[:, 0] + s[:, 1])).reshape(-1, n)                                 # the definition before the normal term existed
        assert total.dtype == torch.float32 and total.numpy().tobytes() == want.numpy().tobytes()
        assert chosen.dtype == torch.int64 and chosen.tolist() == [int(np.argmin(r)) for r in want.numpy()]
        c0, t0 = mesh_score.select(s, n, None, 0.0)
        assert torch.equal(c0, chosen) and t0.numpy().tobytes() == want.numpy().tobytes()


def test_select_refusals():
    s, nc = _table([(1.0, 1.0), (2.0, 2.0)]), _nc([1.0, 1.0])
    with pytest.raises(ValueError, match="normal_weight"):
        mesh_score.select(s, 2, nc, -0.5)
    with pytest.raises(ValueError, match="normal_weight"):
        mesh_score.select(s, 2, nc, float("nan"))
    with pytest.raises(ValueError, match="normal_scores"):
        mesh_score.select(s, 2, None, 0.5)
    with pytest.raises(ValueError, match="normal_scores"):
        mesh_score.select(s, 2, nc[:1], 0.5)


# ---- normal_agreement: what is refused before a device call ---------------------------------------------------------------------
def test_normal_agreement_refusals_without_a_gpu():
    c = torch.from_numpy(np.stack([S.soup(8, 1), S.soup(8, 2)]))
    cl = torch.from_numpy(S.points(16, 3, 6))[None]
    with pytest.raises(ValueError, match="CUDA"):
        mesh_score.normal_agreement(c, cl, 2)                                            # CPU tensors: no fallback
    with pytest.raises(ValueError, match=r"\(G, P, 6\)"):
        mesh_score.normal_agreement(c, cl[:, :, :3], 2)                                  # no normal columns
    for col in (1, 4):                                                                  # a coordinate, a normal
        bad = cl.clone()
        bad[0, 7, col] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            mesh_score.normal_agreement(c, bad, 2)
        bad[0, 7, col] = INF
        with pytest.raises(ValueError, match="non-finite"):
            mesh_score.normal_agreement(c, bad, 2)
    with pytest.raises(ValueError, match="n_per_cloud"):
        mesh_score.normal_agreement(c, cl, 1)
    with pytest.raises(ValueError, match="mesh_scale"):
        mesh_score.normal_agreement(c, cl, 2, mesh_scale=0.0)
    with pytest.raises(ValueError, match="coords"):
        mesh_score.normal_agreement(c[:, :, :2], cl, 2)
    with pytest.raises(ValueError, match="float16 or float32"):
        mesh_score.normal_agreement(c, cl.double(), 2)


# ---- orient_faces ----------------------------------------------------------------------------------------------------------------
def test_orient_faces_on_cpu_tensors():
    c = torch.arange(2 * 5 * 9, dtype=torch.float32).reshape(2, 5, 3, 3)
    c[0, 1] = float("nan")
    c[1, 4] = float("nan")
    a = torch.tensor([[-0.5, -1.0, 0.0, 0.25, -1e-30], [0.0, 1.0, -0.0, -0.125, -2.0]])
    out = mesh_score.orient_faces(c, a)
    assert out.data_ptr() != c.data_ptr() and out.shape == c.shape and out.dtype == c.dtype and out.device.type == "cpu"
    for b in range(2):
        for f in range(5):
            want = c[b, f][[0, 2, 1]] if a[b, f] < 0 else c[b, f]
            assert out[b, f].numpy().tobytes() == want.numpy().tobytes(), (b, f)        # NaN rows included: bitwise
    assert torch.isnan(out[0, 1]).all() and torch.isnan(out[1, 4]).all()
    assert c[0, 0, 1, 0] == 3.0                                                           # the input is untouched
    # one mesh without a batch dimension, numpy agreement
    one = mesh_score.orient_faces(c[0], a[0].numpy())
    assert torch.equal(torch.nan_to_num(one, nan=-1.0), torch.nan_to_num(out[0], nan=-1.0))
    # a flipped face has the opposite normal
    tri = torch.tensor(S.cube())
    flipped = mesh_score.orient_faces(tri, -torch.ones(12))
    assert (N.outward(tri.numpy()) == 1).all() and (N.outward(flipped.numpy()) == -1).all()
    with pytest.raises(ValueError):
        mesh_score.orient_faces(c, a[:, :4])
    with pytest.raises(ValueError):
        mesh_score.orient_faces(c.reshape(2, 5, 9), a)


# ---- the restatement itself, on inputs with a known answer --------------------------------------------------------------------
def test_restatement_on_known_answers():
    """A check of the reference, not of the new code: it runs tests/mesh_normals_ref.py alone (so, unlike the other tests of this file, it
    would pass wherever that module exists), to make sure that what the GPU tests compare the kernel against has the known answers."""
    # one face in the plane z = 0.25 (cloud units), wound to +z, against a cloud whose normals are (0, 0, 1) / (0, 0.6, 0.8) by index parity
    tri = np.array([[[0.0, 0.0, 0.125], [0.25, 0.0, 0.125], [0.0, 0.25, 0.125]]], np.float32)
    cl = np.zeros((2, 6), np.float32)
    cl[0] = [-5, -5, 0, 0, 0, 1]                                     # far: never the nearest
    cl[1] = [0.1, 0.1, 0, 0, 0.6, 0.8]
    for fn in (N.agree_f32, N.agree_f64):
        r = fn(tri, cl)
        assert r["nn_idx"].tolist() == [[1] * 7]
        assert abs(r["face_agree"][0] - 0.8) < 1e-6 and abs(r["face_abs"][0] - 0.8) < 1e-6 and abs(r["face_area"][0] - 0.125) < 1e-7
        assert np.allclose(r["nscores"], [0.8, 0.0, 0.125, 1.0], atol=1e-6)
        r = fn(N.swap12(tri, [0]), cl)
        assert abs(r["face_agree"][0] + 0.8) < 1e-6 and abs(r["face_abs"][0] - 0.8) < 1e-6 and np.allclose(r["nscores"], [0.8, 1.0, 0.125, 1.0], atol=1e-6)
    # coincident points: the lowest index; NaN rows: -1 and nothing added
    cl2 = np.concatenate([cl[1:], cl[1:], cl])
    assert N.agree_f32(tri, cl2)["nn_idx"].tolist() == [[0] * 7]
    both = np.concatenate([np.full((1, 3, 3), np.nan, np.float32), tri])
    r = N.agree_f32(both, cl)
    assert r["nn_idx"][0].tolist() == [-1] * 7 and r["face_area"][0] == -1 and r["nscores"][3] == 1
    # the cube against its cloud: outward everywhere, and the two restatements agree on every index although 12 % of the queries tie
    c, cloud = S.cube(), S.cube_cloud()
    a32, a64 = N.agree_f32(c, cloud), N.agree_f64(c, cloud)
    assert np.array_equal(a32["nn_idx"], a64["nn_idx"]) and (a32["face_agree"] > 0).all() and a32["nscores"][1] == 0
    assert N.tie_share(c, cloud) > 0.05
    # the overflow row: nothing measurable, nothing non-finite
    co, clo = N.degenerate6()
    r = N.batch(N.agree_f32, co, clo)
    assert all(np.isfinite(v).all() for v in r.values()) and r["nscores"][3].tolist() == [0, 0, 0, 4] and r["nscores"][1].tolist() == [0, 0, 0, 3]
    assert r["nscores"][2, 3] == 5 and N.agree_measurable(co[2]).sum() == 3


def test_ranking_inputs_decide_as_designed():
    """The crafted candidates of the GPU ranking test, on the restatement alone: the accordion is closer, the flat mesh more consistent."""
    c, cl = N.ranking()
    d = S.batch(S.score_ref, c, cl, 2)["scores"]
    n = N.batch(N.agree_f64, c, cl, 2)["nscores"]
    tot = 0.5 * (d[:, 0] + d[:, 1])
    assert tot[1] < tot[0] and abs(tot[0] - 0.125) < 5e-3            # every point is DELTA from the flat mesh; its quadrature points a little more
    assert abs(n[0, 0] - 1.0) < 1e-12 and abs(n[1, 0] - np.sqrt(0.5)) < 1e-12 and n[0, 1] == 0 and n[1, 1] == 0
    w = 2.0 * (tot[0] - tot[1]) / (n[0, 0] - n[1, 0])
    chosen, _ = mesh_score.select(torch.tensor(d, dtype=torch.float32), 2)
    assert chosen.tolist() == [1]
    chosen, _ = mesh_score.select(torch.tensor(d, dtype=torch.float32), 2, torch.tensor(n, dtype=torch.float32), w)
    assert chosen.tolist() == [0]


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_cli_flags(capsys):
    import main
    base = ["--input_path", "x.npy", "--input_type", "pc_normal"]
    a = main.get_args(base)
    assert a.normal_weight == 0.0 and a.orient == "volume"
    a = main.get_args(base + ["--sampling", "--num_candidates", "4", "--normal_weight", "0.1", "--orient", "cloud"])
    assert a.normal_weight == 0.1 and a.orient == "cloud" and a.num_candidates == 4
    assert main.get_args(base + ["--orient", "cloud"]).orient == "cloud"                  # orientation needs no candidates
    assert main.get_args(base + ["--normal_weight", "0"]).normal_weight == 0.0
    for bad, word in ((["--normal_weight", "0.1"], "--num_candidates > 1"), (["--sampling", "--num_candidates", "4", "--normal_weight", "-1"], ">= 0"),
                      (["--sampling", "--num_candidates", "4", "--normal_weight", "inf"], "finite"),
                      (["--sampling", "--num_candidates", "4", "--normal_weight", "nan"], "finite"), (["--orient", "winding"], "invalid choice")):
        with pytest.raises(SystemExit):
            main.get_args(base + bad)
        assert word in capsys.readouterr().err, bad
