"""Best-of-N sampling without a GPU: the argument checks of ma_op_score_meshes / ma_score_meshes_workspace_bytes (they run before the
first HIP call), `mesh_score.select` on hand-made score tables, the float64 reference of tests/mesh_score_ref.py against a brute-force
bound, `config_from_args` with num_candidates and main.py's argparse error."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

import mesh_score_ref as R

REPO = R.REPO
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from meshanything_amd import _lib, build                           # noqa: E402
from meshanything_amd import mesh_score                            # noqa: E402

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


def _call(lib, B=4, F=8, cloud_ld=6, P=16, n=2, scale=2.0, ws_bytes=None, coords=1, cloud=1, scores=1, ws=1):
    """ma_op_score_meshes with dummy non-null pointers: every case here is refused before anything is read or launched"""
    buf = (C.c_float * 4)()
    p = lambda on: C.addressof(buf) if on else None                  # noqa: E731
    nb = lib.ma_score_meshes_workspace_bytes(B, F, P) if ws_bytes is None else ws_bytes
    return lib.ma_op_score_meshes(p(coords), B, F, p(cloud), cloud_ld, P, n, scale, p(scores), p(ws), nb, None)


@pytest.mark.parametrize("kw,word", [
    (dict(coords=0), "null"), (dict(cloud=0), "null"), (dict(scores=0), "null"), (dict(ws=0), "null"),
    (dict(B=0, ws_bytes=1 << 20), "B >= 1"), (dict(F=0, ws_bytes=1 << 20), "F"), (dict(F=(1 << 20) + 1, ws_bytes=1 << 40), "F"),
    (dict(P=0, ws_bytes=1 << 20), "P"), (dict(P=(1 << 20) + 1, ws_bytes=1 << 40), "P"),
    (dict(n=0), "n_per_cloud"), (dict(n=3), "n_per_cloud"), (dict(n=-2), "n_per_cloud"),
    (dict(cloud_ld=4), "cloud_ld"), (dict(cloud_ld=0), "cloud_ld"),
    (dict(scale=0.0), "mesh_scale"), (dict(scale=-1.0), "mesh_scale"), (dict(scale=INF), "mesh_scale"), (dict(scale=float("nan")), "mesh_scale"),
    (dict(ws_bytes=0), "workspace"), (dict(ws_bytes=4 * 16 * 4 + 2 * 4 * 8 * 4 - 1), "workspace"),
])
def test_bad_arguments_are_refused_without_a_gpu(lib, kw, word):
    assert _call(lib, **kw) == -1                                    # MA_ERR_INVALID
    msg = lib.ma_last_error(None).decode()
    assert msg.startswith("ma_op_score_meshes:") and word in msg, msg


def test_workspace_bytes(lib):
    a256 = lambda b: (b + 255) & ~255                                # noqa: E731
    for B, F, P in [(1, 1, 1), (4, 8, 16), (12, 130, 67), (64, 800, 4096), (1, 1 << 20, 1 << 20)]:
        assert lib.ma_score_meshes_workspace_bytes(B, F, P) == a256(B * P * 4) + 2 * a256(B * F * 4)
    for B, F, P in [(0, 8, 16), (-1, 8, 16), (1, 0, 16), (1, 8, 0), (1, (1 << 20) + 1, 16), (1, 8, (1 << 20) + 1)]:
        assert lib.ma_score_meshes_workspace_bytes(B, F, P) == 0
    # many candidates of the largest mesh: the size does not wrap
    assert lib.ma_score_meshes_workspace_bytes(1 << 12, 1 << 20, 1 << 20) == 3 * (1 << 34)


def test_score_meshes_checks_its_tensors_before_the_device():
    c, pc = torch.zeros(4, 8, 3, 3), torch.zeros(2, 16, 6)
    for bad in [(torch.zeros(4, 8, 9), pc, 2, 2.0), (c, torch.zeros(2, 16, 4), 2, 2.0), (c, pc, 3, 2.0), (c, pc, 1, 2.0), (c, pc, 0, 2.0),
                (c, pc.double(), 2, 2.0), (c, pc, 2, 0.0), (c, pc, 2, INF), (c, pc, 2, float("nan")), (torch.zeros(0, 8, 3, 3), pc[:0], 1, 2.0)]:
        with pytest.raises(ValueError):
            mesh_score.score_meshes(*bad)
    with pytest.raises(ValueError, match="CUDA"):                   # no CPU fallback
        mesh_score.score_meshes(c, pc, 2)


def _table(rows):
    """(B, 4) scores whose totals 0.5 * ([0] + [1]) are `rows`"""
    t = torch.tensor(rows, dtype=torch.float32).reshape(-1)
    return torch.stack([t, t, torch.ones_like(t), torch.ones_like(t)], 1)


def test_select_takes_the_lowest_total_and_the_lowest_index_on_ties():
    chosen, total = mesh_score.select(_table([[3.0, 1.0, 2.0, 1.0], [0.5, 0.5, 0.5, 0.5], [4.0, 3.0, 2.0, 1.0]]), 4)
    assert chosen.dtype == torch.int64 and chosen.tolist() == [1, 0, 3]
    assert total.shape == (3, 4) and total[0].tolist() == [3.0, 1.0, 2.0, 1.0]
    s = torch.tensor([[1.0, 3.0, 9.0, 2.0], [2.5, 1.0, 9.0, 2.0]])    # total = 0.5 * (cloud to mesh + mesh to cloud): 2.0 and 1.75
    chosen, total = mesh_score.select(s, 2)
    assert chosen.tolist() == [1] and total.tolist() == [[2.0, 1.75]]
    assert mesh_score.select(s, 1)[0].tolist() == [0, 0]
    assert mesh_score.select(s.numpy(), 2)[0].tolist() == [1]


def test_select_never_prefers_inf():
    chosen, total = mesh_score.select(_table([[INF, 7.0, INF, 7.0], [INF, INF, INF, INF], [INF, INF, INF, 1e30]]), 4)
    assert chosen.tolist() == [1, 0, 3]
    assert torch.isinf(total[1]).all()
    # one directed term infinite (no area) is as bad as both
    s = torch.tensor([[0.1, INF, 0.0, 3.0], [5.0, 6.0, 1.0, 3.0]])
    assert mesh_score.select(s, 2)[0].tolist() == [1]
    with pytest.raises(ValueError):
        mesh_score.select(_table([[1.0, 2.0, 3.0]]), 2)


def _bary_samples(tri, n):
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    m = i + j <= n
    u, v = i[m] / n, j[m] / n
    return tri[0] + u[:, None] * (tri[1] - tri[0]) + v[:, None] * (tri[2] - tri[0])


def test_reference_against_dense_sampling_of_the_triangles():
    """The distance to the nearest of (n + 1)(n + 2) / 2 barycentric samples of a triangle is at least the distance to the triangle and
    exceeds it by at most the samples' pitch (longest edge / n: no point of the triangle is further than that from a sample)."""
    n = 96
    for coords, cloud, scale in [(R.soup(6, 70), R.points(40, 71), 2.0), (R.degenerate_batch()[0][2], R.points(40, 72), 2.0),
                                 (R.voronoi()[0][0], R.voronoi()[1][0], 1.0)]:
        ref = R.score_ref(coords, cloud, scale)
        tri = coords[R.valid_rows(coords)].astype(np.float64) * scale
        pts = cloud[:, :3].astype(np.float64)
        brute, pitch = np.full(len(pts), np.inf), 0.0
        for t in tri:
            s = _bary_samples(t, n)
            brute = np.minimum(brute, np.sqrt(((pts[:, None] - s[None]) ** 2).sum(-1)).min(1))
            pitch = max(pitch, max(np.linalg.norm(t[a] - t[b]) for a, b in ((0, 1), (1, 2), (2, 0))) / n)
        assert (ref["pt_dist"] <= brute + 1e-12).all()
        assert (brute <= ref["pt_dist"] + pitch).all()
        assert ref["scores"][0] == pytest.approx(ref["pt_dist"].mean(), abs=1e-15)
        # mesh to cloud: the definition, written out face by face
        num = den = 0.0
        for t in tri:
            q = [t[0], t[1], t[2], (t[0] + t[1]) / 2, (t[1] + t[2]) / 2, (t[2] + t[0]) / 2, t.mean(0)]
            a = 0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0]))
            num += a * np.mean([np.linalg.norm(pts - x, axis=1).min() for x in q])
            den += a
        assert ref["scores"][1] == pytest.approx(num / den, rel=1e-12)
        assert ref["scores"][2] == pytest.approx(den, rel=1e-12) and ref["scores"][3] == len(tri)


def test_reference_edge_cases_and_fp32_restatement():
    c, cloud = R.degenerate_batch()
    r = R.batch(R.score_ref, c, cloud)
    assert np.isinf(r["scores"][0, :2]).all() and r["scores"][0, 3] == 0                       # no valid face
    assert np.isfinite(r["scores"][1, 0]) and np.isinf(r["scores"][1, 1]) and r["scores"][1, 2] == 0 and r["scores"][1, 3] == 3
    assert np.isfinite(r["scores"][2]).all() and r["scores"][2, 3] == 5
    assert not np.isnan(r["scores"]).any()
    # the cube under its own surface cloud: every point lies on a face
    cube = R.score_ref(R.cube(), R.cube_cloud())
    assert cube["scores"][0] == 0.0 and cube["scores"][2] == pytest.approx(6 * 1.5 ** 2) and cube["scores"][3] == 12
    # fp32 restatement: the same numbers up to what fp32 resolves (the GPU test derives its tolerance from this deviation)
    a, b = R.score_ref(R.soup(200, 80), R.points(500, 81)), R.score_f32(R.soup(200, 80), R.points(500, 81))
    dev = max(np.abs(a["pt_dist"] - b["pt_dist"]).max(), np.abs(a["face_nn"] - b["face_nn"]).max())
    print(f"fp32 restatement vs fp64 reference, 200-face soup: largest per-point deviation {dev:.3g}")
    assert 0 < dev < 5e-7


def test_config_from_args_multiplies_the_batch_by_the_candidates():
    from meshanything_amd.model import config_from_args
    base = dict(llm="facebook/opt-350m", codebook_size=8192, codebook_dim=1024, n_max_triangles=800)
    assert config_from_args(types.SimpleNamespace(**base)).max_batch == 1
    assert config_from_args(types.SimpleNamespace(**base, batchsize_per_gpu=2)).max_batch == 2
    assert config_from_args(types.SimpleNamespace(**base, batchsize_per_gpu=2, num_candidates=1)).max_batch == 2
    assert config_from_args(types.SimpleNamespace(**base, batchsize_per_gpu=2, num_candidates=4)).max_batch == 8
    assert config_from_args(types.SimpleNamespace(**base, num_candidates=8)).max_batch == 8
    assert config_from_args(types.SimpleNamespace(**base, num_candidates=0)).max_batch == 1


def test_cli_refuses_candidates_without_sampling(capsys):
    sys.path.insert(0, REPO)
    import main
    base = ["--input_path", "x.npy", "--input_type", "pc_normal"]
    assert main.get_args(base).num_candidates == 1
    assert main.get_args(base + ["--sampling", "--num_candidates", "8"]).num_candidates == 8
    assert main.get_args(base + ["--num_candidates", "1"]).num_candidates == 1
    for bad in (["--num_candidates", "4"], ["--sampling", "--num_candidates", "0"]):
        with pytest.raises(SystemExit) as e:
            main.get_args(base + bad)
        assert e.value.code == 2
    assert "--num_candidates" in capsys.readouterr().err
