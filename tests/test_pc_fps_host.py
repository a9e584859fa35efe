"""Farthest-point sampling (`--point_sampling fps`, meshanything_amd/pc_fps.py) without a GPU: the properties of the definition on its
numpy restatement (tests/pc_fps_ref.py), what it buys on a cloud of uneven density, every refusal that comes before the first device
call (`farthest_point_sample`, `xyz_to_pc_normal`, `Dataset`, the C ABI), and the command line's new flag."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import pc_fps_ref as R

if R.REPO not in sys.path:
    sys.path.insert(0, R.REPO)

from meshanything_amd import _lib, build, pc_fps, pc_normals       # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402


def _check_properties(cloud, n, start):
    idx, d2, m = R.fps_ref(cloud, n, start)
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    assert len(set(idx.tolist())) == n and idx.min() >= 0 and idx.max() < cloud.shape[0]
    assert np.isposinf(d2[0]) and (np.diff(d2[1:]) <= 0).all()
    assert (m[idx] == -1).all() and (np.delete(m, idx) >= 0).all()
    # the covering radius by brute force, with the same float32 key: exactly what m holds (a picked row is at distance 0 of itself)
    brute = R.nearest_key(cloud, idx)
    assert np.array_equal(brute, np.maximum(m, np.float32(0)))
    assert np.sqrt(brute.max()) == np.sqrt(max(m.max(), np.float32(0)))
    if n > 1:
        assert brute.max() <= d2[n - 1]                             # every point lies within sqrt(d2[n - 1]) of a picked one
    return idx, d2, m


@pytest.mark.parametrize("start", [-1, 0, 999])
def test_properties_on_a_random_cloud(start):
    cloud = R.uniform_cloud(1000, 6, seed=1)
    idx, d2, _ = _check_properties(cloud, 200, start)
    assert idx[0] == (R.start_ref(cloud[:, :3]) if start < 0 else start)
    again = R.fps_ref(cloud[:, :3].copy(), 200, start)              # the columns after xyz are not read
    assert np.array_equal(again[0], idx) and again[1].tobytes() == d2.tobytes()


def test_lattice_ties_go_to_the_lowest_index():
    cloud = R.lattice(8)
    idx, d2, _ = _check_properties(cloud, 512, -1)
    assert sorted(idx.tolist()) == list(range(512))                 # n = N: every row, once
    # the centre is (3.5, 3.5, 3.5): the eight corners tie, row 0 is the lowest; then the opposite corner alone is farthest
    assert idx[0] == 0 and idx[1] == 511 and d2[1] == 3 * 49
    # every pick is the lowest index among the rows at the greatest distance from the picks before it
    m = np.full(512, np.inf, np.float32)
    for t in range(64):
        if t:
            assert idx[t] == np.flatnonzero(m == m.max())[0] and (m == m.max()).sum() >= 1
        m = np.minimum(m, R.key_to(cloud, cloud[idx[t]]))
        m[idx[t]] = -1
    ties = sum(int((d2[1:] == v).sum() > 1) for v in np.unique(d2[1:]))
    assert ties >= 3                                                # whole runs of picks at one distance


def test_fewer_distinct_positions_than_picks():
    cloud = R.few_positions(300, 7)
    assert len({tuple(r) for r in cloud.tolist()}) == 7
    idx, d2, _ = _check_properties(cloud, 64, -1)
    assert (d2[1:7] > 0).all() and (d2[7:] == 0).all()              # the seven positions first, then their duplicates at distance 0
    assert len({tuple(r) for r in cloud[idx[:7]].tolist()}) == 7
    assert (np.diff(idx[7:]) > 0).all()                             # among equals (all at 0): ascending index


def test_uneven_density_is_what_fps_is_for():
    """18 000 points on the cap z > 0.8 of the unit sphere and 2 000 over the whole of it: the covering radius farthest-point sampling
    leaves with 4 096 points against the smallest of three uniform draws (measured: 0.0165 against 0.231)."""
    cloud = R.uneven_sphere()
    assert cloud.shape == (20000, 3)
    idx, d2, m = R.fps_ref(cloud.astype(np.float32), 4096)
    fps_radius = R.covering_radius(cloud, idx)
    assert abs(fps_radius - float(np.sqrt(m.max()))) < 1e-5         # float32 key against the float64 brute force
    np.random.seed(0)
    draws = [R.covering_radius(cloud, np.random.choice(20000, 4096, replace=False)) for _ in range(3)]
    print(f"covering radius: fps {fps_radius:.4f}, three random draws {' '.join(f'{r:.4f}' for r in draws)}")
    assert fps_radius <= min(draws) / 4


def test_farthest_point_sample_refuses_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    big = torch.zeros((pc_fps.ONE_MAX_POINTS + 1, 3), dtype=torch.float32)
    for bad, kw in ((torch.zeros((100, 4)), {"n": 10}), (torch.zeros(100), {"n": 10}), (torch.zeros((2, 50, 3)), {"n": 10}), (pts.double(), {"n": 10}),
                    (pts.numpy(), {"n": 10}), (pts, {"n": 101}), (pts, {"n": 0}), (pts, {"n": 10.5}), (pts, {"n": True}), (pts, {"n": (1 << 16) + 1}),
                    (pts, {"n": 10, "start": 100}), (pts, {"n": 10, "start": -1}), (pts, {"n": 10, "start": 1.0}), (pts, {"n": 10, "form": 3}),
                    (pts, {"n": 10, "form": -1}), (pts, {"n": 10, "form": None}), (big, {"n": 10, "form": 1})):
        with pytest.raises(ValueError):
            pc_fps.farthest_point_sample(bad, **kw)
    for kw in ({"n": 10}, {"n": 100, "start": 99, "form": 2}, {"n": 1, "start": 0, "form": 1}):
        with pytest.raises(ValueError, match="no CPU fallback"):    # well-formed host tensors: there is nothing to fall back to
            pc_fps.farthest_point_sample(pts, **kw)
    with pytest.raises(ValueError, match="2\\^22"):
        pc_fps.check_fps_args((1 << 22) + 1, 4096, None, 0)
    assert pc_fps.check_fps_args(1 << 22, 1 << 16, None, 2) == (1 << 16, -1, 2)


def test_input_side_refuses_before_the_device_and_draws_nothing(tmp_path):
    good = R.sphere(5000, seed=0)[0]
    bad = good.copy()
    bad[3, 0] = np.inf
    state = np.random.get_state()[1].copy()
    for arr, kw in ((bad, {}), (good[:4000], {}), (good[:, :2], {}), (good.astype(np.int32), {}), (good, {"device": "cpu"})):
        with pytest.raises(ValueError):
            pc_normals.xyz_to_pc_normal(arr, sampling="fps", **kw)
    with pytest.raises(ValueError, match="sampling"):
        pc_normals.xyz_to_pc_normal(good, sampling="poisson")
    with pytest.raises(ValueError):
        pc_fps.fps_rows(good, 4096, device="cpu")
    wide = np.concatenate([good, np.full_like(good, np.nan)], 1)     # columns after the third are not read
    assert pc_fps.check_cloud_for_fps(wide, 4096) is wide
    files = {"nonfinite.npy": np.concatenate([bad, good], 1), "short.npy": np.concatenate([good, good], 1)[:4000], "flat.npy": good[:, :2],
             "ints.npy": np.zeros((5000, 6), np.int32)}
    for name, arr in files.items():
        np.save(tmp_path / name, arr)
        for kind in ("pc_normal", "pc_xyz"):
            with pytest.raises(ValueError):
                Dataset(kind, [str(tmp_path / name)], point_sampling="fps")
    with pytest.raises(ValueError, match="non-finite"):
        Dataset("pc_normal", [str(tmp_path / "nonfinite.npy")], point_sampling="fps")
    with pytest.raises(ValueError, match="at least"):
        Dataset("pc_normal", [str(tmp_path / "short.npy")], point_sampling="fps")
    with pytest.raises(ValueError, match="mesh"):
        Dataset("mesh", [], point_sampling="fps")
    with pytest.raises(ValueError, match="point_sampling"):
        Dataset("pc_normal", [], point_sampling="voxel")
    assert len(Dataset("pc", [str(tmp_path / "short.npy")], point_sampling="fps")) == 0   # the reference's default type is still empty
    assert np.array_equal(np.random.get_state()[1], state)          # nothing above consumed a draw


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


def test_c_abi_checks_its_arguments_before_the_first_hip_call(lib):
    """dummy non-null pointers: every case is refused before anything is read or launched"""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    big = 1 << 40
    a256 = lambda b: (b + 255) & ~255                               # noqa: E731
    for N, n, form in ((4096, 4096, 0), (4096, 1, 1), (1 << 22, 1 << 16, 2), (1 << 14, 64, 1), ((1 << 14) + 1, 64, 1)):
        G = -(-N // max(512, -(-N // 1024)))
        assert lib.ma_pc_fps_workspace_bytes(N, n, form) >= N * 4 + 2 * 8 * G + 24 * G
        assert lib.ma_pc_fps_workspace_bytes(N, n, form) == lib.ma_pc_fps_workspace_bytes(N, n, 2)   # one layout for every form
    assert lib.ma_pc_fps_workspace_bytes(4096, 4096, 0) == a256(4096 * 4) + 2 * a256(8 * 8) + a256(8 * 24)
    for N, n, form in ((4096, 4097, 0), (4096, 0, 0), (0, 0, 0), ((1 << 22) + 1, 4096, 0), (1 << 20, (1 << 16) + 1, 0), (4096, 64, 3), (4096, 64, -1)):
        assert lib.ma_pc_fps_workspace_bytes(N, n, form) == 0, (N, n, form)
        assert lib.ma_op_pc_fps(p, N, 3, n, 0, form, p, p, p, big, None) == -1
        assert lib.ma_last_error(None).decode().startswith("ma_op_pc_fps:")
    cases = [((None, 100, 3, 10, 0, 0, p, p, p, big, None), "null"), ((p, 100, 3, 10, 0, 0, None, p, p, big, None), "null"),
             ((p, 100, 3, 10, 0, 0, p, None, p, big, None), "null"), ((p, 100, 3, 10, 0, 0, p, p, None, big, None), "null"),
             ((p, 100, 4, 10, 0, 0, p, p, p, big, None), "ref_ld"), ((p, 100, 3, 10, 100, 0, p, p, p, big, None), "start"),
             ((p, 100, 3, 10, -2, 0, p, p, p, big, None), "start"), ((p, (1 << 14) + 1, 3, 10, 0, 1, p, p, p, big, None), "form 1"),
             ((p, 4096, 3, 10, 0, 0, p, p, p, 1000, None), "workspace")]
    for args, word in cases:
        assert lib.ma_op_pc_fps(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_fps:") and word in msg, msg


def test_command_line_knows_point_sampling(capsys, monkeypatch):
    import importlib.util
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))   # main.py sets a default on import
    spec = importlib.util.spec_from_file_location("ma_main_cli_fps", os.path.join(R.REPO, "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.get_args([]).point_sampling == "random"              # the reference's draw stays the default
    assert cli.get_args(["--input_type", "pc_normal", "--point_sampling", "fps"]).point_sampling == "fps"
    assert cli.get_args(["--input_type", "pc_xyz", "--point_sampling", "fps"]).point_sampling == "fps"
    assert cli.get_args(["--input_type", "mesh", "--point_sampling", "random"]).point_sampling == "random"
    for argv in (["--input_type", "mesh", "--point_sampling", "fps"], ["--point_sampling", "voxel"], ["--input_type", "mesh", "--mc", "--point_sampling", "fps"]):
        with pytest.raises(SystemExit):
            cli.get_args(argv)
    capsys.readouterr()
