"""Raw point clouds as input (`--input_type pc_xyz`, meshanything_amd/pc_normals.py) without a GPU: the sign propagation
`orient_normals` on the float64 reference's unoriented normals (tests/pc_normals_ref.py) of clouds whose true normals are known, the
refusals of `knn`, `estimate_normals`, `xyz_to_pc_normal`, the C ABI and `Dataset("pc_xyz")` that come before the first device call,
and the command line's new choices."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import pc_normals_ref as R

if R.REPO not in sys.path:
    sys.path.insert(0, R.REPO)

from meshanything_amd import _lib, build, pc_normals               # noqa: E402
from meshanything_amd.data import Dataset                          # noqa: E402

N_POINTS, K = 4096, 16


@pytest.fixture(scope="module")
def unoriented():
    """name -> (points, true normals, the reference's unoriented normals, the neighbour graph), computed once"""
    out = {}
    for name, make in R.CLOUDS.items():
        p, true = make(N_POINTS, seed=1)
        nbr, _ = R.knn_ref(p, None, K)
        n, _ = R.normals_eigh(p, nbr)
        out[name] = (p, true, n, nbr)
    return out


@pytest.mark.parametrize("name", list(R.CLOUDS))
def test_orientation_matches_the_true_normals(unoriented, name):
    p, true, n, nbr = unoriented[name]
    before = R.signed_share(n, true)
    assert 0.2 < before < 0.8                                       # the sign rule alone orients nothing
    got = pc_normals.orient_normals(p, n, nbr)
    share = R.signed_share(got, true)
    print(f"{name}: correctly signed before {before:.4f}, after {share:.4f}")
    assert got.dtype == np.float64 and np.array_equal(np.abs(got), np.abs(n))      # signs only
    assert share >= 0.99                                            # not 1 - share: the seed rule fixes the sign of the whole cloud
    again = pc_normals.orient_normals(p, n, nbr)
    assert np.array_equal(got, again)
    # the input's signs do not matter, only its lines
    flipped = n * np.where(np.arange(n.shape[0]) % 3 == 0, -1.0, 1.0)[:, None]
    assert np.array_equal(pc_normals.orient_normals(p, flipped, nbr), got)


def test_two_components_are_each_oriented_outward():
    a, ta = R.sphere(600, seed=2, radius=0.5, center=(0, 0, 0))
    b, tb = R.sphere(600, seed=3, radius=0.5, center=(10, 0, -3))
    p, true = np.concatenate([a, b]), np.concatenate([ta, tb])
    nbr, _ = R.knn_ref(p, None, 12)
    assert (nbr[:600] < 600).all() and (nbr[600:] >= 600).all()     # two components
    n, _ = R.normals_eigh(p, nbr)
    got = pc_normals.orient_normals(p, n, nbr)
    assert R.signed_share(got[:600], ta) >= 0.99 and R.signed_share(got[600:], tb) >= 0.99


def test_seed_rule_and_tie_break():
    # four coplanar points, all normals +-z: the seed is the lowest index among the points of greatest z and ends up pointing up
    p = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float64)
    n = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1]], np.float64)
    nbr = np.array([[0, 1, 2], [1, 0, 3], [2, 0, 3], [3, 1, 2]])
    assert np.array_equal(pc_normals.orient_normals(p, n, nbr), np.tile([0.0, 0.0, 1.0], (4, 1)))
    with pytest.raises(ValueError):
        pc_normals.orient_normals(p, n, nbr + 2)
    with pytest.raises(ValueError):
        pc_normals.orient_normals(p, n[:3], nbr)


def test_knn_and_estimate_normals_refuse_before_the_device():
    pts = torch.zeros((100, 3), dtype=torch.float32)
    for bad, kw in ((torch.zeros((100, 4)), {}), (torch.zeros(100), {}), (pts.double(), {}), (pts, {"k": 2}), (pts, {"k": 33}), (pts, {"k": 16.5}),
                    (pts[:15], {"k": 16}), (pts, {"splits": 65}), (pts, {"splits": -1}), (pts, {"query_idx": torch.zeros((2, 2), dtype=torch.int64)}),
                    (pts, {"query_idx": torch.zeros(0, dtype=torch.int64)}), (pts, {"query_idx": torch.zeros(4)}), (pts.numpy(), {})):
        with pytest.raises(ValueError):
            pc_normals.knn(bad, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):        # a well-formed host tensor: there is nothing to fall back to
        pc_normals.knn(pts)
    nbr = torch.zeros((100, 16), dtype=torch.int32)
    for a, b in ((pts, nbr.long()), (pts, nbr[:, :2]), (pts, nbr[0]), (pts[:10], nbr), (pts.double(), nbr)):
        with pytest.raises(ValueError):
            pc_normals.estimate_normals(a, b)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pc_normals.estimate_normals(pts, nbr)


def test_xyz_to_pc_normal_refuses_before_the_device_and_before_it_draws():
    good = R.sphere(5000, seed=0)[0]
    state = np.random.get_state()[1].copy()
    nonfinite = good.copy()
    nonfinite[17, 1] = np.nan
    for bad, kw in ((good[:4095], {}), (good[:, :2], {}), (good.reshape(-1), {}), (good.astype(np.int32), {}), (nonfinite, {}), (good, {"k": 2}),
                    (good, {"k": 33}), (good, {"n_points": 8, "k": 16}), (good, {"device": "cpu"})):
        with pytest.raises(ValueError):
            pc_normals.xyz_to_pc_normal(bad, **kw)
    assert np.array_equal(np.random.get_state()[1], state)          # a refused cloud consumes nothing from the global RNG
    inf_normals = np.concatenate([good, np.full_like(good, np.inf)], 1)
    assert pc_normals.check_xyz(inf_normals, 4096, 16) is not None   # columns after the third are not read


@pytest.fixture(scope="module")
def lib():
    build.build(force=False, verbose=False)
    return _lib.load()


def test_c_abi_checks_its_arguments_before_the_first_hip_call(lib):
    """dummy non-null pointers: every case is refused before anything is read or launched"""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    a256 = lambda b: (b + 255) & ~255                               # noqa: E731
    assert lib.ma_pc_knn_workspace_bytes(4096, 4096, 16, 1) > 0
    assert lib.ma_pc_knn_workspace_bytes(4096, 4096, 16, 7) == 2 * a256(7 * 16 * 4096 * 4)
    assert lib.ma_pc_knn_workspace_bytes(4096, 4096, 9, 7) == 2 * a256(7 * 16 * 4096 * 4)      # 9 neighbours live in a 16-slot list
    assert lib.ma_pc_knn_workspace_bytes(1 << 22, 1 << 20, 32, 64) == 2 * 64 * 32 * (1 << 20) * 4
    assert lib.ma_pc_knn_workspace_bytes(4096, 4096, 16, 0) > 0
    for N, Q, k, s in ((4096, 4096, 2, 0), (4096, 4096, 33, 0), (15, 4, 16, 0), ((1 << 22) + 1, 4, 16, 0), (4096, 0, 16, 0), (4096, (1 << 20) + 1, 16, 0),
                       (4096, 4096, 16, 65), (4096, 4096, 16, -1)):
        assert lib.ma_pc_knn_workspace_bytes(N, Q, k, s) == 0, (N, Q, k, s)
        assert lib.ma_op_pc_knn(p, N, 3, p, Q, k, s, p, p, p, 1 << 40, None) == -1
        assert lib.ma_last_error(None).decode().startswith("ma_op_pc_knn:")
    big = 1 << 40
    cases = [((None, 100, 3, p, 10, 16, 0, p, p, p, big, None), "null"), ((p, 100, 3, p, 10, 16, 0, None, p, p, big, None), "null"),
             ((p, 100, 3, p, 10, 16, 0, p, p, None, big, None), "null"), ((p, 100, 4, p, 10, 16, 0, p, p, p, big, None), "ref_ld"),
             ((p, 100, 3, None, 10, 16, 0, p, p, p, big, None), "Q must equal N"), ((p, 4096, 3, p, 4096, 16, 7, p, p, p, 1000, None), "workspace")]
    for args, word in cases:
        assert lib.ma_op_pc_knn(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_knn:") and word in msg, msg
    cases = [((None, 100, 3, p, 10, 16, p, p, None), "null"), ((p, 100, 3, p, 10, 16, None, p, None), "null"), ((p, 100, 5, p, 10, 16, p, p, None), "ref_ld"),
             ((p, 100, 3, p, 10, 2, p, p, None), "k"), ((p, 10, 3, p, 10, 16, p, p, None), "k"), ((p, 100, 3, p, 0, 16, p, p, None), "Q")]
    for args, word in cases:
        assert lib.ma_op_pc_normals(*args) == -1
        msg = lib.ma_last_error(None).decode()
        assert msg.startswith("ma_op_pc_normals:") and word in msg, msg


def test_dataset_pc_xyz_rejects_bad_clouds_without_a_gpu(tmp_path):
    good = R.sphere(5000, seed=0)[0]
    bad = good.copy()
    bad[3, 0] = np.inf
    short = good[:4000]
    for name, arr in (("nonfinite.npy", bad), ("short.npy", short), ("flat.npy", good[:, :2])):
        np.save(tmp_path / name, arr)
        with pytest.raises(ValueError):
            Dataset("pc_xyz", [str(tmp_path / name)])
    np.savetxt(tmp_path / "short.xyz", short[:50])
    with pytest.raises(ValueError, match="at least 4096"):
        Dataset("pc_xyz", [str(tmp_path / "short.xyz")])
    np.savetxt(tmp_path / "nonfinite.txt", bad)
    with pytest.raises(ValueError, match="non-finite"):
        Dataset("pc_xyz", [str(tmp_path / "nonfinite.txt")])
    with pytest.raises(ValueError):
        Dataset("pc_xyz", [str(tmp_path / "short.npy")], normal_k=2)
    assert len(Dataset("pc", [str(tmp_path / "short.npy")])) == 0   # the reference's default type is still unknown and still empty


def test_command_line_knows_pc_xyz(capsys, monkeypatch):
    import importlib.util
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))   # main.py sets a default on import
    spec = importlib.util.spec_from_file_location("ma_main_cli", os.path.join(R.REPO, "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.get_args(["--input_type", "pc_xyz", "--input_path", "scan.xyz"])
    assert a.input_type == "pc_xyz" and a.normal_k == 16
    assert cli.get_args(["--input_type", "pc_xyz", "--normal_k", "32"]).normal_k == 32
    assert cli.get_args([]).input_type == "pc"                      # the reference's default stays
    for argv in (["--normal_k", "2"], ["--normal_k", "33"], ["--input_type", "pc"]):
        with pytest.raises(SystemExit):
            cli.get_args(argv)
    capsys.readouterr()
