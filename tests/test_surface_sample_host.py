"""GPU surface sampling (meshanything_amd/surface_sample.py, csrc/surface_sample.hpp), host side: the float64 -> float16 conversion the
sampler applies (through the library's host-only ma_f64_to_f16), the ABI's argument checks and the Python wrappers' mesh checks, which
all run before anything touches a device, and the command-line flag.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_sample_ref as S
import watertight_ref as W
from meshanything_amd import _lib
from meshanything_amd.data import Dataset
from meshanything_amd.mesh_input import mesh_to_pc_normal
from meshanything_amd import watertight

REPO = W.REPO
INVALID = -1
P = C.c_void_p(16)                                                 # a non-null pointer that is never dereferenced


@pytest.fixture(scope="module")
def lib():
    W.mc_table()                                                   # builds the library if needed
    return _lib.load()


def _f16(lib, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty(x.shape, np.uint16)
    assert lib.ma_f64_to_f16(x.ctypes.data, x.size, out.ctypes.data) == 0
    return out


def test_f64_to_f16_is_numpys_cast(lib):
    rng = np.random.default_rng(0)
    half = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)          # every finite non-negative float16
    mid = (half[:-1] + half[1:]) / 2                                                       # ties: round to even
    cases = [rng.standard_normal(1 << 20) * 10.0 ** rng.uniform(-9, 6, 1 << 20), half, mid, np.nextafter(mid, 0), np.nextafter(mid, 1),
             np.array([65504.0, 65519.99, 65520.0, 1e300, np.inf, 0.0, -0.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -52), 2.0 ** -24, 5e-324,
                       2.0 ** -14 - 2.0 ** -30])]
    with np.errstate(over="ignore"):
        for x in cases:
            for s in (x, -x):
                assert np.array_equal(_f16(lib, s), s.astype(np.float16).view(np.uint16))
    # one rounding, not two: through float32 this would be 1.0
    x = np.array([1 + 2.0 ** -11 + 2.0 ** -40])
    assert _f16(lib, x)[0] == 0x3C01 == x.astype(np.float16).view(np.uint16)[0]
    assert x.astype(np.float32).astype(np.float16).view(np.uint16)[0] == 0x3C00
    assert np.isnan(_f16(lib, np.array([np.nan])).view(np.float16)[0])


def test_abi_refuses_bad_arguments_on_the_host(lib):
    ws = lib.ma_surface_sample_workspace_bytes(1000)
    assert ws >= 1000 * 8
    assert lib.ma_surface_sample_workspace_bytes(0) == 0
    assert lib.ma_surface_sample_workspace_bytes((1 << 28) + 1) == 0
    assert lib.ma_surface_sample_workspace_bytes(1 << 28) > 0
    cdf = lib.ma_op_surface_cdf
    assert cdf(None, 3, P, 1, P, P, P, ws, None) == INVALID
    assert b"null" in lib.ma_last_error(None)
    for args in [(P, 3, None, 1), (P, 0, P, 1), (P, 3, P, 0), (P, 3, P, -5), (P, 3, P, (1 << 28) + 1)]:
        assert cdf(*args, P, P, P, ws, None) == INVALID
    assert cdf(P, 3, P, 1, None, P, P, ws, None) == INVALID
    assert cdf(P, 3, P, 1, P, None, P, ws, None) == INVALID
    assert cdf(P, 3, P, 1, P, P, None, ws, None) == INVALID
    assert cdf(P, 3, P, 1000, P, P, P, ws - 1, None) == INVALID
    assert b"workspace" in lib.ma_last_error(None)
    draw = lib.ma_op_sample_surface
    good = [P, 3, P, 1, P, P, P, P, 4096, P, None, None]
    for i in (0, 2, 4, 5, 6, 7, 9):                                  # every pointer but face_idx is required
        args = list(good)
        args[i] = None
        assert draw(*args) == INVALID
    for i, bad in [(8, 0), (8, -1), (3, 0), (3, (1 << 28) + 1), (1, 0)]:
        args = list(good)
        args[i] = bad
        assert draw(*args) == INVALID
    center = (C.c_double * 3)(0.0, 0.0, 0.0)
    frame = lib.ma_op_mc_vertices_to_frame
    assert frame(None, 3, 128, 0.9, center, P, None) == INVALID
    assert frame(P, 3, 128, 0.9, None, P, None) == INVALID
    assert frame(P, 0, 128, 0.9, center, P, None) == INVALID
    assert frame(P, 3, 0, 0.9, center, P, None) == INVALID
    assert frame(P, 3, 128, 0.0, center, P, None) == INVALID
    assert frame(P, 3, 128, float("inf"), center, P, None) == INVALID


def test_wrappers_check_the_mesh_before_the_device():
    """Every refusal below comes before any device work (on a host without a GPU anything else would not be a ValueError), and leaves
    the global RNG where it was."""
    v, f = W.open_box()
    bad_vertex = v.copy()
    bad_vertex[3, 1] = np.inf
    cases = [(np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (v, np.zeros((0, 3), np.int64)), (bad_vertex, f),
             (v, np.vstack([f, [[0, 1, 8]]])), (v, np.vstack([f, [[0, -1, 2]]])), (v, f[:, :2]), (v, f.astype(np.float64))]
    np.random.seed(3)
    state = np.random.get_state()
    for vv, ff in cases:
        with pytest.raises(ValueError):
            mesh_to_pc_normal(vv, ff, device="cuda")
        with pytest.raises(ValueError):
            watertight.process_mesh_to_pc([(v, f), (vv, ff)], marching_cubes=True, device="cuda")
    with pytest.raises(ValueError, match="sample_num"):
        mesh_to_pc_normal(v, f, 0, device="cuda")
    with pytest.raises(ValueError, match="CUDA device"):
        mesh_to_pc_normal(v, f, device="cpu")
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    # the device path accepts what the host path accepts: a mesh without extent is refused for its missing area, as on the host
    assert watertight.check_mesh(np.ones((3, 3)), [[0, 1, 2]], need_extent=False)[0].shape == (3, 3)
    with pytest.raises(ValueError, match="extent"):
        watertight.check_mesh(np.ones((3, 3)), [[0, 1, 2]])
    # Dataset keeps refusing --mc whatever the sampling device
    with pytest.raises(NotImplementedError, match="process_mesh_to_pc"):
        Dataset("mesh", ["a.obj"], mc=True, sample_device="cuda")


def test_host_restatement_is_the_host_sampler():
    """surface_sample_ref.host_sample, which the GPU tests compare the kernels with on hand-made draws, is mesh_input's sampler."""
    for name in ("torus", "open_box_degenerate", "boundary"):
        v, f = S.MESHES[name]()
        np.random.seed(11)
        ref = mesh_to_pc_normal(v, f, 512)
        np.random.seed(11)
        u = np.random.random(512)
        uv = np.random.random((512, 2))
        got, idx, _, _ = S.host_sample(v, f, u, uv)
        assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))
    v, f = S.boundary_mesh()
    u = np.array([0.0, 0.25, 0.75, 0.875, 1 - 2.0 ** -53, 1.0])
    _, idx, _, cum = S.host_sample(v, f, u, np.full((6, 2), 0.25))
    assert np.array_equal(cum, [0, 0.5, 0.5, 1.5, 1.75, 1.75, 2, 2])
    assert idx.tolist() == [1, 3, 4, 6, 6, 7]                        # side="right"; only the clamp reaches the zero-area last face


def test_cli_has_the_gpu_sampling_flag():
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--gpu_sampling" in r.stdout
