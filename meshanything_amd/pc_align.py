"""Alignment of input clouds to their tightest box (`--align_iters`): search the rotations for the one under which the cloud's axis-aligned
bounding box is smallest, and turn the rows into that frame; the oriented bounding box of PCL and Open3D.

`data.normalize_pc` centres a cloud on its AXIS-ALIGNED box and the detokenizer's 128-step lattice lies along the same axes, so a scan that
sits askew in its file loses resolution to empty box corners and shows the decoder a turned shape.  PCA does not find the frame (a cube's
moments are degenerate); a search does.  `box_extents` is the call into the HIP library (csrc/pc_align.hpp; C ABI ma_op_pc_align_extents,
whose header comment states the rule): the extents of every row under up to 2^16 rotations, their box volumes and the least of them, equal
to a numpy float32 restatement bit for bit.  `draw_rotations` draws the hypotheses from a private generator, `search` is the loop, coarse
over all rotations and then ever finer about the best so far, with radii that follow from the hypothesis count; `align_rows` is what
`cloud_prep` calls.  They need CUDA tensors; there is no CPU fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_common import check_device_cloud, check_host_cloud, check_int, check_want, cuda_device, is_real, need_cuda

MAX_HYPOTHESES = 1 << 16                                         # MA_PC_ALIGN_MAX_HYPOTHESES
MIN_ITERS, MAX_ROUNDS = 256, 8
WANT = ("extents", "volumes", "best")
SEED = 0x616c69676e                                              # "align"


def box_extents(points: torch.Tensor, rotations: torch.Tensor, centre, want=("volumes", "best")):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns, 1 <= N <= 2^22; rotations (H, 9) or (H, 3, 3) float32 on the
    same device, row-major, 1 <= H <= 2^16; centre: three host numbers (cast to float32) -> a dict with the entries named in `want`:
    "extents" (H, 6) float32, the min (three) and max (three) over the rows of r (p - centre) under the rule of ma_op_pc_align_extents, six
    NaN for a bad hypothesis (a non-finite entry or coordinate); "volumes" (H) float64, the box volumes, +inf for a bad one; "best" (1)
    int32, the hypothesis of the least volume, the lowest index among equals, -1 if all are bad.  Equal to the numpy restatement and to a
    second run, bit for bit."""
    check_device_cloud(points, 1)
    want = check_want(want, WANT)
    if not torch.is_tensor(rotations) or rotations.dtype != torch.float32 or tuple(rotations.shape[1:]) not in ((9,), (3, 3)):
        raise ValueError(f"rotations must be a (H, 9) or (H, 3, 3) float32 tensor, got {tuple(rotations.shape) if hasattr(rotations, 'shape') else type(rotations).__name__}"
                         f" {getattr(rotations, 'dtype', '')}")
    if not 1 <= rotations.shape[0] <= MAX_HYPOTHESES:
        raise ValueError(f"need 1 <= H <= 2^16 hypotheses, got H = {rotations.shape[0]}")
    try:
        centre = np.asarray(centre.detach().cpu() if torch.is_tensor(centre) else centre, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"centre must be three numbers, got {centre!r}") from None
    if centre.shape != (3,):
        raise ValueError(f"centre must be three numbers, got shape {centre.shape}")
    need_cuda(points, "box_extents")
    if rotations.device != points.device:
        raise ValueError(f"box_extents runs on the GPU: rotations must be on the points' device {points.device}, got {rotations.device}")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref, rot = points.contiguous(), rotations.reshape(rotations.shape[0], 9).contiguous()
        N, H = ref.shape[0], rot.shape[0]
        nbytes = lib.ma_pc_align_workspace_bytes(N, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        extents = torch.empty((H, 6), dtype=torch.float32, device=dev) if "extents" in want else None
        volumes = torch.empty(H, dtype=torch.float64, device=dev) if "volumes" in want else None
        best = torch.empty(1, dtype=torch.int32, device=dev) if "best" in want else None
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        _lib.check(lib.ma_op_pc_align_extents(ref.data_ptr(), N, ref.shape[1], (C.c_float * 3)(*centre.tolist()), rot.data_ptr(), H, ptr(extents), ptr(volumes),
                                              ptr(best), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = {"extents": extents, "volumes": volumes, "best": best}
    return {w: out[w] for w in WANT if w in want}


def cube_rotations() -> np.ndarray:
    """(24, 3, 3) float64: the proper rotations of the cube, the signed permutation matrices of determinant +1.  The order is fixed: by the
    permutation (row a has its entry in column perm[a]) in lexicographic order, (0 1 2) first, and within one permutation by the signs of
    rows 0 and 1, (+ +), (+ -), (- +), (- -), the sign of row 2 being the one that makes the determinant +1.  Index 0 is the identity."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        parity = 1.0 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1.0
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                m = np.zeros((3, 3))
                m[0, perm[0]], m[1, perm[1]], m[2, perm[2]] = s0, s1, parity * s0 * s1
                out.append(m)
    return np.stack(out)


def nearest_representative(R) -> np.ndarray:
    """C R for the C of `cube_rotations()` with the greatest trace of C R, the first among equals.  A box fixes its axes only up to the 24;
    the greatest trace is the least angle of rotation, so a cloud whose axes are roughly right keeps its up and its front."""
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3):
        raise ValueError(f"R must be a 3 x 3 matrix, got shape {R.shape}")
    cand = cube_rotations() @ R                                      # signed row permutations: exact
    return cand[int(np.argmax(np.trace(cand, axis1=1, axis2=2)))]


def _exp(w: np.ndarray) -> np.ndarray:
    """Rodrigues: w (H, 3) rotation vectors -> (H, 3, 3)"""
    theta = np.linalg.norm(w, axis=1)
    k = w / np.where(theta > 0, theta, 1.0)[:, None]
    K = np.zeros((w.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(theta)[:, None, None] * K + (1.0 - np.cos(theta))[:, None, None] * (K @ K)


def draw_rotations(H: int, round: int, about=None, radius=None) -> np.ndarray:
    """(H, 3, 3) float64 rotations from a generator of its own seeded with (SEED, round): the global numpy RNG is not touched.  Round 0:
    index 0 is the identity, the rest are uniform over the rotations (unit quaternions from normalised 4-vectors of normals).  Round
    r >= 1: index 0 is `about` itself, bit for bit, the rest are exp([w]) about with w uniform in the ball of `radius` radians."""
    check_int("H", H, 1, MAX_HYPOTHESES)
    check_int("round", round, 0, 1 << 31)
    g = np.random.Generator(np.random.PCG64([SEED, int(round)]))
    if int(round) == 0:
        if about is not None or radius is not None:
            raise ValueError("round 0 covers every rotation: about and radius must be None")
        q = g.standard_normal((int(H), 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        out = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        out[0] = np.eye(3)
        return out
    about = np.asarray(about, np.float64) if about is not None else None
    if about is None or about.shape != (3, 3) or not is_real(radius) or not 0.0 < float(radius) <= math.pi:
        raise ValueError(f"round {round} draws about a 3 x 3 rotation within a radius in (0, pi], got {None if about is None else about.shape} and {radius!r}")
    d = g.standard_normal((int(H), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = _exp(d * (float(radius) * np.cbrt(g.random(int(H))))[:, None]) @ about
    out[0] = about
    return out


def radii(H: int, rounds: int) -> list:
    """The radius of every refinement round, derived from H alone.  Round 0 covers the rotations modulo the cube group, of Haar volume
    8 pi^2 / 24, with spacing s0 = (8 pi^2 / 24 / H)^(1/3); the first ball has twice that radius.  H draws in a ball of radius t have spacing
    t (4 pi / 3 / H)^(1/3), and every further ball has twice its predecessor's spacing as radius."""
    out, theta = [], 2.0 * (8.0 * math.pi ** 2 / 24.0 / H) ** (1.0 / 3.0)
    for _ in range(rounds):
        out.append(min(theta, math.pi))
        theta = 2.0 * theta * (4.0 * math.pi / 3.0 / H) ** (1.0 / 3.0)
    return out


def search(score, H: int, rounds: int = 4, min_gain: float = 0.02):
    """score(rot32 (H, 9) float32) -> (volumes (H) float64, best int): the box volume of every hypothesis, +inf for a bad one, and the index
    of the least, -1 if all are bad -> (R', V_identity, V_best).  Round 0 scores `draw_rotations(H, 0)`, whose index 0 is the identity:
    V_identity.  Round r = 1..rounds scores `draw_rotations(H, r, about=the best so far, radius=radii(H, rounds)[r - 1])`, whose index 0 is
    the best so far: its volume reproduces, so the best never gets worse.  The best is kept as the float64 matrix whose float32 rounding
    was scored.  Unless V_best < (1 - min_gain) V_identity the result is the identity: a ball has no orientation to find, and a random one
    would throw away the file's up.  Otherwise R' = nearest_representative(best)."""
    H, rounds, min_gain = check_align_args(H, rounds, min_gain)
    best_R, v_identity, v_best = np.eye(3), None, None
    for r, radius in enumerate([None] + radii(H, rounds)):
        rots = draw_rotations(H, r) if r == 0 else draw_rotations(H, r, about=best_R, radius=radius)
        volumes, best = score(np.ascontiguousarray(rots.reshape(H, 9), dtype=np.float32))
        volumes, best = np.asarray(volumes, np.float64), int(best)
        if r == 0:
            v_identity = float(volumes[0])
        if best < 0:                                                 # every hypothesis bad: nothing to go by
            return np.eye(3), v_identity, v_identity
        best_R, v_best = rots[best].copy(), float(volumes[best])
    if not v_best < (1.0 - min_gain) * v_identity:
        return np.eye(3), v_identity, v_best
    return nearest_representative(best_R), v_identity, v_best


def check_align_args(iters, rounds=4, min_gain=0.02) -> tuple:
    """The checks on (iters, rounds, min_gain); returns them as (int, int, float)."""
    check_int("iters", iters, MIN_ITERS, MAX_HYPOTHESES)
    check_int("rounds", rounds, 0, MAX_ROUNDS)
    if not is_real(min_gain) or not 0.0 <= float(min_gain) < 1.0:
        raise ValueError(f"min_gain must be in [0, 1), got {min_gain!r}")
    return int(iters), int(rounds), float(min_gain)


def _upload(array: np.ndarray, dev) -> torch.Tensor:
    """The one place `align_rows` moves an array to the device."""
    return torch.from_numpy(array).to(dev)


def align_rows(rows, iters, rounds, min_gain, uid: str, device="cuda"):
    """rows (N, >= 3) host array, xyz in the first three columns (uploaded as float32), normals in columns 3:6 when there are six or more
    -> (rows', (R', c)): c = the float32 bounding-box mid-point as float64, R' = `search` over `box_extents`; xyz' = c + (xyz - c) R'T and
    normals' = n R'T in float64, cast to the rows' dtype (float32 if that is narrower); further columns are copied.  When the search
    returns the identity, rows' is `rows` itself.  Prints the pose line of the command line."""
    iters, rounds, min_gain = check_align_args(iters, rounds, min_gain)
    rows = check_host_cloud(rows, "alignment", 1)
    dev = cuda_device(device, "align_rows")
    xyz32 = np.ascontiguousarray(rows[:, :3], dtype=np.float32)
    c32 = (xyz32.min(axis=0) + xyz32.max(axis=0)) / np.float32(2)
    hypotheses = iters * (rounds + 1)
    pts = _upload(xyz32, dev)

    def score(rot32):
        got = box_extents(pts, _upload(rot32, dev), c32)
        return got["volumes"].cpu().numpy(), int(got["best"].item())
    R, v_identity, v_best = search(score, iters, rounds, min_gain)
    c = c32.astype(np.float64)
    if np.array_equal(R, np.eye(3)):
        print(f"{uid}: alignment kept the file's axes: best box volume {v_best:.6g} against {v_identity:.6g}, gain under {min_gain:g}, {hypotheses} hypotheses")
        return rows, (R, c)
    out = rows.astype(np.float32) if rows.dtype.itemsize < 4 else rows.copy()
    out[:, :3] = (c[None, :] + (rows[:, :3].astype(np.float64) - c[None, :]) @ R.T).astype(out.dtype)
    if rows.shape[1] >= 6:
        out[:, 3:6] = (rows[:, 3:6].astype(np.float64) @ R.T).astype(out.dtype)
    angle = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    axis /= np.linalg.norm(axis) or 1.0
    print(f"{uid}: alignment turned the cloud {angle:.3f} deg about ({axis[0]:+.4f} {axis[1]:+.4f} {axis[2]:+.4f}): box volume {v_identity:.6g} -> {v_best:.6g}, "
          f"{hypotheses} hypotheses")
    return out, (R, c)
