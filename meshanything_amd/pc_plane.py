"""Dominant-plane removal of input clouds (`--plane_threshold`): find the plane that holds the most rows by RANSAC, refit it to its
inliers, drop them; PCL's SACSegmentation followed by an extraction of the outliers is the same operation.

A scanned object stands on a table or a floor.  That support is locally as dense as the object, so the statistical outlier filter keeps
it, and it touches the object, so Euclidean clustering returns "object + table" as one part however small the radius.  `score_planes`
and `apply_plane` are the two calls into the HIP library (csrc/pc_plane.hpp; C ABI ma_op_pc_plane_score / ma_op_pc_plane_apply, whose
header comment states the inlier rule): the first counts, for up to 2^16 plane hypotheses given as row triples, the rows within the
threshold of each, in integers that equal a numpy float32 restatement; the second gives one plane's inlier mask, count and float64
moments.  `draw_triples` draws the hypotheses from a private generator, `fit_plane` refits on the host, `remove_planes` is the loop
`data.Dataset` calls.  They need CUDA tensors; there is no CPU fallback.  There is no reference counterpart.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .pc_common import MAX_POINTS, check_device_cloud, check_host_cloud, check_int, check_want, cuda_device, is_real, need_cuda, upload_xyz

MAX_HYPOTHESES = 1 << 16                                         # MA_PC_PLANE_MAX_HYPOTHESES
MAX_COUNT = 8                                                    # planes removed from one cloud
SCORE_WANT = ("planes", "counts", "best")
APPLY_WANT = ("mask", "count", "moments")
SEED = 0x706c616e65                                              # "plane"


def check_threshold(threshold) -> float:
    if not is_real(threshold) or not (0.0 < float(threshold) < float("inf")):
        raise ValueError(f"threshold must be finite and > 0, got {threshold!r}")
    if not np.isfinite(np.float32(threshold)) or not np.float32(threshold) > 0:
        raise ValueError(f"threshold must be a positive finite float32, got {threshold!r}")
    return float(threshold)


def score_planes(points: torch.Tensor, triples: torch.Tensor, threshold, want=("counts", "best")):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns; triples (H, 3) int32 on the same device, the rows (i, j, k)
    that span hypothesis h -> a dict with the entries named in `want`: "planes" (H, 6) float32, the point p_i and the normal
    (p_j - p_i) x (p_k - p_i) in float32; "counts" (H) int32, the rows within `threshold` of the plane under the inlier rule of
    ma_op_pc_plane_score, -1 for a degenerate hypothesis (a repeated or out-of-range index, collinear rows); "best" (1) int32, the
    hypothesis of the greatest count, the lowest index among equals, -1 if all are degenerate.  Equal to the numpy restatement and to a
    second run, bit for bit."""
    threshold = check_threshold(threshold)
    check_device_cloud(points, 3)
    want = check_want(want, SCORE_WANT)
    if not torch.is_tensor(triples) or triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype != torch.int32:
        raise ValueError(f"triples must be a (H, 3) int32 tensor, got {tuple(triples.shape) if hasattr(triples, 'shape') else type(triples).__name__}"
                         f" {getattr(triples, 'dtype', '')}")
    if not 1 <= triples.shape[0] <= MAX_HYPOTHESES:
        raise ValueError(f"need 1 <= H <= 2^16 hypotheses, got H = {triples.shape[0]}")
    need_cuda(points, "score_planes")
    if triples.device != points.device:
        raise ValueError(f"score_planes runs on the GPU: triples must be on the points' device {points.device}, got {triples.device}")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref, tri = points.contiguous(), triples.contiguous()
        N, H = ref.shape[0], tri.shape[0]
        nbytes = lib.ma_pc_plane_workspace_bytes(N, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        planes = torch.empty((H, 6), dtype=torch.float32, device=dev) if "planes" in want else None
        counts = torch.empty(H, dtype=torch.int32, device=dev)
        best = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.ma_op_pc_plane_score(ref.data_ptr(), N, ref.shape[1], tri.data_ptr(), H, threshold, None if planes is None else planes.data_ptr(),
                                            counts.data_ptr(), best.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = {"planes": planes, "counts": counts, "best": best}
    return {w: out[w] for w in SCORE_WANT if w in want}


def _check_plane(plane) -> np.ndarray:
    try:
        plane = np.asarray(plane.detach().cpu() if torch.is_tensor(plane) else plane, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"plane must be six numbers, a point and a normal, got {plane!r}") from None
    if plane.shape != (6,):
        raise ValueError(f"plane must be six numbers, a point and a normal, got shape {plane.shape}")
    return np.ascontiguousarray(plane)


def apply_plane(points: torch.Tensor, plane, threshold, want=("mask",)):
    """points as for `score_planes`; plane: six host numbers, a point a and a normal n of any length (cast to float32) -> a dict with the
    entries named in `want`: "mask" (N) uint8, 1 = within `threshold` of the plane under the inlier rule; "count" (1) int32, its sum;
    "moments" (10) float64 over the inliers with q = p - a in float64: n, the sums of q and of the six products q qT (xx, xy, xz, yy, yz,
    zz), from a reduction of fixed shape: the same bits on every run, within n * 2^-52 * sum|term| of any other summation order."""
    threshold = check_threshold(threshold)
    check_device_cloud(points, 3)
    want = check_want(want, APPLY_WANT)
    plane = _check_plane(plane)
    need_cuda(points, "apply_plane")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        N = ref.shape[0]
        nbytes = lib.ma_pc_plane_workspace_bytes(N, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mask = torch.empty(N, dtype=torch.uint8, device=dev) if "mask" in want else None
        count = torch.empty(1, dtype=torch.int32, device=dev) if "count" in want else None
        moments = torch.empty(10, dtype=torch.float64, device=dev) if "moments" in want else None
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        _lib.check(lib.ma_op_pc_plane_apply(ref.data_ptr(), N, ref.shape[1], (C.c_float * 6)(*plane.tolist()), threshold, ptr(mask), ptr(count), ptr(moments),
                                            ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = {"mask": mask, "count": count, "moments": moments}
    return {w: out[w] for w in APPLY_WANT if w in want}


def draw_triples(N: int, iters: int, round: int) -> np.ndarray:
    """(iters, 3) int32 rows in [0, N), from a generator of its own seeded with (SEED, round): the global numpy RNG is not touched, so the
    uniform draw of `Dataset` that follows sees the state it would have seen.  Repeated indices are allowed; they score as degenerate."""
    for name, v, lo, hi in (("N", N, 1, MAX_POINTS), ("iters", iters, 1, MAX_HYPOTHESES), ("round", round, 0, 1 << 31)):
        check_int(name, v, lo, hi)
    return np.random.Generator(np.random.PCG64([SEED, int(round)])).integers(0, int(N), (int(iters), 3)).astype(np.int32)


def fit_plane(moments, a):
    """moments (10) float64 of `apply_plane`, a (3) the point they are taken about -> (c (3), n (3)) float32: the least-squares plane of
    the inliers, c = a + S1 / n their centroid, n the unit eigenvector of the least eigenvalue of the covariance S2 / n - m mT
    (np.linalg.eigh, float64).  Moments of no rows, or non-finite ones: a zero normal, which is a degenerate plane."""
    m = np.asarray(moments, np.float64)
    a = np.asarray(a, np.float64)
    if m.shape != (10,) or a.shape != (3,):
        raise ValueError(f"moments must be (10) and a (3), got {m.shape} and {a.shape}")
    if not (np.isfinite(m).all() and np.isfinite(a).all() and m[0] >= 1):
        return a.astype(np.float32), np.zeros(3, np.float32)
    mean = m[1:4] / m[0]
    s2 = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]) / m[0]
    _, vec = np.linalg.eigh(s2 - np.outer(mean, mean))
    return (a + mean).astype(np.float32), vec[:, 0].astype(np.float32)


def check_remove_args(threshold, iters, count, min_fraction) -> tuple:
    """The checks on (threshold, iters, count, min_fraction); returns them as (float, int, int, float)."""
    threshold = check_threshold(threshold)
    check_int("iters", iters, 1, MAX_HYPOTHESES)
    check_int("count", count, 1, MAX_COUNT)
    if not is_real(min_fraction) or not 0.0 < float(min_fraction) <= 1.0:
        raise ValueError(f"min_fraction must be in (0, 1], got {min_fraction!r}")
    return threshold, int(iters), int(count), float(min_fraction)


def remove_planes(xyz, threshold, iters, count, min_fraction, n_points, uid: str, device="cuda"):
    """xyz (N, >= 3) host array, only the first three columns are read (uploaded as float32) -> the row indices (int64, in file order)
    that are left after up to `count` rounds.  Round r, over the rows still kept: `draw_triples(rows, iters, r)`, `score_planes`, the best
    hypothesis; stop if there is none or it holds fewer than min_fraction of the round's rows; `apply_plane` with moments, `fit_plane`,
    `apply_plane` of the refitted plane; of the two planes the one with more inliers, the unrefitted one on a tie (integers decide), loses
    its inliers.  Prints the plane line of the command line.  Fewer than n_points rows left is a ValueError naming the uid and the
    number."""
    threshold, iters, count, min_fraction = check_remove_args(threshold, iters, count, min_fraction)
    xyz = check_host_cloud(xyz, "plane removal", 3)
    dev = cuda_device(device, "remove_planes")
    N = xyz.shape[0]
    kept = np.arange(N, dtype=np.int64)
    found, stopped = [], None
    with torch.cuda.device(dev):
        pts = upload_xyz(xyz, dev)
        for r in range(count):
            rows = pts.shape[0]
            if rows < 3:
                break
            tri = torch.from_numpy(draw_triples(rows, iters, r)).to(dev)
            got = score_planes(pts, tri, threshold, want=SCORE_WANT)
            best = int(got["best"].item())
            if best < 0 or int(got["counts"][best].item()) < min_fraction * rows:
                stopped = f"no plane of at least {min_fraction:g} of the rows found"
                break
            plane = got["planes"][best].cpu().numpy()
            first = apply_plane(pts, plane, threshold, want=APPLY_WANT)
            refit = np.concatenate(fit_plane(first["moments"].cpu().numpy(), plane[:3]))
            second = apply_plane(pts, refit, threshold, want=("mask", "count"))
            if int(second["count"].item()) > int(first["count"].item()):
                plane, first = refit, second
            mask = first["mask"].bool()
            normal = plane[3:].astype(np.float64)
            normal /= np.linalg.norm(normal) * (1.0 if normal[np.argmax(np.abs(normal))] > 0 else -1.0)   # printed with its largest component positive
            found.append((int(first["count"].item()), normal))
            kept = kept[~mask.cpu().numpy()]
            pts = pts[~mask].contiguous()
    parts = [f"{c} inliers, normal ({n[0]:+.4f} {n[1]:+.4f} {n[2]:+.4f})" for c, n in found] + ([stopped] if stopped else [])
    print(f"{uid}: plane removal (threshold {threshold:g}) removed {len(found)} plane{'' if len(found) == 1 else 's'}: {'; '.join(parts) or 'none'}, "
          f"dropped {N - kept.shape[0]} of {N} points")
    if kept.shape[0] < n_points:
        raise ValueError(f"{uid}: plane removal left {kept.shape[0]} points, fewer than the {n_points} the encoder takes")
    return kept
