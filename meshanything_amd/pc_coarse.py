"""Coarse registration of a scan from an UNKNOWN pose (`--coarse_radius`), the stage in front of `pc_register.icp`;
PCL's FPFHEstimation + SampleConsensusPrerejective and Open3D's compute_fpfh_feature + registration_ransac_based_on_feature_matching do
the same job.

ICP only works when a scan already lies within its pairing distance of its place; a turntable without an encoder, a hand-held scanner
and files exported one by one deliver scans in arbitrary frames.  `spfh`, `spfh_gather`, `desc_match` and `pose_score` are the four calls
into the HIP library (csrc/pc_coarse.hpp; C ABI ma_op_pc_spfh, _spfh_gather, _desc_match, _pose_score, whose header comment states the
rules): a sign-free point feature histogram over every row's radius neighbourhood, its second pass at the keypoints, the nearest
descriptor of one set in another, and the number of matched pairs that agree with each of H pose hypotheses.  Their integer outputs
equal a numpy float32 restatement byte for byte.  The rest is host numpy in float64: `mutual_matches`, `draw_triples` from a private
generator (the global numpy RNG is untouched), `prune_triples` (Open3D's edge-length check), the batched `kabsch`, and `coarse_pose`,
which `pc_register.register_rows` calls per scan when the stage is on.  It needs CUDA tensors; there is no CPU fallback.  There is no
reference counterpart.  Out of reach: a solid of large flat faces or near symmetry, whose descriptors all look alike and whose
half-turn twin overlaps as well as the truth; loop closure, colour, non-rigid motion.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_cluster import check_max_pairs, check_pair_bound, check_radius, check_radius_grid, grid_workspace
from .pc_common import check_device_cloud, check_int, is_real, need_cuda

BINS, DESC, COLS, MAX_USED = 11, 33, 34, 65535                  # MA_PC_SPFH_BINS, _DESC, _COLS, _MAX_USED
MAX_QUERIES = 1 << 20                                            # MA_PC_SPFH_MAX_QUERIES
MAX_KEYPOINTS, MAX_HYPOTHESES = 4096, 1 << 16                    # MA_PC_COARSE_MAX_KEYPOINTS, _MAX_HYPOTHESES
MIN_KEYPOINTS, MIN_HYPOTHESES = 64, 256
DEFAULT_POINTS, DEFAULT_ITERS = 1024, 4096
MIN_MUTUAL = 16                                                  # fewer mutual matches: every source -> target match is kept
MIN_AGREE = 4                                                    # a hypothesis is three pairs; a fourth must agree
EDGE_RATIO = 0.9                                                 # Open3D's CorrespondenceCheckerBasedOnEdgeLength
SEED = 0x636f61727365                                            # "coarse"


# ---- the ops ---------------------------------------------------------------------------------------------------------------------------
def _normals_of(points: torch.Tensor, normals):
    """-> (pointer, ld, the tensor to keep alive): "cloud" = columns 3:6 of a six-column cloud, or a (N, >= 3) float32 tensor"""
    if isinstance(normals, str):
        if normals != "cloud" or points.shape[1] != 6:
            raise ValueError('normals="cloud" needs a six-column cloud; pass a (N, >= 3) float32 tensor')
        return points.data_ptr() + 12, 6, None
    if not torch.is_tensor(normals) or normals.dim() != 2 or normals.shape[0] != points.shape[0] or normals.shape[1] < 3 or normals.dtype != torch.float32 or normals.device != points.device:
        raise ValueError(f"normals must be a (N = {points.shape[0]}, >= 3) float32 tensor on the cloud's device")
    keep = normals.contiguous()
    return keep.data_ptr(), keep.shape[1], keep


def spfh(points: torch.Tensor, radius, normals="cloud", grid=None, max_pairs=None) -> torch.Tensor:
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns; normals: "cloud" = its columns 3:6, or a (N, >= 3) float32
    tensor -> hist (N, 34) int64 holding uint32 values (ma_op_pc_spfh): per row three histograms of 11 bins over the rows within
    `radius` of it, of |n_p . D| / |D|, |n_q . D| / |D| and |n_p . n_q|, and in column 33 the pairs used.  grid: (origin, cell, dims) with
    radius / cell <= 8, None = `pc_cluster.choose_cluster_grid`; the result does not depend on it.  More than 65 535 used pairs in one
    row, or a pair bound above max_pairs, is a ValueError."""
    radius = check_radius(radius)
    check_device_cloud(points, 1)
    cap = check_max_pairs(max_pairs)
    grid = check_radius_grid(grid, radius)
    need_cuda(points, "spfh")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        N = ref.shape[0]
        nptr, nld, keep = _normals_of(ref, normals)
        grid_args, ws, nbytes = grid_workspace(lib, "spfh", ref, radius, grid)
        hist = torch.empty((N, COLS), dtype=torch.int32, device=dev)
        bound, most = C.c_uint64(0), C.c_uint32(0)
        rc = lib.ma_op_pc_spfh(ref.data_ptr(), N, ref.shape[1], nptr, nld, radius, *grid_args, cap, hist.data_ptr(), C.byref(bound), C.byref(most), ws.data_ptr(),
                               nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        check_pair_bound("spfh", rc, bound.value, cap, N, radius)
        if rc != _lib.MA_OK and most.value > MAX_USED:
            raise ValueError(f"spfh: a row has {most.value} neighbours within the radius {radius}, more than {MAX_USED}: thin the scans with --voxel_size "
                             "or use a smaller --coarse_radius")
        _lib.check(rc)
        del keep
    return hist.to(torch.int64) & 0xFFFFFFFF


def _as_u32(t: torch.Tensor, cols: int, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != cols or t.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"{name} must be a (rows, {cols}) integer tensor")
    return (t.to(torch.int64) & 0xFFFFFFFF).to(torch.int32) if t.dtype == torch.int64 else t.contiguous()      # the low 32 bits: the uint32 the library reads


def spfh_gather(points: torch.Tensor, hist: torch.Tensor, radius, query: torch.Tensor, grid=None, max_pairs=None) -> torch.Tensor:
    """The same cloud, radius and (any) grid, `spfh`'s hist and query (Q) integer rows of the cloud, 1 <= Q <= 2^20, repeats allowed ->
    desc (Q, 33) int64 holding uint32 values: hist[p] + the sum of hist[q] over the rows q within the radius of p, as integers
    (ma_op_pc_spfh_gather)."""
    radius = check_radius(radius)
    check_device_cloud(points, 1)
    cap = check_max_pairs(max_pairs)
    grid = check_radius_grid(grid, radius)
    need_cuda(points, "spfh_gather")
    N = points.shape[0]
    h = _as_u32(hist, COLS, "hist")
    if h.shape[0] != N or h.device != points.device:
        raise ValueError(f"hist must have the cloud's {N} rows and lie on its device")
    if not torch.is_tensor(query) or query.dim() != 1 or query.dtype not in (torch.int32, torch.int64) or not 1 <= query.shape[0] <= MAX_QUERIES:
        raise ValueError("query must be a (Q) integer tensor, 1 <= Q <= 2^20")
    q = query.to(points.device)
    if int(q.min()) < 0 or int(q.max()) >= N:
        raise ValueError(f"query must hold rows in [0, {N})")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref, q = points.contiguous(), q.to(torch.int32).contiguous()
        grid_args, ws, nbytes = grid_workspace(lib, "spfh", ref, radius, grid)
        desc = torch.empty((q.shape[0], DESC), dtype=torch.int32, device=dev)
        bound = C.c_uint64(0)
        rc = lib.ma_op_pc_spfh_gather(ref.data_ptr(), N, ref.shape[1], radius, *grid_args, cap, h.data_ptr(), q.data_ptr(), q.shape[0], desc.data_ptr(),
                                      C.byref(bound), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        check_pair_bound("spfh_gather", rc, bound.value, cap, N, radius)
        _lib.check(rc)
    return desc.to(torch.int64) & 0xFFFFFFFF


def desc_match(A: torch.Tensor, B: torch.Tensor):
    """A (Ka, 33), B (Kb, 33) integer descriptors on one GPU, 1 <= Ka, Kb <= 4096 -> (idx (Ka) int32, dist (Ka) float32): for every row of
    A the row of B least in (distance, index) between the descriptors, each block of 11 normalised by its sum (ma_op_pc_desc_match)."""
    a, b = _as_u32(A, DESC, "A"), _as_u32(B, DESC, "B")
    if not (1 <= a.shape[0] <= MAX_KEYPOINTS and 1 <= b.shape[0] <= MAX_KEYPOINTS):
        raise ValueError(f"desc_match takes 1..{MAX_KEYPOINTS} rows a side, got {a.shape[0]} and {b.shape[0]}")
    need_cuda(a, "desc_match")
    if b.device != a.device:
        raise ValueError("desc_match: A and B must be on one device")
    lib = _lib.load()
    with torch.cuda.device(a.device):
        idx = torch.empty(a.shape[0], dtype=torch.int32, device=a.device)
        dist = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
        _lib.check(lib.ma_op_pc_desc_match(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], idx.data_ptr(), dist.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return idx, dist


def pose_score(poses: torch.Tensor, P: torch.Tensor, Q: torch.Tensor, dist):
    """poses (H, 12) float32, R row-major then t, 1 <= H <= 2^16; P, Q (C, 3) float32, 1 <= C <= 4096, all on one GPU -> (counts (H) int32,
    best (1) int32): the pairs i with |R P_i + t - Q_i| <= dist by the float32 rule of ma_op_pc_register_step, and the hypothesis of the
    highest count, the lowest index among equals (ma_op_pc_pose_score)."""
    dist = check_radius(dist)
    for name, t, cols in (("poses", poses, 12), ("P", P, 3), ("Q", Q, 3)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != cols or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a (rows, {cols}) float32 tensor")
    if not 1 <= poses.shape[0] <= MAX_HYPOTHESES or not 1 <= P.shape[0] <= MAX_KEYPOINTS or Q.shape[0] != P.shape[0]:
        raise ValueError(f"pose_score takes 1..{MAX_HYPOTHESES} poses and 1..{MAX_KEYPOINTS} pairs, P and Q of one length")
    need_cuda(poses, "pose_score")
    if P.device != poses.device or Q.device != poses.device:
        raise ValueError("pose_score: poses, P and Q must be on one device")
    lib = _lib.load()
    with torch.cuda.device(poses.device):
        h, p, q = poses.contiguous(), P.contiguous(), Q.contiguous()
        counts = torch.empty(h.shape[0], dtype=torch.int32, device=h.device)
        best = torch.empty(1, dtype=torch.int32, device=h.device)
        _lib.check(lib.ma_op_pc_pose_score(h.data_ptr(), h.shape[0], p.data_ptr(), q.data_ptr(), p.shape[0], dist, counts.data_ptr(), best.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return counts, best


class DeviceOps:
    """The five device steps of `coarse_pose` on host arrays: what the host tests replace by the numpy restatement."""

    def __init__(self, device):
        self.device = device

    def keypoints(self, xyz: np.ndarray, k: int) -> np.ndarray:
        from .pc_fps import farthest_point_sample
        return farthest_point_sample(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(self.device), k)[0].cpu().numpy().astype(np.int64)

    def describe(self, xyz: np.ndarray, normals: np.ndarray, radius: float, query: np.ndarray) -> np.ndarray:
        cloud = torch.from_numpy(np.ascontiguousarray(np.concatenate([xyz, normals], 1), np.float32)).to(self.device)
        hist = spfh(cloud, radius)
        return spfh_gather(cloud, hist, radius, torch.from_numpy(query).to(self.device)).cpu().numpy()

    def match(self, A: np.ndarray, B: np.ndarray) -> np.ndarray:
        return desc_match(torch.from_numpy(A).to(self.device), torch.from_numpy(B).to(self.device))[0].cpu().numpy().astype(np.int64)

    def score(self, poses: np.ndarray, P: np.ndarray, Q: np.ndarray, dist: float):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)    # noqa: E731
        counts, best = pose_score(up(poses), up(P), up(Q), dist)
        return counts.cpu().numpy(), int(best.cpu()[0])


# ---- the host side: float64 throughout ---------------------------------------------------------------------------------------------------
def check_coarse_args(radius, points, iters, dist) -> tuple:
    """The checks on the options; returns them as (float, int, int, float), dist None = radius / 4."""
    radius = check_radius(radius)
    points = check_int("coarse_points", points, MIN_KEYPOINTS, MAX_KEYPOINTS)
    iters = check_int("coarse_iters", iters, MIN_HYPOTHESES, MAX_HYPOTHESES)
    if dist is None:
        dist = radius / 4.0
    if not is_real(dist) or not 0.0 < float(dist) < float("inf") or not np.isfinite(np.float32(dist)) or not np.float32(dist) > 0:
        raise ValueError(f"coarse_dist must be finite and > 0, got {dist!r}")
    return radius, points, iters, float(dist)


def mutual_matches(ab, ba) -> np.ndarray:
    """ab (Ka): the row of B nearest every row of A; ba (Kb): the other way -> (C, 2) int64, the pairs (a, ab[a]) with ba[ab[a]] == a, in
    the order of a; with fewer than MIN_MUTUAL of them, every (a, ab[a])."""
    ab, ba = np.asarray(ab, np.int64), np.asarray(ba, np.int64)
    a = np.arange(ab.shape[0], dtype=np.int64)
    keep = ba[ab] == a
    if int(keep.sum()) < MIN_MUTUAL:
        keep = np.ones_like(keep)
    return np.stack([a[keep], ab[keep]], 1)


def draw_triples(C_: int, H: int, seed: int = SEED) -> np.ndarray:
    """(H, 3) int64 in [0, C): H triples of matches from a generator of its own; the global numpy RNG is untouched."""
    return np.random.Generator(np.random.PCG64(seed)).integers(0, C_, (H, 3), dtype=np.int64)


def prune_triples(triples, P, Q, dist) -> np.ndarray:
    """triples (H, 3) into the matched points P, Q (C, 3) -> the triples kept, in order: no index twice, every edge of either triangle at
    least 2 * dist long, and corresponding edges within a factor EDGE_RATIO of each other."""
    t = np.asarray(triples, np.int64)
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    keep = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    for a, b in ((0, 1), (1, 2), (0, 2)):
        lp = np.linalg.norm(P[t[:, a]] - P[t[:, b]], axis=1)
        lq = np.linalg.norm(Q[t[:, a]] - Q[t[:, b]], axis=1)
        keep &= (lp >= 2.0 * dist) & (lq >= 2.0 * dist) & (np.minimum(lp, lq) >= EDGE_RATIO * np.maximum(lp, lq))
    return t[keep]


def kabsch(P, Q):
    """P, Q (..., n, 3) -> (R (..., 3, 3), t (..., 3)) float64, the rigid motions that minimise sum |R P_i + t - Q_i|^2, batched: np.linalg.svd
    of the cross-covariance, the last singular direction flipped where the product would be a reflection."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    mp, mq = P.mean(-2, keepdims=True), Q.mean(-2, keepdims=True)
    Hm = np.swapaxes(P - mp, -1, -2) @ (Q - mq)
    U, _, Vt = np.linalg.svd(Hm)
    V, Ut = np.swapaxes(Vt, -1, -2), np.swapaxes(U, -1, -2)
    d = np.where(np.linalg.det(V @ Ut) < 0, -1.0, 1.0)
    D = np.zeros(Hm.shape)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    R = V @ D @ Ut
    return R, mq[..., 0, :] - (R @ mp[..., 0, :, None])[..., 0]


def poses12(R, t) -> np.ndarray:
    """(H, 3, 3), (H, 3) float64 -> (H, 12) float32: what the kernel takes."""
    return np.concatenate([np.asarray(R, np.float64).reshape(-1, 9), np.asarray(t, np.float64).reshape(-1, 3)], 1).astype(np.float32)


def agreeing(pose12, P, Q, dist) -> np.ndarray:
    """The pairs ma_op_pc_pose_score counts for one pose, by its float32 rule with every rounding explicit -> (C) bool."""
    f = np.float32
    pose, P, Q = np.asarray(pose12, f), np.asarray(P, f), np.asarray(Q, f)
    with np.errstate(all="ignore"):
        d = []
        for a in range(3):
            s = (pose[3 * a] * P[:, 0]).astype(f) + (pose[3 * a + 1] * P[:, 1]).astype(f)
            s = s.astype(f) + (pose[3 * a + 2] * P[:, 2]).astype(f)
            d.append((s.astype(f) + pose[9 + a]).astype(f) - Q[:, a])
        key = ((d[0] * d[0]).astype(f) + (d[1] * d[1]).astype(f)).astype(f) + (d[2] * d[2]).astype(f)
        return key <= f(f(dist) * f(dist))


def coarse_pose(target, target_normals, source, source_normals, radius, points: int = DEFAULT_POINTS, iters: int = DEFAULT_ITERS, dist=None, ops=None,
                scan="?", uid: str = "?", seed: int = SEED):
    """target (N, 3), source (M, 3) host arrays with their (unoriented) unit normals -> dict(pose (R, t) float64 with R source + t on the
    target, mutual, triples, count, angle).  In this order: min(points, rows) farthest-point keypoints on both clouds; the histograms
    over all rows and the descriptors at the keypoints; the nearest descriptor both ways and the mutual matches (`mutual_matches`);
    `iters` triples of matches from a private generator; `prune_triples`; the batched `kabsch` of the survivors, cast to float32, and
    their agreement counts over ALL matches within `dist` (None = radius / 4); `kabsch` again over the matches that agree with the
    best.  Fewer than 3 matches, no surviving triple or a best count below MIN_AGREE is a ValueError that names scan and uid: a refusal
    beats a silently wrong merge.  ops: the device steps (`DeviceOps`)."""
    radius, points, iters, dist = check_coarse_args(radius, points, iters, dist)
    tx, sx = np.asarray(target, np.float32)[:, :3], np.asarray(source, np.float32)[:, :3]
    tn, sn = np.asarray(target_normals, np.float32)[:, :3], np.asarray(source_normals, np.float32)[:, :3]
    kt, ks = ops.keypoints(tx, min(points, tx.shape[0])), ops.keypoints(sx, min(points, sx.shape[0]))
    dt, ds = ops.describe(tx, tn, radius, kt), ops.describe(sx, sn, radius, ks)
    pairs = mutual_matches(ops.match(ds, dt), ops.match(dt, ds))
    if pairs.shape[0] < 3:
        raise ValueError(f"{uid}: coarse registration of scan {scan} found {pairs.shape[0]} matches, fewer than the 3 a pose takes: is --coarse_radius "
                         "several point spacings wide?")
    P, Q = sx[ks[pairs[:, 0]]].astype(np.float64), tx[kt[pairs[:, 1]]].astype(np.float64)
    triples = prune_triples(draw_triples(pairs.shape[0], iters, seed), P, Q, dist)
    if triples.shape[0] == 0:
        raise ValueError(f"{uid}: coarse registration of scan {scan}: none of {iters} triples of its {pairs.shape[0]} matches has edges of matching "
                         "length: do the scans overlap, and is --coarse_dist small against the object?")
    R, t = kabsch(P[triples], Q[triples])
    hyp = poses12(R, t)
    counts, best = ops.score(hyp, P, Q, dist)
    count = int(counts[best])
    if count < MIN_AGREE:
        raise ValueError(f"{uid}: coarse registration of scan {scan}: the best of {triples.shape[0]} hypotheses agrees with {count} matches, fewer than "
                         f"{MIN_AGREE}: do the scans overlap?")
    agree = agreeing(hyp[best], P, Q, dist)
    R, t = kabsch(P[agree], Q[agree]) if int(agree.sum()) >= 3 else (R[best], t[best])
    angle = math.degrees(math.acos(min(max((np.trace(R) - 1.0) / 2.0, -1.0), 1.0)))
    return {"pose": (R, t), "mutual": int(pairs.shape[0]), "triples": int(triples.shape[0]), "count": count, "angle": angle}
