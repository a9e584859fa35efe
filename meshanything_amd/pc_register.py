"""Registration of the partial scans of one object (`--register_dist`): iterative closest point, scan by scan, onto the union of the scans
before; PCL's registration module and Open3D's registration_icp do the same job.

A scanner, a depth camera on a turntable or a photogrammetry rig delivers several scans per object, each in its own, roughly known, pose;
every other input step assumes one file in one frame.  `build` and `icp_step` are the two calls into the HIP library (csrc/pc_register.hpp;
C ABI ma_op_pc_register_build / ma_op_pc_register_step, whose header comment states the rule): the nearest target row within the distance
for every transformed source row, over the cell grid of the other cloud ops, and 32 float64 sums over the pairs, formed in a fixed order
so that they are the same on every run.  The rest is host numpy in float64: `solve_plane` (point-to-plane, the metric of the feature: flat
faces do not resist sliding along themselves), `solve_point` (Kabsch, for clouds without usable normals), `compose`, the loop `icp` over a
callable pose -> sums, and `register_rows`, which `data.Dataset` calls.  The poses are composed in float64 and applied to the ORIGINAL
source rows every time, so no error accumulates in the points.  It needs CUDA tensors; there is no CPU fallback.  There is no reference
counterpart.  Scans in unknown poses: `register_rows(..., coarse=...)` puts `pc_coarse.coarse_pose` in front of every scan's ICP
(`--coarse_radius`).  Out of scope: loop closure, colour, non-rigid motion, mesh inputs.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .pc_cluster import check_max_pairs, check_radius, check_radius_grid, choose_cluster_grid, MAX_PAIRS
from .pc_common import MAX_POINTS, MAX_QUERIES, as_host_cloud, check_device_cloud, check_finite, check_int, check_want, cuda_device, is_real, need_cuda

SUMS, THREADS, ROWS_PER_THREAD = 32, 256, 16                     # MA_PC_REGISTER_SUMS, _THREADS, _ROWS_PER_THREAD
WANT = ("sums", "idx", "d2")
METRICS = ("plane", "point")
MIN_PAIRS = {"plane": 6, "point": 3}                             # the unknowns of a rigid motion against what one pair gives
MIN_ROWS = 64                                                    # the fewest rows of a scan
MAX_ITERS = 256
IDENTITY = (np.eye(3), np.zeros(3))


# ---- the op ----------------------------------------------------------------------------------------------------------------------------
class Built:
    """What `build` leaves for `icp_step`: both clouds on the device, the grid's ctypes arguments and the filled workspace."""

    def __init__(self, target, source, grid_args, ws, nbytes):
        self.target, self.source, self.grid_args, self.ws, self.nbytes = target, source, grid_args, ws, nbytes


def build(target: torch.Tensor, source: torch.Tensor, dist, grid=None) -> Built:
    """target (N, 3 | 6) and source (M, 3 | 6) float32 on one GPU, xyz in the first three columns, 1 <= N, M <= 2^22 -> the binned clouds
    (ma_op_pc_register_build).  grid: (origin, cell, dims) with dist / cell <= 8, None = `pc_cluster.choose_cluster_grid` of the target
    (copied to the host for it) and dist.  The grid only decides the time."""
    dist = check_radius(dist)
    check_device_cloud(target, 1)
    check_device_cloud(source, 1)
    grid = check_radius_grid(grid, dist)
    need_cuda(target, "pc_register.build")
    if source.device != target.device:
        raise ValueError(f"pc_register.build runs on the GPU: source must be on the target's device {target.device}, got {source.device}")
    lib = _lib.load()
    with torch.cuda.device(target.device):
        tgt, src = target.contiguous(), source.contiguous()
        if grid is None:
            host = tgt[:, :3].cpu().numpy()
            check_finite(host)
            grid = choose_cluster_grid(host, dist)
        origin, cell, dims = grid
        nbytes = lib.ma_pc_register_workspace_bytes(tgt.shape[0], src.shape[0], int(dims[0]), int(dims[1]), int(dims[2]))
        if nbytes == 0:
            raise ValueError(f"outside the limits of ma_op_pc_register_build: N = {tgt.shape[0]}, M = {src.shape[0]}, dims = {dims.tolist()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=tgt.device)
        grid_args = ((C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist()))
        _lib.check(lib.ma_op_pc_register_build(tgt.data_ptr(), tgt.shape[0], tgt.shape[1], src.data_ptr(), src.shape[0], src.shape[1], *grid_args,
                                               ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return Built(tgt, src, grid_args, ws, nbytes)


def _floats(name: str, v, n: int) -> np.ndarray:
    try:
        a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {n} numbers, got {v!r}") from None
    if a.shape != (n,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be {n} finite numbers, got shape {np.shape(v)}")
    return a


def icp_step(built: Built, pose, centre, dist, normals="target", want=("sums",), max_pairs=None):
    """One iteration's device work over `build`'s clouds (ma_op_pc_register_step).  pose: 12 numbers, R row-major then t (or (R, t)),
    cast to float32; centre: 3 numbers; dist: the pairing distance D.  normals: "target" = columns 3:6 of a six-column target (the
    plane metric), None = the point metric, or a (N, >= 3) float32 tensor on the device.  -> a dict with the entries named in `want`:
    "sums" (32) float64, "idx" (M) int32, the target row paired with every source row, -1 for none, and "d2" (M) float32, its key, +inf
    for none.  idx and d2 equal a brute force over all rows; the sums are bit-identical from run to run and grid to grid.  max_pairs:
    the cap on the pair bound the library computes before it searches (None = its own, 2^36); a bound above it is a ValueError that
    names both."""
    if not isinstance(built, Built):
        raise ValueError(f"built must come from pc_register.build, got {type(built).__name__}")
    dist = check_radius(dist)
    want = check_want(want, WANT)
    cap = check_max_pairs(max_pairs)
    if isinstance(pose, tuple) and len(pose) == 2:
        pose = np.concatenate([np.asarray(pose[0], np.float64).reshape(-1), np.asarray(pose[1], np.float64).reshape(-1)])
    pose, centre = _floats("pose", pose, 12), _floats("centre", centre, 3)
    tgt, src = built.target, built.source
    N, M = tgt.shape[0], src.shape[0]
    if isinstance(normals, str):
        if normals != "target" or tgt.shape[1] != 6:
            raise ValueError('normals="target" needs a six-column target; pass None for the point metric')
        nptr, nld, keep = tgt.data_ptr() + 12, 6, None
    elif normals is None:
        nptr, nld, keep = None, 0, None
    else:
        if not torch.is_tensor(normals) or normals.dim() != 2 or normals.shape[0] != N or normals.shape[1] < 3 or normals.dtype != torch.float32 or normals.device != tgt.device:
            raise ValueError(f"normals must be a (N = {N}, >= 3) float32 tensor on the target's device")
        keep = normals.contiguous()
        nptr, nld = keep.data_ptr(), keep.shape[1]
    lib = _lib.load()
    dev = tgt.device
    with torch.cuda.device(dev):
        out = {"sums": torch.empty(SUMS, dtype=torch.float64, device=dev) if "sums" in want else None,
               "idx": torch.empty(M, dtype=torch.int32, device=dev) if "idx" in want else None,
               "d2": torch.empty(M, dtype=torch.float32, device=dev) if "d2" in want else None}
        ptr = lambda w: None if out[w] is None else out[w].data_ptr()    # noqa: E731
        bound = C.c_uint64(0)
        rc = lib.ma_op_pc_register_step(tgt.data_ptr(), N, tgt.shape[1], src.data_ptr(), M, src.shape[1], *built.grid_args, (C.c_float * 12)(*pose.tolist()),
                                        (C.c_float * 3)(*centre.tolist()), dist, nptr, nld, cap, ptr("idx"), ptr("d2"), C.byref(bound), ptr("sums"),
                                        built.ws.data_ptr(), built.nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != _lib.MA_OK and bound.value > (cap or MAX_PAIRS):
            raise ValueError(f"icp_step: the pair bound {bound.value} exceeds max_pairs {cap or MAX_PAIRS} (N = {N}, M = {M}, dist {dist}): "
                             "use a smaller distance or fewer points")
        _lib.check(rc)
    return {w: out[w] for w in WANT if w in want}


# ---- the host side: float64 throughout ---------------------------------------------------------------------------------------------------
def exp_so3(w) -> np.ndarray:
    """The rotation about w by |w| radians, Rodrigues' formula with sin(a)/a and (1 - cos a)/a^2 = (sin(a/2)/(a/2))^2 / 2 evaluated without
    cancellation: orthonormal to rounding for every w."""
    w = np.asarray(w, np.float64).reshape(3)
    a = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    s = math.sin(a) / a if a > 0 else 1.0
    h = math.sin(a / 2) / (a / 2) if a > 0 else 1.0
    return np.eye(3) + s * K + (0.5 * h * h) * (K @ K)


def _sums(sums) -> np.ndarray:
    sums = np.asarray(sums, np.float64).reshape(-1)
    if sums.shape != (SUMS,):
        raise ValueError(f"sums must be {SUMS} numbers, got shape {sums.shape}")
    return sums


def solve_plane(sums, centre):
    """The plane metric's sums and their centre c -> the motion (dR, dt), p'' = dR p' + dt, that minimises sum (r + J . (w, v))^2, the
    residuals linearised about p': (sum J J^T)(w, v) = -sum J r by np.linalg.solve, dR = exp_so3(w) exactly, dt = c + v - dR c."""
    sums, c = _sums(sums), np.asarray(centre, np.float64).reshape(3)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[9:30]
    A = A + np.triu(A, 1).T
    try:
        x = np.linalg.solve(A, -sums[3:9])
    except np.linalg.LinAlgError:
        raise ValueError("the point-to-plane system is singular: the paired normals do not fix the motion") from None
    if not np.isfinite(x).all():
        raise ValueError("the point-to-plane system has no finite solution")
    dR = exp_so3(x[:3])
    return dR, c + x[3:] - dR @ c


def solve_point(sums, centre):
    """The point metric's sums and their centre c -> the rigid motion (dR, dt) that minimises sum |dR p' + dt - q|^2 over the pairs: Kabsch,
    np.linalg.svd of the cross-covariance, the determinant fixed so that dR is a rotation."""
    sums, c = _sums(sums), np.asarray(centre, np.float64).reshape(3)
    n = sums[0]
    if not n > 0:
        raise ValueError("no pairs")
    mp, mq = sums[2:5] / n, sums[5:8] / n
    H = sums[8:17].reshape(3, 3) - n * np.outer(mp, mq)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0
    dR = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return dR, c + mq - dR @ (c + mp)


def compose(pose, step):
    """(R, t) then (dR, dt) -> (dR R, dR t + dt), and one Newton step of the polar decomposition, R (3 I - R^T R) / 2, which takes the
    product's rounding off again: R stays orthonormal to a few 1e-16 over any number of steps."""
    R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    dR, dt = np.asarray(step[0], np.float64), np.asarray(step[1], np.float64)
    Rn = dR @ R
    Rn = 0.5 * Rn @ (3.0 * np.eye(3) - Rn.T @ Rn)
    return Rn, dR @ t + dt


def pose12(pose) -> np.ndarray:
    """(R, t) float64 -> the 12 float32 the kernel takes."""
    return np.concatenate([np.asarray(pose[0], np.float64).reshape(9), np.asarray(pose[1], np.float64).reshape(3)]).astype(np.float32)


def apply_pose(rows, pose, normals: bool = True) -> np.ndarray:
    """rows (N, >= 3) host array, pose (R, t) -> a copy in rows' dtype with xyz replaced by R x + t, computed in float64, and, with
    `normals` and six columns or more, columns 3:6 by R n: the normals turn with the points.  Every other column is kept."""
    R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64)
    out = rows.copy()
    out[:, :3] = (rows[:, :3].astype(np.float64) @ R.T + t).astype(rows.dtype)
    if normals and rows.shape[1] >= 6:
        out[:, 3:6] = (rows[:, 3:6].astype(np.float64) @ R.T).astype(rows.dtype)
    return out


def rms_of(sums, metric: str) -> float:
    sums = _sums(sums)
    return math.sqrt(max(float(sums[2] if metric == "plane" else sums[1]) / float(sums[0]), 0.0))


def icp(step, centre, rows: int, iters: int = 30, tol: float = 1e-6, metric: str = "plane", min_overlap: float = 0.3, scan="?", uid: str = "?", pose=IDENTITY):
    """The loop.  step: a callable, pose (R, t) float64 -> the 32 sums of that pose (`icp_step` on the device, the numpy restatement in the
    host tests); centre: the c of the sums; rows: the source's rows.  Per iteration: the sums of the current pose; fewer than 6 used
    pairs (3 for the point metric) is a ValueError that names scan and uid; RMS = sqrt(sum r^2 / pairs) (point: sqrt(sum d / pairs)); the
    loop ends when |RMS - previous| <= tol * previous, or after `iters` solves; otherwise the pose is composed with the solve.  The sums
    of the last pose decide the share of paired rows, (used + skipped) / rows; below min_overlap it is a ValueError: a silently wrong
    merge is worse than a refusal.  -> dict(pose, iterations, share, rms_first, rms_last)."""
    solve = solve_plane if metric == "plane" else solve_point
    prev = first = None
    done = 0

    def evaluate(p):
        sums = _sums(step(p))
        if sums[0] < MIN_PAIRS[metric]:
            raise ValueError(f"{uid}: registration of scan {scan} found {int(sums[0])} usable pairs, fewer than the {MIN_PAIRS[metric]} the {metric} metric needs: "
                             "do the scans start within --register_dist of each other?")
        return sums, rms_of(sums, metric)

    while True:
        sums, rms = evaluate(pose)
        first = rms if first is None else first
        if (prev is not None and abs(rms - prev) <= tol * prev) or done == iters:
            break
        pose = compose(pose, solve(sums, centre))
        prev = rms
        done += 1
    share = float(sums[0] + sums[30]) / rows
    if share < min_overlap:
        raise ValueError(f"{uid}: registration of scan {scan} paired {share:.3f} of its rows, below the minimum overlap {min_overlap:g}: "
                         "do the scans start within --register_dist of each other?")
    return {"pose": pose, "iterations": done, "share": share, "rms_first": first, "rms_last": rms}


def check_register_args(dist, iters, tol, metric, min_overlap) -> tuple:
    """The checks on the options; returns them as (float, int, float, str, float)."""
    dist = check_radius(dist)
    iters = check_int("iters", iters, 1, MAX_ITERS)
    if not is_real(tol) or not 0.0 <= float(tol) < 1.0:
        raise ValueError(f"tol must be in [0, 1), got {tol!r}")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if not is_real(min_overlap) or not 0.0 < float(min_overlap) <= 1.0:
        raise ValueError(f"min_overlap must be in (0, 1], got {min_overlap!r}")
    return dist, iters, float(tol), metric, float(min_overlap)


def scan_normals(cloud: torch.Tensor, k: int) -> torch.Tensor:
    """cloud (N, 3) float32 on the GPU -> (N, 3) float32 unoriented unit normals from the k nearest neighbours of every row in that cloud
    alone (`pc_outliers.grid_knn` + `pc_normals.estimate_normals`, 2^20 rows at a time).  The sign does not matter to r = n . (p' - q)."""
    from .pc_normals import estimate_normals
    from .pc_outliers import grid_knn
    idx = grid_knn(cloud, k, want=("idx",))["idx"]
    return torch.cat([estimate_normals(cloud, idx[a:a + MAX_QUERIES].contiguous())[0] for a in range(0, cloud.shape[0], MAX_QUERIES)]).to(torch.float32)


def register_rows(scans, dist, iters: int = 30, tol: float = 1e-6, metric: str = "plane", min_overlap: float = 0.3, normal_k=None, uid: str = "?", device="cuda",
                  names=None, coarse=None):
    """scans: host arrays (N_j, >= 3) of one object, all with the same number of columns, each of >= 64 finite rows -> (the merged rows,
    [(R_j, t_j)] float64).  Scan 0 is the frame, (I, 0).  Scan j is registered by `icp` onto the UNION of scans 0 .. j - 1 as registered
    (float32), from the identity, then appended: xyz -> R x + t in float64, cast to the scans' dtype.  normal_k None: columns 3:6 are the
    scans' normals (pc_normal), they serve the plane metric and are turned by R in the merged rows.  normal_k = k (pc_xyz): the plane
    metric's normals are estimated per scan, once, on that scan alone (`scan_normals`) and turned with it; no column but xyz changes.
    The union may hold at most 2^22 rows.  Prints one line per scan.  Makes no draw from any RNG.
    coarse: None, or (radius, points, iters, dist) as `pc_coarse.check_coarse_args` takes them: scan j then starts ICP not from the identity
    but from `pc_coarse.coarse_pose` of the scan against the union, for scans in unknown poses.  That takes normals on both sides whatever
    the metric, so every scan's are estimated (or read) and none is skipped; it prints a second line per scan, and its triples come from a
    generator of its own, not from the numpy RNG."""
    dist, iters, tol, metric, min_overlap = check_register_args(dist, iters, tol, metric, min_overlap)
    if coarse is not None:
        from . import pc_coarse
        coarse = pc_coarse.check_coarse_args(*coarse)
    scans = [as_host_cloud(s) for s in scans]
    names = [str(j) for j in range(len(scans))] if names is None else list(names)
    if not scans or len(names) != len(scans):
        raise ValueError(f"{uid}: registration needs at least one scan and a name for each")
    for s, name in zip(scans, names):
        if s.shape[0] < MIN_ROWS:
            raise ValueError(f"{uid}: scan {name} has {s.shape[0]} rows, fewer than the {MIN_ROWS} registration takes")
        if s.shape[1] != scans[0].shape[1]:
            raise ValueError(f"{uid}: scan {name} has {s.shape[1]} columns, scan {names[0]} has {scans[0].shape[1]}")
        check_finite(s)
    if normal_k is None and metric == "plane" and scans[0].shape[1] < 6:
        raise ValueError(f"{uid}: the plane metric needs normals in columns 3:6, or normal_k to estimate them")
    if normal_k is None and coarse is not None and scans[0].shape[1] < 6:
        raise ValueError(f"{uid}: coarse registration needs normals in columns 3:6, or normal_k to estimate them")
    total = sum(s.shape[0] for s in scans)
    if total > MAX_POINTS:
        raise ValueError(f"{uid}: the union of the scans has {total} rows, more than 2^22: thin the scans with --voxel_size")
    dev = cuda_device(device, "register_rows")
    plane = metric == "plane"
    normals = plane or coarse is not None                            # whether the device clouds carry normals in columns 3:6
    poses, merged = [IDENTITY], [scans[0].copy()]
    print(f"{uid}: registration (distance {dist:g}, {metric} metric): scan {names[0]} is the frame, {scans[0].shape[0]} rows")
    with torch.cuda.device(dev):
        def device_scan(s):
            xyz = torch.from_numpy(np.ascontiguousarray(s[:, :3], dtype=np.float32)).to(dev)
            if not normals:
                return xyz
            n = scan_normals(xyz, normal_k) if normal_k is not None else torch.from_numpy(np.ascontiguousarray(s[:, 3:6], dtype=np.float32)).to(dev)
            return torch.cat([xyz, n], 1)

        union = device_scan(scans[0])
        for j in range(1, len(scans)):
            s = scans[j]
            last = j == len(scans) - 1
            skip = last and normal_k is not None and coarse is None     # the last scan's estimated normals would serve nothing
            source = device_scan(s) if normals and not skip else torch.from_numpy(np.ascontiguousarray(s[:, :3], dtype=np.float32)).to(dev)
            centre = s[:, :3].astype(np.float64).mean(0).astype(np.float32)
            start = IDENTITY
            if coarse is not None:
                tgt, src = union.cpu().numpy(), source.cpu().numpy()
                found = pc_coarse.coarse_pose(tgt[:, :3], tgt[:, 3:6], src[:, :3], src[:, 3:6], *coarse, ops=pc_coarse.DeviceOps(dev), scan=names[j], uid=uid)
                start = found["pose"]
                print(f"{uid}: scan {names[j]}: coarse pose from {found['mutual']} matches, {found['triples']} triples, {found['count']} agreeing, "
                      f"turned {found['angle']:.4g} degrees")
            built = build(union, source, dist)
            res = icp(lambda p: icp_step(built, pose12(p), centre, dist, "target" if plane else None)["sums"].cpu().numpy(), centre.astype(np.float64), s.shape[0],
                      iters, tol, metric, min_overlap, names[j], uid, pose=start)
            R, t = res["pose"]
            poses.append((R, t))
            merged.append(apply_pose(s, (R, t), normals=normal_k is None))
            angle = math.degrees(math.acos(min(max((np.trace(R) - 1.0) / 2.0, -1.0), 1.0)))
            print(f"{uid}: scan {names[j]}: {res['iterations']} iterations, {res['share']:.3f} of {s.shape[0]} rows paired, RMS {res['rms_first']:.6g} -> "
                  f"{res['rms_last']:.6g}, turned {angle:.4g} degrees, moved {float(np.linalg.norm(t)):.6g}")
            if not last:                                             # the union grows by the scan as registered: float64 on the host, then cast
                moved = (s[:, :3].astype(np.float64) @ R.T + t).astype(np.float32)
                if normals:
                    moved = np.concatenate([moved, (source[:, 3:6].cpu().numpy().astype(np.float64) @ R.T).astype(np.float32)], 1)
                union = torch.cat([union, torch.from_numpy(moved).to(dev)])
    return np.concatenate(merged), poses
