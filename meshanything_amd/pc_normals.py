"""Raw point clouds as input (`--input_type pc_xyz`): estimate the normals the encoder needs from xyz alone.

Three stages.  `knn` and `estimate_normals` are one call each into the HIP library (csrc/pc_normals.hpp; C ABI
ma_op_pc_knn / ma_op_pc_normals): the k nearest neighbours under the total order (squared distance, index), and per point the
eigenvector of the smallest eigenvalue of its neighbourhood's covariance, in float64.  They need CUDA tensors; there is no CPU
fallback.  `orient_normals` is Hoppe's sign propagation over the neighbour graph, a sequential walk over a few thousand points: host
numpy with a heap.  `xyz_to_pc_normal` does the whole input side and returns the (n_points, 6) cloud `data.normalize_pc` accepts.
There is no reference counterpart: the reference takes only clouds that already carry unit normals, or meshes.
"""
from __future__ import annotations

import ctypes as C
import heapq

import numpy as np
import torch

from . import _lib
from .pc_common import MAX_POINTS, MAX_QUERIES, as_host_cloud, check_device_cloud, check_finite, cuda_device, need_cuda, upload_xyz

MIN_K, MAX_K, MAX_SPLITS = 3, 32, 64                             # MA_PC_KNN_MIN_K, _MAX_K, _MAX_SPLITS


def check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or not MIN_K <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in {MIN_K}..{MAX_K}, got {k!r}")
    return int(k)


def knn(points: torch.Tensor, query_idx=None, k: int = 16, splits: int = 0):
    """points (N, 3 | 6) float32 on the GPU, xyz in the first three columns; query_idx (Q) integer rows of points, None = every row ->
    (nbr_idx (Q, k) int32, nbr_d2 (Q, k) float32), nearest first, ordered by (squared distance, index) (ma_op_pc_knn).  splits: the
    number of chunks the reference range is searched in, 0 = the library's choice; the result does not depend on it."""
    k = check_k(k)
    check_device_cloud(points, k, "k")
    if isinstance(splits, bool) or int(splits) != splits or not 0 <= int(splits) <= MAX_SPLITS:
        raise ValueError(f"splits must be an integer in 0..{MAX_SPLITS}, got {splits!r}")
    N = points.shape[0]
    if query_idx is not None:
        query_idx = torch.as_tensor(query_idx)
        if query_idx.dim() != 1 or query_idx.dtype not in (torch.int32, torch.int64) or not 1 <= query_idx.shape[0] <= MAX_QUERIES:
            raise ValueError(f"query_idx must be a (Q) int32 or int64 tensor with 1 <= Q <= 2^20, got {tuple(query_idx.shape)} {query_idx.dtype}")
    elif N > MAX_QUERIES:
        raise ValueError(f"without query_idx every point is a query: N = {N} exceeds 2^20 queries")
    need_cuda(points, "knn")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        qi = None
        if query_idx is not None:
            qi = query_idx.to(dev)
            if int(qi.min()) < 0 or int(qi.max()) >= N:
                raise ValueError(f"query_idx must lie in [0, {N})")
            qi = qi.to(torch.int32).contiguous()
        Q = N if qi is None else qi.shape[0]
        nbytes = lib.ma_pc_knn_workspace_bytes(N, Q, k, int(splits))
        if nbytes == 0:
            raise ValueError(f"outside the limits of ma_op_pc_knn: N = {N}, Q = {Q}, k = {k}, splits = {splits}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nbr_idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
        nbr_d2 = torch.empty((Q, k), dtype=torch.float32, device=dev)
        _lib.check(lib.ma_op_pc_knn(ref.data_ptr(), N, ref.shape[1], None if qi is None else qi.data_ptr(), Q, k, int(splits), nbr_idx.data_ptr(),
                                    nbr_d2.data_ptr(), ws.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return nbr_idx, nbr_d2


def estimate_normals(points: torch.Tensor, nbr_idx: torch.Tensor):
    """points (N, 3 | 6) float32 on the GPU, nbr_idx (Q, k) int32 rows of points (knn's output) -> (normals (Q, 3), eigvals (Q, 3))
    float64: the covariance of each neighbourhood, its eigenvalues ascending and the unit eigenvector of the smallest, its component
    of largest magnitude positive (ma_op_pc_normals).  Unoriented: `orient_normals` decides the signs."""
    if not torch.is_tensor(nbr_idx) or nbr_idx.dim() != 2 or nbr_idx.dtype != torch.int32 or not 1 <= nbr_idx.shape[0] <= MAX_QUERIES:
        raise ValueError("nbr_idx must be a (Q, k) int32 tensor with 1 <= Q <= 2^20")
    k = check_k(nbr_idx.shape[1])
    check_device_cloud(points, k, "k")
    need_cuda(points, "estimate_normals")
    lib = _lib.load()
    dev = points.device
    with torch.cuda.device(dev):
        ref = points.contiguous()
        nb = nbr_idx.to(dev).contiguous()
        Q = nb.shape[0]
        normals = torch.empty((Q, 3), dtype=torch.float64, device=dev)
        eigvals = torch.empty((Q, 3), dtype=torch.float64, device=dev)
        _lib.check(lib.ma_op_pc_normals(ref.data_ptr(), ref.shape[0], ref.shape[1], nb.data_ptr(), Q, k, normals.data_ptr(), eigvals.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return normals, eigvals


def orient_normals(points, normals, nbr_idx) -> np.ndarray:
    """Hoppe's propagation of a consistent sign over the neighbour graph, made deterministic.  points (n, >= 3), normals (n, 3) unit and
    unoriented, nbr_idx (n, k) rows of points -> the normals (n, 3) float64, each kept or negated.

    Start at the not-yet-visited point of greatest z (the lowest index on ties) and make its normal point up (flip when n_z < 0); grow
    a tree with a heap keyed by (1 - |n_i . n_j|, i, j) over the directed edges i -> j, j in nbr_idx[i]; when j is reached from i with
    n_i . n_j < 0, flip n_j; repeat for every component."""
    pts = np.asarray(points)
    n = np.array(normals, dtype=np.float64)
    nbr = np.asarray(nbr_idx)
    if n.ndim != 2 or n.shape[1] != 3 or pts.ndim != 2 or pts.shape[1] < 3 or pts.shape[0] != n.shape[0] or nbr.ndim != 2 or nbr.shape[0] != n.shape[0]:
        raise ValueError(f"need points (n, >= 3), normals (n, 3) and nbr_idx (n, k), got {pts.shape}, {n.shape}, {nbr.shape}")
    if nbr.size and (nbr.min() < 0 or nbr.max() >= n.shape[0]):
        raise ValueError(f"nbr_idx must lie in [0, {n.shape[0]})")
    count = n.shape[0]
    weight = (1.0 - np.abs(np.einsum("ic,ikc->ik", n, n[nbr]))).tolist()     # the key's first part does not change under a flip
    nbrs = nbr.tolist()
    z_order = np.lexsort((np.arange(count), -pts[:, 2].astype(np.float64))).tolist()   # greatest z first, the lowest index among equals
    visited = [False] * count
    flip = [False] * count
    nl = n.tolist()
    heap: list = []

    def reach(i):
        visited[i] = True
        wi, ni = weight[i], nbrs[i]
        for e in range(len(ni)):
            j = ni[e]
            if not visited[j]:
                heapq.heappush(heap, (wi[e], i, j))

    for seed in z_order:
        if visited[seed]:
            continue
        flip[seed] = nl[seed][2] < 0
        reach(seed)
        while heap:
            _, i, j = heapq.heappop(heap)
            if visited[j]:
                continue
            a, b = nl[i], nl[j]
            dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]              # of the normals as given; n_i may have been flipped since
            flip[j] = (-dot if flip[i] else dot) < 0
            reach(j)
    n[np.asarray(flip)] *= -1.0
    return n


def check_xyz(xyz, n_points: int, k: int, max_points=None) -> np.ndarray:
    """The checks of xyz_to_pc_normal that need no device; returns xyz as an array.  max_points: the row cap of a file that voxel thinning
    (pc_voxel.py) reduces before anything else sees it, instead of 2^22."""
    xyz = as_host_cloud(xyz)
    k = check_k(k)
    if n_points < k:
        raise ValueError(f"n_points = {n_points} is less than k = {k}")
    if xyz.shape[0] < n_points:
        raise ValueError(f"a pc_xyz input should have at least {n_points} points, got {xyz.shape[0]}")
    if max_points is not None and xyz.shape[0] > max_points:
        raise ValueError(f"a pc_xyz input may have at most {max_points} points with voxel thinning, got {xyz.shape[0]}")
    if max_points is None and xyz.shape[0] > MAX_POINTS:
        raise ValueError(f"a pc_xyz input may have at most 2^22 points, got {xyz.shape[0]}")
    if n_points > MAX_QUERIES:
        raise ValueError(f"n_points may be at most 2^20, got {n_points}")
    check_finite(xyz)
    return xyz


def xyz_to_pc_normal(xyz, n_points: int = 4096, k: int = 16, device="cuda", sampling: str = "random") -> np.ndarray:
    """xyz (N, >= 3), N >= n_points, only the first three columns are read -> (n_points, 6) in xyz's dtype: n_points rows of xyz and
    their estimated, consistently oriented unit normals.

    The rows are `np.random.choice(N, n_points, replace=False)` from the GLOBAL numpy RNG, the draw Dataset's pc_normal branch makes.
    With sampling = "fps" they are the rows farthest-point sampling keeps (pc_fps.farthest_point_sample over the uploaded float32
    cloud, automatic start), in pick order, and the global RNG is not touched.
    Each chosen point's normal comes from its k nearest neighbours in the WHOLE cloud (the dense cloud gives the better plane); the
    signs are then propagated over the k-neighbour graph of the chosen points alone (`orient_normals`)."""
    xyz = check_xyz(xyz, n_points, k)
    if sampling not in ("random", "fps"):
        raise ValueError(f'sampling must be "random" or "fps", got {sampling!r}')
    dev = cuda_device(device, "xyz_to_pc_normal")
    if sampling == "fps":
        from .pc_fps import check_fps_args, farthest_point_sample
        check_fps_args(xyz.shape[0], n_points, None, 0)
    else:
        idx = np.random.choice(xyz.shape[0], n_points, replace=False)
    with torch.cuda.device(dev):
        cloud = upload_xyz(xyz, dev)
        if sampling == "fps":
            rows = farthest_point_sample(cloud, n_points)[0]
            idx = rows.cpu().numpy().astype(np.int64)
        else:
            rows = torch.from_numpy(idx.astype(np.int32)).to(dev)
        nbr, _ = knn(cloud, rows, k)
        normals, _ = estimate_normals(cloud, nbr)
        chosen = cloud[rows.long()].contiguous()
        graph, _ = knn(chosen, None, k)
        normals, graph = normals.cpu().numpy(), graph.cpu().numpy()
    picked = xyz[idx, :3]
    oriented = orient_normals(picked, normals, graph)
    return np.concatenate([picked, oriented.astype(xyz.dtype)], axis=-1)
