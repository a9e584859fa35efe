"""Input side of the hot path: the reference's `Dataset` (main.py:15-58) for point-cloud and mesh-file inputs, and one input type the
reference does not have: `pc_xyz`, a raw point cloud whose normals are estimated on the GPU (pc_normals.py)."""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np


def normalize_pc(pc_normal: np.ndarray) -> np.ndarray:
    """Dataset.__getitem__ (main.py:45-58): centre xyz on the bounding-box mid-point, scale so that max |coord| = 0.9995,
    keep the normals, return float16.  All arithmetic stays in the input's dtype (an fp16 .npy is normalised in fp16),
    exactly as numpy does it in the reference."""
    pc_coor = pc_normal[:, :3]
    normals = pc_normal[:, 3:]
    bounds = np.array([pc_coor.min(axis=0), pc_coor.max(axis=0)])
    pc_coor = pc_coor - (bounds[0] + bounds[1])[None, :] / 2
    pc_coor = pc_coor / np.abs(pc_coor).max() * 0.9995
    assert (np.linalg.norm(normals, axis=-1) > 0.99).all(), "normals should be unit vectors, something wrong"
    return np.concatenate([pc_coor, normals], axis=-1, dtype=np.float16)


def pc_frame(pc_normal: np.ndarray):
    """(centre (3) float64, scale float64): the inverse of `normalize_pc`'s affine map on the same rows, x ~ centre + scale * normalised.
    Computed in float64: centre = the bounding-box mid-point, scale = max |x - centre| / 0.9995."""
    pc_coor = np.asarray(pc_normal)[:, :3].astype(np.float64)
    centre = (pc_coor.min(axis=0) + pc_coor.max(axis=0)) / 2
    return centre, float(np.abs(pc_coor - centre[None, :]).max() / 0.9995)


def uid_of(input_path: str) -> str:
    """main.py:27,39: the sample's name, the file name up to its first dot."""
    return input_path.split("/")[-1].split(".")[0]


class Dataset:
    """`Dataset('pc_normal' | 'mesh', paths)` of main.py:15-58.  Sampling uses the GLOBAL numpy RNG like the reference
    (seed it first: main.py:129-133 calls accelerate.set_seed(args.seed) -> np.random.seed).  sample_device (e.g. "cuda"): sample
    mesh inputs on that GPU (mesh_input.mesh_to_pc_normal(..., device=...)): the same draws, the same clouds.

    `Dataset('pc_xyz', paths, normal_k=16)` has no reference counterpart: points without normals, from .npy files of shape (N, >= 3)
    (only the first three columns are read, so the normals of an (N, 6) file are ignored) or .xyz / .txt files (np.loadtxt), N >=
    n_points.  The same n_points rows as the pc_normal branch would draw are kept and their normals estimated from normal_k
    neighbours on the GPU (pc_normals.xyz_to_pc_normal).  It is not called 'pc': that is the reference's command-line default, a type
    its Dataset does not know and which therefore yields an empty dataset; that behaviour is restated here and pinned by the tests,
    so the new type needs a name of its own.

    point_sampling="fps" (pc_normal and pc_xyz; the reference has nothing like it): the n_points rows are the ones farthest-point
    sampling keeps (pc_fps.farthest_point_sample on the GPU over the first three columns as float32, N <= 2^22, finite), in pick
    order, instead of a uniform draw: a scan's density follows the scanner, and a uniform draw leaves its thin parts a handful of
    points.  Such an input consumes no draws from the numpy RNG.  With "mesh" it is a ValueError.

    outlier_k=K > 0 (pc_normal and pc_xyz; the reference has nothing like it): statistical outlier removal before anything else
    happens (pc_outliers.remove_statistical_outliers on the GPU, K neighbours, N <= 2^22, finite): the rows whose mean distance to
    their K nearest neighbours exceeds the cloud's mean by more than outlier_std standard deviations are dropped, the survivors keep
    their order and stand in for the file's rows: the uniform draw or FPS runs over them, and pc_xyz takes its normals from their
    neighbours.  One stray row would otherwise set the scale of `normalize_pc`, and FPS picks strays first.  Fewer than n_points
    survivors is a ValueError.  0 = off: no code path and no RNG draw changes.  With "mesh" a non-zero value is a ValueError.

    cluster_radius=R > 0 (pc_normal and pc_xyz; the reference has nothing like it): Euclidean clustering over the outlier filter's
    survivors (pc_cluster.split_rows on the GPU, N <= 2^22, finite): the rows fall into the connected components of the graph that
    links two rows at most R apart, and the components of fewer than cluster_min_points rows (>= n_points) are dropped: a floating
    clump the outlier filter cannot see, or a second object.  Every kept component then stands in for the file's rows: the uniform
    draw or FPS runs over it, and pc_xyz takes its normals from its rows alone.  cluster_mode "largest": the largest component only,
    one item, uid unchanged.  "split": one item per kept component, adjacent, largest first, with uid "{uid}_part{j}" and the extra
    keys "group" (the file's uid) and "part" (j); `__getitem__` adds "frame" = pc_frame of the item's rows, with which main.py maps
    the part's mesh back into the file's coordinates.  No component of cluster_min_points rows is a ValueError.  0 = off: no code
    path and no RNG draw changes, and the items keep exactly the keys above.  With "mesh" a non-zero value is a ValueError.

    plane_threshold=T > 0 (pc_normal and pc_xyz; the reference has nothing like it): dominant-plane removal AFTER the outlier filter and
    BEFORE clustering (pc_plane.remove_planes on the GPU, N <= 2^22, finite): up to plane_count times, plane_iters RANSAC hypotheses from
    a private generator are scored against the rows still kept, the one that holds the most rows within T (file units) is refitted to
    them and its inliers are dropped; a best plane that holds fewer than plane_min_fraction of the rows ends the search.  That is the
    table, floor or wall a scanned object stands on: as dense as the object, so the outlier filter keeps it, and in touch with it, so
    clustering cannot part them.  The survivors keep their order and stand in for the file's rows.  An object's own large flat face is
    a plane too: the floor plane_min_fraction and the opt-in are the only guard.  Fewer than n_points survivors is a ValueError.
    0 = off: no code path and no draw from the numpy RNG changes (the hypotheses never use the global RNG).  With "mesh" a non-zero
    value is a ValueError.

    smooth_radius=R > 0 (pc_normal and pc_xyz; the reference has nothing like it): moving-least-squares smoothing, the LAST of the cleaning
    steps and before sampling (pc_smooth.smooth_rows on the GPU, N <= 2^22, finite), once per kept part: every row that stands in for the
    file is projected onto the plane fitted to the rows within R of it (file units), smooth_iters times (1..8), and a file's normals are
    replaced by the fitted ones on the file's side.  The strays and the table are gone by then and cannot pull the fit.  The uniform draw
    or FPS then runs over the smoothed rows, and pc_xyz estimates its normals from them.  A plane fit shrinks a curved surface by roughly
    R^2 / (8 * its radius of curvature) and rounds edges over a width of R.  0 = off: no code path, key, print or RNG draw changes.
    With "mesh" a non-zero value is a ValueError.

    upsample_radius=R > 0 (pc_normal and pc_xyz; the reference has nothing like it): upsampling of a SPARSE cloud, after smoothing and once
    per kept part, before the uniform draw, FPS or the pc_xyz normal estimate (pc_upsample.upsample_rows on the GPU): a part of fewer than
    upsample_points rows (default 4 * n_points, n_points..2^22) gains lattice points at spacing R / m in the plane fitted to the rows within
    R of each row (file units), each kept where its own row is the nearest, m the first of 2, 4, ..., 64 that reaches upsample_points; a new
    row is a copy of its seed's row with xyz replaced, so a file's normals are the seed's, and pc_xyz estimates its normals from the
    upsampled rows.  With it, and only then, the floor on the rows of a file, of the outlier filter's and plane removal's survivors and of
    cluster_min_points is pc_upsample.MIN_ROWS = 64 instead of n_points; fewer than n_points rows after upsampling is a ValueError.  The
    patches are flat, an open border grows outward by up to R, at a sharp edge the patch sticks out; choose R at about one to two point
    spacings, and prefer point_sampling="fps": a uniform draw follows the uneven density that patches of different size leave.  0 = off: no
    code path, key, print, floor or RNG draw changes.  With "mesh" a non-zero value is a ValueError."""

    def __init__(self, input_type: str, input_list: List[str], mc: bool = False, n_points: int = 4096, sample_device=None, normal_k: int = 16,
                 point_sampling: str = "random", outlier_k: int = 0, outlier_std: float = 2.0, cluster_radius: float = 0.0,
                 cluster_mode: str = "largest", cluster_min_points: int = 4096, plane_threshold: float = 0.0, plane_iters: int = 1024,
                 plane_count: int = 1, plane_min_fraction: float = 0.2, smooth_radius: float = 0.0, smooth_iters: int = 1,
                 upsample_radius: float = 0.0, upsample_points=None):
        self.data: List[Dict] = []
        if point_sampling not in ("random", "fps"):
            raise ValueError(f'point_sampling must be "random" or "fps", got {point_sampling!r}')
        if point_sampling == "fps" and input_type == "mesh":
            raise ValueError('point_sampling="fps" applies to pc_normal and pc_xyz inputs: the points of a mesh input are already drawn from its surface')
        floor = n_points                                             # the fewest rows a file, and what a cleaning step leaves of it, may have
        if upsample_radius:
            from .pc_upsample import MIN_ROWS, check_upsample_args, upsample_rows
            if input_type == "mesh":
                raise ValueError("upsample_radius applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface")
            upsample_points = 4 * n_points if upsample_points is None else upsample_points
            check_upsample_args(upsample_radius, upsample_points, n_points)   # before any file is read
            floor = min(MIN_ROWS, n_points)
        elif upsample_points is not None:
            raise ValueError("upsample_points needs upsample_radius > 0")
        if outlier_k:
            from .pc_outliers import check_filter_args, filter_rows
            if input_type == "mesh":
                raise ValueError("outlier_k applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface")
            check_filter_args(outlier_k, outlier_std)                # before any file is read
        if plane_threshold:
            from .pc_plane import check_remove_args, remove_planes
            if input_type == "mesh":
                raise ValueError("plane_threshold applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface")
            check_remove_args(plane_threshold, plane_iters, plane_count, plane_min_fraction)   # before any file is read
        if cluster_radius:
            from .pc_cluster import check_split_args, split_rows
            if input_type == "mesh":
                raise ValueError("cluster_radius applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface")
            check_split_args(cluster_radius, cluster_min_points, cluster_mode)
            if cluster_min_points < floor:
                raise ValueError(f"cluster_min_points = {cluster_min_points} is less than the {floor} rows " +
                                 ("upsampling takes" if upsample_radius else "the encoder takes"))
        if smooth_radius:
            from .pc_smooth import check_smooth_args, smooth_rows
            if input_type == "mesh":
                raise ValueError("smooth_radius applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface")
            check_smooth_args(smooth_radius, smooth_iters)           # before any file is read

        def parts_of(cur_data, uid):
            """[(rows of the file that stand in for it, the item's extra keys)]: the file itself, or its kept components; smoothed, then upsampled"""
            if not upsample_radius:
                return smoothed_of(cur_data, uid)
            parts = []
            for rows, keys in smoothed_of(cur_data, uid):
                if rows.shape[0] < floor:
                    raise ValueError(f"{keys['uid']}: upsampling takes at least {floor} rows, got {rows.shape[0]}")
                rows = upsample_rows(rows, upsample_radius, upsample_points, keys["uid"], device=sample_device or "cuda")
                if rows.shape[0] < n_points:
                    raise ValueError(f"{keys['uid']}: upsampling left {rows.shape[0]} rows, fewer than the {n_points} the encoder takes")
                parts.append((rows, keys))
            return parts

        def smoothed_of(cur_data, uid):
            if smooth_radius:
                return [(smooth_rows(rows, smooth_radius, smooth_iters, keys["uid"], device=sample_device or "cuda"), keys) for rows, keys in split_of(cur_data, uid)]
            return split_of(cur_data, uid)

        def split_of(cur_data, uid):
            if not cluster_radius:
                return [(cur_data, {"uid": uid})]
            rows = split_rows(cur_data, cluster_radius, cluster_min_points, cluster_mode, uid, device=sample_device or "cuda")
            if cluster_mode == "largest":
                return [(cur_data[rows[0]], {"uid": uid})]
            return [(cur_data[r], {"uid": f"{uid}_part{j}", "group": uid, "part": j}) for j, r in enumerate(rows)]
        if input_type == "pc_normal":
            for input_path in input_list:
                cur_data = np.load(input_path)
                if outlier_k:
                    cur_data = filter_rows(cur_data, outlier_k, outlier_std, floor, uid_of(input_path), device=sample_device or "cuda")
                if plane_threshold:
                    cur_data = cur_data[remove_planes(cur_data, plane_threshold, plane_iters, plane_count, plane_min_fraction, floor, uid_of(input_path),
                                                      device=sample_device or "cuda")]
                for cur_data, keys in parts_of(cur_data, uid_of(input_path)):
                    if point_sampling == "fps":
                        from .pc_fps import fps_rows
                        idx = fps_rows(cur_data, n_points, device=sample_device or "cuda")   # shape, length, finite: checked before the GPU is touched
                    else:
                        assert cur_data.shape[0] >= n_points, "input pc_normal should have at least 4096 points"
                        idx = np.random.choice(cur_data.shape[0], n_points, replace=False)
                    self.data.append({"pc_normal": cur_data[idx], **keys})
        elif input_type == "mesh":
            # main.py:29-39 -> mesh_to_pc.py:42-57: load the file, draw n_points surface points + the normal of the face under each
            from .mesh_input import load_mesh, mesh_to_pc_normal
            if mc:
                raise NotImplementedError("--mc (mesh_to_pc.py:13-40: make the input watertight before sampling) runs on the GPU and this "
                                          "Dataset is host-only: run meshanything_amd.watertight.process_mesh_to_pc(meshes, "
                                          "marching_cubes=True) and build the dataset with Dataset.from_clouds(clouds, uids)")
            for input_path in input_list:
                vertices, faces = load_mesh(input_path)
                self.data.append({"pc_normal": mesh_to_pc_normal(vertices, faces, n_points, device=sample_device), "uid": uid_of(input_path)})
        elif input_type == "pc_xyz":
            from .pc_normals import check_xyz, xyz_to_pc_normal
            for input_path in input_list:
                cur_data = np.load(input_path) if input_path.lower().endswith(".npy") else np.loadtxt(input_path, ndmin=2)
                cur_data = check_xyz(cur_data, floor, normal_k)          # shape, length, finite: before anything touches the GPU
                if outlier_k:
                    cur_data = filter_rows(cur_data, outlier_k, outlier_std, floor, uid_of(input_path), device=sample_device or "cuda")
                if plane_threshold:
                    cur_data = cur_data[remove_planes(cur_data, plane_threshold, plane_iters, plane_count, plane_min_fraction, floor, uid_of(input_path),
                                                      device=sample_device or "cuda")]
                for cur_data, keys in parts_of(cur_data, uid_of(input_path)):
                    self.data.append({"pc_normal": xyz_to_pc_normal(cur_data, n_points, normal_k, device=sample_device or "cuda", sampling=point_sampling), **keys})
        # any other value yields an empty dataset, like the reference's default 'pc' (main.py:70-75)
        print(f"dataset total data samples: {len(self.data)}")

    @classmethod
    def from_clouds(cls, clouds: List[np.ndarray], uids: List[str]) -> "Dataset":
        """The dataset of already sampled (N, 6) clouds, e.g. the output of watertight.process_mesh_to_pc(..., marching_cubes=True)
        (main.py:29-39 with --mc); items are normalised on access exactly like the constructor's."""
        if len(clouds) != len(uids):
            raise ValueError(f"{len(clouds)} clouds but {len(uids)} uids")
        self = cls.__new__(cls)
        self.data = [{"pc_normal": c, "uid": u} for c, u in zip(clouds, uids)]
        print(f"dataset total data samples: {len(self.data)}")
        return self

    def __len__(self) -> int:
        return len(self.data)

    def groups(self) -> List[int]:
        """Per item the index of its group: the items of one file split into parts (cluster_mode "split") share one, adjacent; every
        other item is a group of its own.  What dp.shard_grouped shards over."""
        out: List[int] = []
        for i, d in enumerate(self.data):
            same = i > 0 and "group" in d and self.data[i - 1].get("group") == d["group"] and self.data[i - 1]["part"] + 1 == d["part"]
            out.append(out[-1] if same else (out[-1] + 1 if out else 0))
        return out

    def __getitem__(self, idx: int) -> Dict:
        d = self.data[idx]
        item = {"pc_normal": normalize_pc(d["pc_normal"]), "uid": d["uid"]}
        if "group" in d:
            item.update(group=d["group"], part=d["part"], frame=pc_frame(d["pc_normal"]))
        return item
