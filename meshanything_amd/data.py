"""Input side of the hot path: the reference's `Dataset` (main.py:15-58) for point-cloud and mesh-file inputs, and one input type the
reference does not have: `pc_xyz`, a raw point cloud whose normals are estimated on the GPU (pc_normals.py)."""
from __future__ import annotations

import os
from typing import Dict, List

import numpy as np

from .cloud_prep import CloudPrep


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


def to_file_frame(verts: np.ndarray, frame, pose=None) -> np.ndarray:
    """Mesh vertices in the decoder's +-0.5 box -> the input file's coordinates, in float64: the inverse of the normalisation, centre +
    scale * 2 * v with frame = `pc_frame`'s (centre, scale) (times 2: the decoder's +-0.5 is the unit box), and then, with pose = (R', c) of
    `pc_align.align_rows`, the inverse of the alignment, c + R'T (x - c)."""
    from .mesh_score import DEFAULT_MESH_SCALE
    centre, scale = frame
    verts = centre[None, :] + scale * DEFAULT_MESH_SCALE * verts.astype(np.float64)
    if pose is not None:
        R, c = pose
        verts = c[None, :] + (verts - c[None, :]) @ R                # rows times R = R'T times columns
    return verts


SCAN_EXTENSIONS = {"pc_normal": (".npy", ".ply"), "pc_xyz": (".npy", ".xyz", ".txt", ".ply")}   # the point files of a directory of scans (register_dist)


def uid_of(input_path: str) -> str:
    """main.py:27,39: the sample's name, the file name up to its first dot."""
    return input_path.split("/")[-1].split(".")[0]


class Dataset:
    """`Dataset('pc_normal' | 'mesh', paths)` of main.py:15-58.  Sampling uses the GLOBAL numpy RNG like the reference
    (seed it first: main.py:129-133 calls accelerate.set_seed(args.seed) -> np.random.seed).  sample_device (e.g. "cuda"): sample
    mesh inputs on that GPU (mesh_input.mesh_to_pc_normal(..., device=...)): the same draws, the same clouds.

    `Dataset('pc_xyz', paths, normal_k=16)` has no reference counterpart: points without normals, from .npy files of shape (N, >= 3)
    (only the first three columns are read, so the normals of an (N, 6) file are ignored), .xyz / .txt files (np.loadtxt) or .ply files
    (the vertex element's x y z; with 'pc_normal' a .ply's x y z nx ny nz are read too: mesh_input.load_ply_points), N >= n_points.
    The same n_points rows as the pc_normal branch would draw are kept and their normals estimated from normal_k
    neighbours on the GPU (pc_normals.xyz_to_pc_normal).  It is not called 'pc': that is the reference's command-line default, a type
    its Dataset does not know and which therefore yields an empty dataset; that behaviour is restated here and pinned by the tests,
    so the new type needs a name of its own.

    Every other keyword is a field of `cloud_prep.CloudPrep`, which states what it does: point_sampling, and the six optional steps
    a pc_normal or pc_xyz file's rows go through, in the order of `cloud_prep.STAGES`, before the n_points rows are picked.  voxel_size
    (voxel thinning, pc_voxel.py) is the first of them: it is the only step that takes more than 2^22 rows, and with it a pc_xyz file may
    hold up to 2^28; the outlier filter after it then sees an even density, in which the strays, kept one per voxel, have a larger share.
    After the six, on what they left and before the pick, align_iters (alignment to the tightest box, pc_align.py) turns every kept part into
    the frame in which its bounding box is smallest: `normalize_pc` and the decoder's lattice work along the axes, and a scan that sits askew
    in its file wastes them.  Such an item carries "pose": (R', c), the turn and its fixed point.
    Before all of them, register_dist (registration, pc_register.py) lets an entry of input_list be a DIRECTORY: one object, whose point files
    (the type's extensions, in sorted order) are its partial scans and whose name is the uid.  Each scan is thinned on its own if voxel_size is
    on, the scans are registered onto the first and merged, and the union then goes the way of a file's rows.  Such an item carries
    "scan_poses": [(R, t)] float64, scan j's rows in the frame of scan 0 being R x + t.  A plain file passes through as without it.
    coarse_radius (with register_dist; pc_coarse.py) is for scans in UNKNOWN poses: every scan's ICP starts from a pose found by matching
    feature histograms over that radius at coarse_points keypoints and scoring coarse_iters triples of matches within coarse_dist."""

    def __init__(self, input_type: str, input_list: List[str], mc: bool = False, n_points: int = 4096, sample_device=None, normal_k: int = 16,
                 point_sampling: str = "random", outlier_k: int = 0, outlier_std: float = 2.0, cluster_radius: float = 0.0,
                 cluster_mode: str = "largest", cluster_min_points: int = 4096, plane_threshold: float = 0.0, plane_iters: int = 1024,
                 plane_count: int = 1, plane_min_fraction: float = 0.2, smooth_radius: float = 0.0, smooth_iters: int = 1,
                 upsample_radius: float = 0.0, upsample_points=None, voxel_size: float = 0.0, align_iters: int = 0, align_rounds: int = 4,
                 align_min_gain: float = 0.02, register_dist: float = 0.0, register_iters: int = 30, register_tol: float = 1e-6,
                 register_metric: str = "plane", register_min_overlap: float = 0.3, coarse_radius: float = 0.0, coarse_points: int = 1024,
                 coarse_iters: int = 4096, coarse_dist=None):
        self.data: List[Dict] = []
        prep = CloudPrep(normal_k=normal_k, point_sampling=point_sampling, outlier_k=outlier_k, outlier_std=outlier_std, plane_threshold=plane_threshold,
                         plane_iters=plane_iters, plane_count=plane_count, plane_min_fraction=plane_min_fraction, cluster_radius=cluster_radius,
                         cluster_mode=cluster_mode, cluster_min_points=cluster_min_points, smooth_radius=smooth_radius, smooth_iters=smooth_iters,
                         upsample_radius=upsample_radius, upsample_points=upsample_points, voxel_size=voxel_size, align_iters=align_iters,
                         align_rounds=align_rounds, align_min_gain=align_min_gain, register_dist=register_dist, register_iters=register_iters,
                         register_tol=register_tol, register_metric=register_metric, register_min_overlap=register_min_overlap,
                         coarse_radius=coarse_radius, coarse_points=coarse_points, coarse_iters=coarse_iters, coarse_dist=coarse_dist)
        floor = prep.check(input_type, n_points)                     # the fewest rows a file may have; every refusal that needs no file
        device = sample_device or "cuda"

        def pick_pc_normal(cur_data):
            if point_sampling == "fps":
                from . import pc_fps
                idx = pc_fps.fps_rows(cur_data, n_points, device=device)   # shape, length, finite: checked before the GPU is touched
            else:
                assert cur_data.shape[0] >= n_points, "input pc_normal should have at least 4096 points"
                idx = np.random.choice(cur_data.shape[0], n_points, replace=False)
            return cur_data[idx]

        def load_pc_normal(input_path):
            if input_path.lower().endswith(".ply"):                  # a scan as it comes: x y z nx ny nz of the vertex element
                from .mesh_input import load_ply_points
                return load_ply_points(input_path, normals=True)
            return np.load(input_path)

        def load_pc_xyz(input_path, floor=floor):
            from . import pc_normals
            if input_path.lower().endswith(".ply"):
                from .mesh_input import load_ply_points
                cur_data = load_ply_points(input_path)
            else:
                cur_data = np.load(input_path) if input_path.lower().endswith(".npy") else np.loadtxt(input_path, ndmin=2)
            if voxel_size:                                           # thinning takes what no other step does: up to 2^28 rows
                from . import pc_voxel
                return pc_normals.check_xyz(cur_data, floor, normal_k, max_points=pc_voxel.MAX_POINTS)
            return pc_normals.check_xyz(cur_data, floor, normal_k)   # shape, length, finite: before anything touches the GPU

        def pick_pc_xyz(cur_data):
            from . import pc_normals
            return pc_normals.xyz_to_pc_normal(cur_data, n_points, normal_k, device=device, sampling=point_sampling)
        def load_scans(input_path):
            """A directory of partial scans -> (the merged rows, the uid, the scans' poses): cloud_prep.SCANS"""
            (stage, module), = prep.scans()
            uid = os.path.basename(os.path.normpath(input_path))
            names = sorted(x for x in os.listdir(input_path) if x.lower().endswith(SCAN_EXTENSIONS[input_type]) and os.path.isfile(os.path.join(input_path, x)))
            if not names:
                raise ValueError(f"{uid}: the directory holds no {input_type} scan ({', '.join(SCAN_EXTENSIONS[input_type])})")
            xyz = input_type == "pc_xyz"
            scans = [load_pc_xyz(os.path.join(input_path, x), module.MIN_ROWS) if xyz else load_pc_normal(os.path.join(input_path, x)) for x in names]
            if voxel_size:                                           # each scan on its own; the union is thinned again by the stage, where they overlap
                from . import pc_voxel
                scans = [pc_voxel.thin_rows(rows, voxel_size, module.MIN_ROWS, f"{uid}/{uid_of(x)}", device=device) for rows, x in zip(scans, names)]
            merged, poses = stage.apply(module, prep, scans, [uid_of(x) for x in names], uid, normal_k if xyz else None, device)
            if xyz:
                from . import pc_normals
                merged = pc_normals.check_xyz(merged, floor, normal_k)
            return merged, uid, poses
        clouds = {"pc_normal": (load_pc_normal, pick_pc_normal), "pc_xyz": (load_pc_xyz, pick_pc_xyz)}   # how a file is loaded, how its n_points rows are picked
        if input_type in clouds:
            load, pick = clouds[input_type]
            for input_path in input_list:
                if register_dist and os.path.isdir(input_path):
                    rows, uid, poses = load_scans(input_path)
                    for cur_data, keys in prep.parts(rows, uid, device, n_points):
                        self.data.append({"pc_normal": pick(cur_data), **keys, "scan_poses": poses})
                    continue
                for cur_data, keys in prep.parts(load(input_path), uid_of(input_path), device, n_points):
                    self.data.append({"pc_normal": pick(cur_data), **keys})
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
        if "pose" in d:
            item["pose"] = d["pose"]
        if "scan_poses" in d:
            item["scan_poses"] = d["scan_poses"]
        return item
