#!/usr/bin/env python3
"""Command line of the reference (`main.py:60-177`) on the MI355X engine.

    python main.py --input_path pc_examples/mouse.npy --input_type pc_normal --out_dir out --pretrained_weights ckpt.safetensors
    python -m torch.distributed.run --nproc-per-node 8 main.py --input_dir clouds/ --input_type pc_normal ...

Same flags as the reference.  Differences, all forced by the environment (no network, no trimesh): the checkpoint is
read from `--pretrained_weights` (the reference ignores that flag and downloads `MeshAnything_350m.pth`, main.py:95-98;
`--synthetic_weights` uses the seeded random checkpoint of the tests instead); `--input_type mesh` reads .obj / .ply / .off /
.stl and samples the surface in numpy (`meshanything_amd/mesh_input.py`; with the extra flag `--gpu_sampling` the same samples come from
HIP kernels, `meshanything_amd/surface_sample.py`), `--mc` makes the input watertight on the GPU first
(`meshanything_amd/watertight.py`: unsigned distance + marching cubes in HIP instead of mesh2sdf + scikit-image); the
mesh clean-up of main.py:156-175 is restated without trimesh in `meshanything_amd/mesh_export.py`.  One flag the reference does
not have: `--sampling --num_candidates N` draws N meshes per input in one batch and writes the one closest to the input cloud
(`meshanything_amd/mesh_score.py`); `--normal_weight W` adds W * (1 - normal consistency between the candidate's faces and the cloud's
normals) to that ranking, and `--orient cloud` winds every written face the way the nearest cloud normals face instead of by
`fix_normals`' signed volume (`--orient volume`, the default and the reference's behaviour).  And one input type it does not have: `--input_type pc_xyz` takes points WITHOUT normals (.npy of
shape (N, >= 3), .xyz, .txt or .ply) and estimates them on the GPU from `--normal_k` neighbours (`meshanything_amd/pc_normals.py`).
Both cloud types read `.ply` point files as scanners and photogrammetry write them (ascii, binary little or big endian): the vertex
element's `x y z` for pc_xyz, `x y z nx ny nz` for pc_normal, float or double; faces are ignored.
`--voxel_size L` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input file) thins a DENSE input before anything else:
of the points in one cube of edge L, counted from the cloud's minimum corner, the one nearest the cube's centre is kept, on the GPU through
a hash table over the cubes (`meshanything_amd/pc_voxel.py`).  It is the only step that takes more than 4194304 points, up to 268435456,
fed through the GPU in pieces; at most 4194304 cubes may be occupied, else choose a larger L.  The later steps then cost less and see an
even density; strays survive it one per cube, so their share rises: follow it with `--outlier_k`.  One line per input reports the rows kept.
`--point_sampling fps` (with pc_normal and pc_xyz) keeps the 4096 points farthest-point sampling picks on the GPU
(`meshanything_amd/pc_fps.py`) instead of the reference's uniform draw; such an input consumes no draws from the numpy RNG, so the RNG
state later stages see differs from a `--point_sampling random` run.
`--outlier_k K` (with pc_normal and pc_xyz; 0 = off, the default) removes statistical outliers first: the rows whose mean distance to
their K nearest neighbours exceeds the cloud's mean by more than `--outlier_std` standard deviations, found on the GPU over a cell grid
(`meshanything_amd/pc_outliers.py`); sampling and normal estimation then see the survivors only, and one line per input reports how many
rows went.
`--plane_threshold T` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input file) then removes the dominant plane,
the table, floor or wall a scanned object stands on: `--plane_iters` RANSAC hypotheses (default 1024, 1..65536), three rows each from a
private generator (the numpy RNG is not touched), are scored against every row on the GPU (`meshanything_amd/pc_plane.py`), the plane that
holds the most rows within T is refitted to them and its inliers are dropped, `--plane_count` times (default 1, 1..8).  A best plane that
holds fewer than `--plane_min_fraction` of the rows (default 0.2, in (0, 1]) ends the search: 1024 draws find a plane of 0.2 of the rows
with probability 1 - 2.7e-4, one of 0.1 only with 0.64, so raise `--plane_iters` when you lower the floor.  An object's own large flat
face is a plane too; the floor and the opt-in are the only guard.  One line per input reports the planes.
`--cluster_radius R` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input file) then splits what is left into the
connected parts of the graph that links two points at most R apart, on the GPU over the same cell grid (`meshanything_amd/pc_cluster.py`),
and drops the parts of fewer than `--cluster_min_points` points (default and least 4096): a floating clump the outlier filter cannot see,
or a second object; one line per input reports the parts.  `--cluster_mode largest` (the default) meshes the largest part as the input;
`--cluster_mode split` meshes every kept part as a row of the batch, writes `{uid}_part{j}_gen.obj` in the INPUT's coordinates (centre +
scale * 2 * v, the inverse of the normalisation) and, after a file's last part, `{uid}_gen.obj`: the parts one after the other, no vertex
merged across them.  The parts of one file stay on one rank (`dp.shard_grouped`).
`--smooth_radius R` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input file) smooths what is left, last of the
cleaning steps and once per kept part: every point is projected onto the plane fitted to the points within R of it, weights
(1 - d^2 / R^2)^3, on the GPU over the same cell grid (`meshanything_amd/pc_smooth.py`), `--smooth_iters` times (1..8, default 1), and a
pc_normal file's normals are replaced by the fitted ones on the file's side; sampling and the pc_xyz normal estimate then see the smoothed
points, and one line per input reports how far they moved.  It removes measurement noise on the surface itself, which no other step touches.
A plane fit shrinks a curved surface by roughly R^2 / (8 * its radius of curvature) and rounds edges over a width of R.
`--upsample_radius R` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input file) then upsamples a SPARSE input, once
per kept part and before sampling: an input of fewer than `--upsample_points` points (default 16384, 4096..4194304) gains lattice points
at spacing R / m in the plane fitted to the points within R of each point, each kept where its own point is the nearest, on the GPU over
the same cell grid (`meshanything_amd/pc_upsample.py`); m is the first of 2, 4, ..., 64 that reaches `--upsample_points`.  A new row copies
its seed's row, so a pc_normal file's normals are the seed's; the pc_xyz normal estimate sees the upsampled points; one line per input
reports m and the rows before and after.  With it an input file, the survivors of the cleaning steps and `--cluster_min_points` may go down
to 64 points instead of 4096.  The patches are flat, an open border grows outward by up to R, and at a sharp edge the fitted plane is
diagonal and the patch sticks out: choose R at about one to two point spacings, and use `--point_sampling fps`, since a uniform draw
follows the uneven density that patches of different size leave.
`--align_iters H` (with pc_normal and pc_xyz; 0 = off, the default; 256..65536) then aligns what is left to its tightest box, once per kept
part and before sampling: the input is centred and scaled by its AXIS-ALIGNED box and the mesh lies on a 128-step lattice along the same
axes, so a scan that sits askew in its file wastes resolution on empty corners and shows the decoder a turned shape.  H rotations from a
private generator (the numpy RNG is not touched) are scored on the GPU by the volume of the box around the turned points
(`meshanything_amd/pc_align.py`), over all rotations first and then `--align_rounds` times (default 4, 0..8) over ever smaller balls about
the best so far, whose radii follow from H.  Of the 24 equivalent frames of a box the one nearest the file's is taken, so an up that is
roughly right stays up; unless the box shrinks by more than `--align_min_gain` (default 0.02, in [0, 1)) the input keeps its axes: a
ball has no orientation to find.  One line per part reports the angle, the axis and the box volumes.  The mesh is written in the aligned
frame, except with `--cluster_mode split`, whose files are in the INPUT's coordinates as before.
`--register_dist D` (with pc_normal and pc_xyz; 0 = off, the default; in the units of the input files) takes objects that come as several
partial scans, each in its own, roughly known, pose: a sub-directory of `--input_dir`, or a directory given as `--input_path`, is ONE object,
its point files in sorted order are its scans and its name names the output.  The first scan is the frame; every further scan is moved
onto the union of the ones before it by ICP on the GPU (`meshanything_amd/pc_register.py`): per iteration the nearest point within D of
every point, over the same cell grid, and a least-squares step on the point-to-plane distances (`--register_metric point`: point-to-point,
for clouds without usable normals; pc_xyz scans get normals from `--normal_k` neighbours within each scan), at most `--register_iters`
times (default 30, 1..256) or until the RMS changes by at most `--register_tol` of itself (default 1e-6, in [0, 1)).  The scans must start
within D of their place: a scan of whose points less than `--register_min_overlap` (default 0.3, in (0, 1]) find a partner is an error, not
a guess.  With `--voxel_size` each scan is thinned before, and the union again after, where overlapping scans doubled the density.  One
line per scan reports iterations, the paired share, the RMS and the motion.  No loop closure.
`--coarse_radius F` (with `--register_dist`; 0 = off, the default; in the units of the input files) is for scans in UNKNOWN poses -- a
turntable without an encoder, a hand-held scanner, files exported one by one: every scan's ICP then starts not from the file's frame but
from a coarse pose found on the GPU (`meshanything_amd/pc_coarse.py`).  `--coarse_points` (default 1024, 64..4096) farthest-point keypoints
are picked on the scan and on the union before it; every point gets a histogram of three angle features over the points within F of it
(PCL's and Open3D's FPFH without the signs, which unoriented normals do not have, and without distance weights, so that it is integer and
exact), summed once more over the same neighbourhood at the keypoints; the descriptors are matched both ways and the mutual matches kept;
`--coarse_iters` (default 4096, 256..65536) triples of matches from a private generator, less those whose triangles do not match in edge
length, each give a pose, and the pose with which the most matches land within `--coarse_dist` (default F / 4) of their partner wins and is
refitted to them.  F should span several point spacings and a fraction of the object.  One more line per scan reports the matches, the
surviving triples, the agreeing matches and the turn.  Too few matches or agreeing pairs is an error, not a guess.  Out of its reach: a
solid of large flat faces, whose descriptors all look alike, and a nearly symmetric one, whose half-turn twin overlaps as well as the truth
-- no overlap check can tell them apart.
`--fit_iters K` (every input type; 0 = off, the default; 1..32) is the one step AFTER the decoder that moves a vertex: the generated vertices
lie on the detokenizer's 128-step lattice, up to half a step per axis off the surface, and the 4096 rows the encoder saw know that surface
far better.  K damped Gauss-Newton steps of the point-to-plane fit pull the merged vertices onto them (`meshanything_amd/mesh_fit.py`): per
step every row is paired on the GPU with the nearest face within `--fit_dist` (default 4 lattice steps, at most 64; one step is 1/128 of the
mesh box), optionally only with faces whose normal agrees with the row's to `--fit_normal_cos` (default 0 = off, in [0, 1)), the per-face
sums of the normal equations come back as exact integers and the host solves the vertex system in float64, each vertex held in place with
the weight of `--fit_stiffness` points (default 1).  No vertex leaves the ball of `--fit_max_move` (default 2 steps, at most --fit_dist)
about where the decoder put it, and one without paired rows stays put.  With `--num_candidates` only the chosen mesh is fitted.  The fit is
kept only if the mean of the two directed distances between mesh and cloud fell, else the decoder's vertices are written: a refusal, not a
guess; one line per mesh reports the pairs, the RMS before and after, the largest move and which it was.  Faces are not re-merged.  The
defaults follow from the lattice, not from released weights, which nobody could try offline.
Multi-GPU: one process per GPU; rank r takes the shapes i % world == r and the weights travel in one RCCL broadcast.
"""
import argparse
import datetime
import os
import time

# multi-process GPU work on this driver stack needs dmabuf IPC (RCCL / tensor sharing fail with the legacy mode); keep a caller's value
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


# The input steps whose switch is a distance or, for --align_iters, a count (0 = off), in the order their errors are reported: the switch, then the flags that need it as
# {flag: (default, range test or None, the range's wording)}.  The fifth step's --outlier_k and --outlier_std follow another pattern, below.
STEP_FLAGS = (
    ("upsample_radius", {"upsample_points": (4 * 4096, lambda v: 4096 <= v <= 1 << 22, "in 4096..4194304")}),
    ("smooth_radius", {"smooth_iters": (1, lambda v: 1 <= v <= 8, "in 1..8")}),
    ("plane_threshold", {"plane_iters": (1024, lambda v: 1 <= v <= 65536, "in 1..65536"), "plane_count": (1, lambda v: 1 <= v <= 8, "in 1..8"),
                         "plane_min_fraction": (0.2, lambda v: 0.0 < v <= 1.0, "in (0, 1]")}),
    ("cluster_radius", {"cluster_mode": ("largest", None, None), "cluster_min_points": (4096, None, None)}),   # its two floors: after the table
    ("voxel_size", {}),
    ("align_iters", {"align_rounds": (4, lambda v: 0 <= v <= 8, "in 0..8"), "align_min_gain": (0.02, lambda v: 0.0 <= v < 1.0, "in [0, 1)")}),
    ("register_dist", {"register_iters": (30, lambda v: 1 <= v <= 256, "in 1..256"), "register_tol": (1e-6, lambda v: 0.0 <= v < 1.0, "in [0, 1)"),
                       "register_metric": ("plane", None, None), "register_min_overlap": (0.3, lambda v: 0.0 < v <= 1.0, "in (0, 1]")}),
    ("coarse_radius", {"coarse_points": (1024, lambda v: 64 <= v <= 4096, "in 64..4096"), "coarse_iters": (4096, lambda v: 256 <= v <= 65536, "in 256..65536"),
                       "coarse_dist": (None, lambda v: 0.0 < v < float("inf"), "finite and > 0")}),       # its need of --register_dist: after the table
)


# The mesh fit after the decoder (--fit_iters, 0 = off): the flags that need it, worded like the table above.  Not an input step: it is
# no part of CloudPrep or Dataset.  Distances are in lattice steps of the decoder.
FIT_FLAGS = {"fit_dist": (4.0, lambda v: 0.0 < v <= 64.0, "finite, > 0 and at most 64 (lattice steps)"),
             "fit_max_move": (2.0, lambda v: 0.0 < v < float("inf"), "finite and > 0"),
             "fit_stiffness": (1.0, lambda v: 0.0 < v < float("inf"), "finite and > 0"),
             "fit_normal_cos": (0.0, lambda v: 0.0 <= v < 1.0, "in [0, 1) (0 = off)")}


def _listed(flags) -> str:
    return flags[0] if len(flags) == 1 else ", ".join(flags[:-1]) + " and " + flags[-1]


def get_args(argv=None):
    p = argparse.ArgumentParser("MeshAnything", add_help=True)
    p.add_argument("--llm", default="facebook/opt-350m", type=str)
    p.add_argument("--input_dir", default=None, type=str)
    p.add_argument("--input_path", default=None, type=str)
    p.add_argument("--out_dir", default="inference_out", type=str)
    p.add_argument("--pretrained_weights", default="MeshAnything_350m.pth", type=str)
    p.add_argument("--input_type", choices=["mesh", "pc_normal", "pc_xyz"], default="pc", help="Type of the asset to process (default: pc)")
    p.add_argument("--codebook_size", default=8192, type=int)
    p.add_argument("--codebook_dim", default=1024, type=int)
    p.add_argument("--n_max_triangles", default=800, type=int)
    p.add_argument("--batchsize_per_gpu", default=1, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--mc", default=False, action="store_true")
    p.add_argument("--sampling", default=False, action="store_true")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--gpu_sampling", default=False, action="store_true",
                   help="sample mesh inputs (and the --mc surface) on the GPU: the same draws and clouds as the host sampler")
    p.add_argument("--synthetic_weights", default=False, action="store_true", help="seeded random checkpoint (no released file offline)")
    p.add_argument("--num_candidates", default=1, type=int,
                   help="with --sampling: draw this many meshes per input in one batch and keep the one closest to the input cloud")
    p.add_argument("--normal_k", default=16, type=int, help="with --input_type pc_xyz: neighbours per point in the normal estimate (3..32)")
    p.add_argument("--normal_weight", default=0.0, type=float,
                   help="with --num_candidates > 1: add this times (1 - normal consistency with the cloud's normals) to a candidate's total")
    p.add_argument("--orient", default="volume", choices=["volume", "cloud"],
                   help="winding of the written faces: by signed volume (fix_normals, the reference) or by the cloud's normals")
    p.add_argument("--point_sampling", default="random", choices=["random", "fps"],
                   help="with --input_type pc_normal / pc_xyz: which 4096 rows of the input to keep: a uniform draw (the reference) or farthest-point sampling on the GPU")
    p.add_argument("--outlier_k", default=0, type=int,
                   help="with --input_type pc_normal / pc_xyz: remove statistical outliers first, from this many neighbours per point (3..32; 0 = off)")
    p.add_argument("--outlier_std", default=2.0, type=float,
                   help="with --outlier_k: drop a point whose mean neighbour distance exceeds the cloud's mean by more than this many standard deviations")
    p.add_argument("--cluster_radius", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: split the input into the connected parts of the graph that links points at most this "
                        "far apart, in the units of the input file, and drop the small ones (0 = off)")
    p.add_argument("--cluster_mode", default=None, choices=["largest", "split"],
                   help="with --cluster_radius: mesh the largest part only (the default), or every kept part, written in the input's coordinates")
    p.add_argument("--cluster_min_points", default=None, type=int,
                   help="with --cluster_radius: drop the parts of fewer points than this (default 4096, the rows the encoder takes)")
    p.add_argument("--plane_threshold", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: remove the dominant plane (a table, a floor) before clustering: the rows within this "
                        "distance of it, in the units of the input file (0 = off)")
    p.add_argument("--plane_iters", default=None, type=int,
                   help="with --plane_threshold: RANSAC hypotheses per plane (1..65536, default 1024); raise it when you lower --plane_min_fraction: a plane "
                        "holding a fraction w of the rows is missed by n draws with probability (1 - w^3)^n")
    p.add_argument("--plane_count", default=None, type=int, help="with --plane_threshold: remove up to this many planes, one after the other (1..8, default 1)")
    p.add_argument("--plane_min_fraction", default=None, type=float,
                   help="with --plane_threshold: stop when the best plane holds less than this fraction of the remaining rows (in (0, 1], default 0.2)")
    p.add_argument("--smooth_radius", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: smooth the input last of the cleaning steps: project every point onto the plane fitted to "
                        "the points within this distance of it, in the units of the input file (0 = off)")
    p.add_argument("--smooth_iters", default=None, type=int, help="with --smooth_radius: smoothing passes (1..8, default 1)")
    p.add_argument("--upsample_radius", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: upsample a sparse input after the cleaning steps: add lattice points in the plane fitted to "
                        "the points within this distance of each point, in the units of the input file, each kept where its own point is the nearest "
                        "(0 = off).  The patches are flat, an open border grows outward by up to this distance, and at a sharp edge the patch sticks "
                        "out: choose about one to two point spacings, and use --point_sampling fps, which thins the uneven density evenly")
    p.add_argument("--upsample_points", default=None, type=int,
                   help="with --upsample_radius: upsample an input of fewer points to at least this many (4096..4194304, default 16384 = 4 x 4096)")
    p.add_argument("--voxel_size", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: thin a dense input first, on the GPU: keep one point per cube of this edge, in the units of "
                        "the input file, the one nearest the cube's centre (0 = off).  The only step that takes more than 4194304 points (up to "
                        "268435456); at most 4194304 cubes may be occupied")
    p.add_argument("--align_iters", default=0, type=int,
                   help="with --input_type pc_normal / pc_xyz: turn the input into the frame of its tightest box before sampling: this many rotations "
                        "per round, scored on the GPU by the volume of the box around the turned points (256..65536; 0 = off)")
    p.add_argument("--align_rounds", default=None, type=int,
                   help="with --align_iters: refinement rounds after the one over all rotations, each over a smaller ball about the best so far (0..8, default 4)")
    p.add_argument("--align_min_gain", default=None, type=float,
                   help="with --align_iters: keep the file's axes unless the box shrinks by more than this fraction (in [0, 1), default 0.02)")
    p.add_argument("--register_dist", default=0.0, type=float,
                   help="with --input_type pc_normal / pc_xyz: a directory (--input_path, or a sub-directory of --input_dir) is one object and its point "
                        "files are partial scans: register each onto the ones before it by ICP on the GPU, pairing points at most this far apart, in the "
                        "units of the input files, and merge them (0 = off)")
    p.add_argument("--register_iters", default=None, type=int, help="with --register_dist: ICP iterations per scan at the most (1..256, default 30)")
    p.add_argument("--register_tol", default=None, type=float,
                   help="with --register_dist: stop when the RMS changes by at most this fraction of itself (in [0, 1), default 1e-6)")
    p.add_argument("--register_metric", default=None, choices=["plane", "point"],
                   help="with --register_dist: point-to-plane distances (the default) or point-to-point, for clouds without usable normals")
    p.add_argument("--register_min_overlap", default=None, type=float,
                   help="with --register_dist: refuse a scan of whose points less than this fraction find a partner (in (0, 1], default 0.3)")
    p.add_argument("--coarse_radius", default=0.0, type=float,
                   help="with --register_dist: the scans are in UNKNOWN poses: start every scan's ICP from a pose found on the GPU by matching feature "
                        "histograms over the points within this distance of each keypoint, in the units of the input files: several point spacings, "
                        "a fraction of the object (0 = off).  Large flat faces and near-symmetric objects are out of its reach")
    p.add_argument("--coarse_points", default=None, type=int, help="with --coarse_radius: farthest-point keypoints per cloud (64..4096, default 1024)")
    p.add_argument("--coarse_iters", default=None, type=int, help="with --coarse_radius: pose hypotheses, each from three matches (256..65536, default 4096)")
    p.add_argument("--coarse_dist", default=None, type=float,
                   help="with --coarse_radius: a matched pair agrees with a hypothesis when it lands within this distance (default --coarse_radius / 4)")
    p.add_argument("--fit_iters", default=0, type=int,
                   help="fit the generated mesh to the input's 4096 rows on the GPU: this many point-to-plane Gauss-Newton steps on the merged "
                        "vertices, kept only if the mesh came closer to the cloud (1..32; 0 = off)")
    p.add_argument("--fit_dist", default=None, type=float,
                   help="with --fit_iters: pair a row with the nearest face at most this far away, in lattice steps of 1/128 of the mesh box (default 4, at most 64)")
    p.add_argument("--fit_max_move", default=None, type=float,
                   help="with --fit_iters: no vertex moves further than this from where the decoder put it, in lattice steps (default 2, at most --fit_dist)")
    p.add_argument("--fit_stiffness", default=None, type=float,
                   help="with --fit_iters: every vertex is held in place with the weight of this many paired rows (default 1.0)")
    p.add_argument("--fit_normal_cos", default=None, type=float,
                   help="with --fit_iters: pair a row only with faces whose normal agrees with the row's to at least this |cosine| (in [0, 1), default 0 = off)")
    args = p.parse_args(argv)
    for switch, others in STEP_FLAGS:
        flags = [f"--{name}" for name in (switch, *others)]
        given = [getattr(args, name) is not None for name in others]
        if not (0.0 <= getattr(args, switch) < float("inf")):
            p.error(f"{flags[0]} must be finite and >= 0 (0 = off)")
        if args.input_type == "mesh" and (getattr(args, switch) != 0 or any(given)):
            p.error(f"{_listed(flags)} appl{'y' if others else 'ies'} to --input_type pc_normal and pc_xyz, not to mesh inputs")
        if getattr(args, switch) == 0 and any(given):
            p.error(f"{_listed(flags[1:])} need{'s' if len(others) == 1 else ''} {flags[0]} > 0")
        for name, (default, ok, wording) in others.items():
            if getattr(args, name) is None:
                setattr(args, name, default)
            elif ok is not None and not ok(getattr(args, name)):
                p.error(f"--{name} must be {wording}")
    if not 0 <= args.fit_iters <= 32:
        p.error("--fit_iters must be 0 (off) or in 1..32")
    if args.fit_iters == 0 and any(getattr(args, name) is not None for name in FIT_FLAGS):
        named = [f"--{name}" for name in FIT_FLAGS if getattr(args, name) is not None]
        p.error(f"{_listed(named)} need{'s' if len(named) == 1 else ''} --fit_iters > 0")
    for name, (default, ok, wording) in FIT_FLAGS.items():
        if args.fit_iters == 0:
            continue                                     # off: the flags stay None, nothing reads them
        if getattr(args, name) is None:
            setattr(args, name, default)
        elif not ok(getattr(args, name)):
            p.error(f"--{name} must be {wording}")
    if args.fit_iters > 0 and args.fit_max_move > args.fit_dist:
        p.error("--fit_max_move must be at most --fit_dist")
    if args.coarse_radius > 0 and args.register_dist == 0:
        p.error("--coarse_radius needs --register_dist > 0: the coarse pose is where a scan's registration starts")
    if args.align_iters != 0 and not 256 <= args.align_iters <= 65536:
        p.error("--align_iters must be 0 (off) or in 256..65536")
    if args.upsample_radius > 0 and args.cluster_min_points < 64:            # the default passes both
        p.error("--cluster_min_points must be at least 64, the rows upsampling takes")
    if args.upsample_radius == 0 and args.cluster_min_points < 4096:
        p.error("--cluster_min_points must be at least 4096, the rows the uniform draw needs")
    if args.outlier_k != 0 and not 3 <= args.outlier_k <= 32:
        p.error("--outlier_k must be 0 (off) or in 3..32")
    if not (0.0 <= args.outlier_std < float("inf")):
        p.error("--outlier_std must be finite and >= 0")
    if args.outlier_k != 0 and args.input_type == "mesh":
        p.error("--outlier_k applies to --input_type pc_normal and pc_xyz, not to mesh inputs")
    if args.point_sampling == "fps" and args.input_type == "mesh":
        p.error("--point_sampling fps applies to --input_type pc_normal and pc_xyz, not to mesh inputs")
    if not 3 <= args.normal_k <= 32:
        p.error("--normal_k must be in 3..32")
    if args.num_candidates < 1:
        p.error("--num_candidates must be >= 1")
    if args.num_candidates > 1 and not args.sampling:
        p.error("--num_candidates > 1 needs --sampling (greedy candidates are identical)")
    if not (0.0 <= args.normal_weight < float("inf")):
        p.error("--normal_weight must be finite and >= 0")
    if args.normal_weight > 0 and args.num_candidates < 2:
        p.error("--normal_weight > 0 needs --num_candidates > 1")
    return args


def main():
    from meshanything_amd import dp
    from meshanything_amd.checkpoint import load_safetensors_items, synthetic_items
    from meshanything_amd.cloud_prep import CloudPrep
    from meshanything_amd.data import Dataset, to_file_frame, uid_of
    from meshanything_amd.mesh_export import faces_from_coords, fix_normals, merge_meshes, write_obj
    from meshanything_amd.model import MeshAnything

    args = get_args()
    rank, world, local = dp.init_process_group()
    cur_time = datetime.datetime.now().strftime("%d_%H-%M-%S")
    out_dir = os.path.join(args.out_dir, cur_time)
    os.makedirs(out_dir, exist_ok=True)

    torch.cuda.set_device(local)
    model = MeshAnything(args, device=local)
    print("load model over!!!")
    items = (lambda: synthetic_items(model.cfg)) if args.synthetic_weights else (lambda: load_safetensors_items(args.pretrained_weights))
    dp.load_weights_dp(model.engine, items, rank, world)
    print("load weights over!!!")

    if args.input_dir is not None:
        input_list = sorted(os.listdir(args.input_dir))
        scans = [os.path.join(args.input_dir, x) for x in input_list if args.register_dist > 0 and os.path.isdir(os.path.join(args.input_dir, x))]
        if args.input_type == "pc_normal":
            input_list = [os.path.join(args.input_dir, x) for x in input_list if x.endswith(".npy") or x.lower().endswith(".ply")]
        elif args.input_type == "pc_xyz":
            input_list = [os.path.join(args.input_dir, x) for x in input_list if x.lower().endswith((".npy", ".xyz", ".txt", ".ply"))]
        else:                                    # main.py:125-128 keeps .ply / .obj / .npy for meshes; .npy is not a mesh file, .off / .stl are read too
            input_list = [os.path.join(args.input_dir, x) for x in input_list if x.lower().endswith((".ply", ".obj", ".off", ".stl"))]
        input_list = sorted(input_list + scans)              # --register_dist: a sub-directory is one object, its files its scans
    elif args.input_path is not None:
        input_list = [args.input_path]
    else:
        raise ValueError("input_dir or input_path must be provided.")
    np.random.seed(args.seed)                    # accelerate.set_seed(args.seed) before Dataset (main.py:129-133)
    torch.manual_seed(args.seed)
    sample_device = "cuda" if args.gpu_sampling else None     # the current device: torch.cuda.set_device(local) above
    if args.input_type == "mesh" and args.mc:
        # main.py:29-39 with --mc: every rank remeshes every input, in file order, so that the global numpy RNG is consumed as in a
        # one-process run (the sampling draws from it after each shape)
        from meshanything_amd.mesh_input import load_mesh
        from meshanything_amd.watertight import process_mesh_to_pc
        meshes = [load_mesh(p) for p in input_list]
        print("First Marching Cubes and then sample point cloud, need several minutes...")
        pc_list, _ = process_mesh_to_pc(meshes, marching_cubes=True, device=sample_device)
        dataset = Dataset.from_clouds(pc_list, [uid_of(p) for p in input_list])
    else:
        dataset = Dataset(args.input_type, input_list, args.mc, sample_device=sample_device, **vars(CloudPrep.from_args(args)))

    begin = time.time()
    print("Generation Start!!!")
    split = args.cluster_radius > 0 and args.cluster_mode == "split"
    groups = dataset.groups() if split else None
    group_parts = {}                                 # --cluster_mode split: a group's parts so far, in part order (one rank holds a whole group)
    mine = dp.shard_grouped(groups, rank, world) if split else dp.shard_indices(len(dataset), rank, world)
    for batch in dp.batches(mine, args.batchsize_per_gpu):
        data = [dataset[i] for i in batch]
        pc = torch.from_numpy(np.stack([d["pc_normal"] for d in data])).cuda()
        orient = "cloud" if args.orient == "cloud" else None
        if args.num_candidates > 1:
            det = model.forward_detailed(pc, sampling=True, num_candidates=args.num_candidates, normal_weight=args.normal_weight, orient=orient)
            outputs = det["coords"].cpu().numpy()
            ncs = det["normal_scores"][..., 0].tolist() if args.normal_weight > 0 else [None] * len(data)
            for d, c, tot, nc in zip(data, det["chosen"].tolist(), det["total"].tolist(), ncs):
                line = f'{d["uid"]}: candidate {c} of {args.num_candidates} chosen, totals ' + " ".join(f"{t:.6f}" for t in tot)
                print(line if nc is None else line + ", NC " + " ".join(f"{v:.6f}" for v in nc))
        else:
            outputs = model(pc, sampling=args.sampling, orient=orient).cpu().numpy()
        for i, d, coords in zip(batch, data, outputs):
            verts, faces = faces_from_coords(coords)
            if args.fit_iters > 0 and len(faces):        # the merged vertices onto the rows the encoder saw; the faces stay as they are
                from meshanything_amd.mesh_fit import fit_mesh, report_line
                verts, fit = fit_mesh(verts, faces, d["pc_normal"], args.fit_iters, args.fit_dist, args.fit_max_move, args.fit_stiffness, args.fit_normal_cos)
                print(report_line(d["uid"], fit))
            if orient is None:                       # --orient cloud: the winding came with the coordinates
                faces = fix_normals(verts, faces)
            if split:                                # into the input file's frame, in float64, out of the aligned one if --align_iters turned the part
                verts = to_file_frame(verts, d["frame"], d.get("pose"))
            path = os.path.join(out_dir, f'{d["uid"]}_gen.obj')
            write_obj(path, verts, faces)
            print(f"{path} Over!!")
            if split:
                parts = group_parts.setdefault(groups[i], [])
                parts.append((verts, faces))
                if len(parts) == groups.count(groups[i]):            # the group's last part: the parts in one file, nothing merged across them
                    path = os.path.join(out_dir, f'{d["group"]}_gen.obj')
                    write_obj(path, *merge_meshes(group_parts.pop(groups[i])))
                    print(f"{path} Over!!")
    print(f"Total time: {time.time() - begin}")
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
