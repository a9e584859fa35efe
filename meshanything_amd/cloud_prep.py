"""What happens to the rows of a pc_normal or pc_xyz file between loading and the pick of the rows the encoder takes: six optional steps on
the GPU, none of which the reference has.  `CloudPrep` holds their options, `STAGES` lists them in the order they run, and each stage's
function states its contract.  A step is on when its switch field is non-zero.  Off: no code path, key, print, floor or draw from the numpy
RNG changes, and its module (pc_*.py, which needs torch) is not imported.  On: the step is looked up in its module at each call; with "mesh"
inputs it is a ValueError.  No step draws from the global numpy RNG.  A stage function takes (its module, the options, parts, n_points, device)
and returns parts: [(the rows that stand in for the file, the item's keys besides the cloud)], one entry until clustering splits the file.
Voxel thinning comes first because it is the only step that takes more than 2^22 rows (up to 2^28): it is what lets a dense scan in at all,
and every later step costs less on what it leaves.  The outlier statistic then sees an even density, which it assumes; strays survive
thinning one per voxel while the surface loses most of its rows, so the strays' share of the cloud RISES and the outlier filter after it
matters more, not less.  After the six, and before the pick, comes a step of its own kind, `POSE` (align_iters): it drops and adds no row but
turns every kept part into the frame of its tightest box, and the part's keys gain "pose", with which the turn can be undone.  BEFORE the six
comes another step of its own kind, `SCANS` (register_dist): an input that is a directory of partial scans becomes one cloud in the frame of
its first scan (pc_register.register_rows); `data.Dataset` runs it, since it is the only step that takes several files.  coarse_radius is an
option OF that step, not a stage: with it every scan's registration starts from a pose found by pc_coarse.coarse_pose, for scans in unknown poses."""
from __future__ import annotations

import importlib
from dataclasses import dataclass, fields
from typing import Callable, NamedTuple, Optional


def voxel(m, p, parts, n_points, device):
    """voxel_size=L: uniform voxel thinning, once per file and before anything else (pc_voxel.thin_rows, N <= 2^28, finite): of the rows in
    one voxel of edge L (file units), counted from the cloud's per-axis minimum, the one nearest the voxel's centre survives, the lowest row
    among equals; at most 2^22 voxels may be occupied.  The survivors keep their order and their columns.  Fewer than the floor is a ValueError."""
    return [(m.thin_rows(rows, p.voxel_size, p.floor(n_points), keys["uid"], device=device), keys) for rows, keys in parts]


def outliers(m, p, parts, n_points, device):
    """outlier_k=K: statistical outlier removal, the first of the cleaning steps (pc_outliers.remove_statistical_outliers, K neighbours, N <= 2^22, finite):
    the rows whose mean distance to their K nearest neighbours exceeds the cloud's mean by more than outlier_std standard deviations are
    dropped; the survivors keep their order.  Fewer survivors than the floor is a ValueError."""
    return [(m.filter_rows(rows, p.outlier_k, p.outlier_std, p.floor(n_points), keys["uid"], device=device), keys) for rows, keys in parts]


def plane(m, p, parts, n_points, device):
    """plane_threshold=T: dominant-plane removal (pc_plane.remove_planes, N <= 2^22, finite): up to plane_count times, plane_iters RANSAC
    hypotheses from a private generator are scored against the rows still kept, the one that holds the most rows within T (file units) is
    refitted to them and its inliers are dropped; a best plane that holds fewer than plane_min_fraction of the rows ends the search.  It comes
    after the outlier filter, which keeps a table, and before clustering, which cannot part it from the object.  An object's own large flat
    face is a plane too: plane_min_fraction and the opt-in are the only guard.  The survivors keep their order.  Fewer than the floor is a ValueError."""
    return [(rows[m.remove_planes(rows, p.plane_threshold, p.plane_iters, p.plane_count, p.plane_min_fraction, p.floor(n_points), keys["uid"], device=device)],
             keys) for rows, keys in parts]


def cluster(m, p, parts, n_points, device):
    """cluster_radius=R: Euclidean clustering (pc_cluster.split_rows, N <= 2^22, finite): the rows fall into the connected components of the
    graph that links two rows at most R apart, and the components of fewer than cluster_min_points rows (at least the floor) are dropped.
    Every kept component then stands in for the file's rows.  cluster_mode "largest": the largest component only, one item, uid unchanged.
    "split": one item per kept component, adjacent, largest first, with uid "{uid}_part{j}" and the extra keys "group" (the file's uid) and
    "part" (j); `Dataset.__getitem__` adds "frame", with which main.py maps the part's mesh back into the file's coordinates.  No component of
    cluster_min_points rows is a ValueError."""
    out = []
    for rows, keys in parts:
        uid = keys["uid"]
        kept = m.split_rows(rows, p.cluster_radius, p.cluster_min_points, p.cluster_mode, uid, device=device)
        if p.cluster_mode == "largest":
            out.append((rows[kept[0]], keys))
        else:
            out += [(rows[r], {"uid": f"{uid}_part{j}", "group": uid, "part": j}) for j, r in enumerate(kept)]
    return out


def smooth(m, p, parts, n_points, device):
    """smooth_radius=R: moving-least-squares smoothing, once per kept part (pc_smooth.smooth_rows, N <= 2^22, finite): every row is projected
    onto the plane fitted to the rows within R of it (file units), smooth_iters times (1..8), and a file's normals are replaced by the
    fitted ones on the file's side.  The last of the cleaning steps: the strays and the table are gone by then and cannot pull the fit."""
    return [(m.smooth_rows(rows, p.smooth_radius, p.smooth_iters, keys["uid"], device=device), keys) for rows, keys in parts]


def upsample(m, p, parts, n_points, device):
    """upsample_radius=R: upsampling of a SPARSE cloud, once per kept part (pc_upsample.upsample_rows): a part of fewer than upsample_points
    rows (default 4 * n_points, n_points..2^22) gains lattice points at spacing R / m in the plane fitted to the rows within R of each row
    (file units), each kept where its own row is the nearest, m the first of 2, 4, ..., 64 that reaches upsample_points; a new row is a copy of
    its seed's row with xyz replaced, so a file's normals are the seed's.  With it, and only then, the floor on the rows of a file, of the
    outlier filter's and plane removal's survivors and of cluster_min_points is pc_upsample.MIN_ROWS = 64 instead of n_points; fewer than
    n_points rows after upsampling is a ValueError.  pc_upsample.py says what the patches look like and why point_sampling="fps" suits them."""
    floor, out = p.floor(n_points), []
    for rows, keys in parts:
        if rows.shape[0] < floor:
            raise ValueError(f"{keys['uid']}: upsampling takes at least {floor} rows, got {rows.shape[0]}")
        rows = m.upsample_rows(rows, p.upsample_radius, p.upsample_target(n_points), keys["uid"], device=device)
        if rows.shape[0] < n_points:
            raise ValueError(f"{keys['uid']}: upsampling left {rows.shape[0]} rows, fewer than the {n_points} the encoder takes")
        out.append((rows, keys))
    return out


def align(m, p, parts, n_points, device):
    """align_iters=H: alignment to the tightest box, once per kept part, on what upsampling left and before the pick (pc_align.align_rows,
    N <= 2^22, finite): 1 + align_rounds times (rounds 0..8), H rotations (256..65 536) from a private generator are scored on the GPU by the
    volume of the part's axis-aligned box under them, all rotations first and then ever smaller balls about the best so far; if the best
    box is smaller than the file's by more than align_min_gain (in [0, 1)), the part is turned about its bounding-box mid-point c into the
    frame R' of that box, the one of its 24 equivalents nearest the file's, normals included, else it is left as it is.  The keys gain
    "pose": (R', c), which `Dataset.__getitem__` passes on and `data.to_file_frame` undoes.  Not one of STAGES: no row comes or goes."""
    out = []
    for rows, keys in parts:
        rows, pose = m.align_rows(rows, p.align_iters, p.align_rounds, p.align_min_gain, keys["uid"], device=device)
        out.append((rows, {**keys, "pose": pose}))
    return out


def register(m, p, scans, names, uid, normal_k, device):
    """register_dist=D: registration of the scans of one object, before anything else but each scan's own voxel thinning
    (pc_register.register_rows, every scan >= 64 rows, the union <= 2^22, finite): scan 0 is the frame; scan j is moved onto the union of
    the scans before it by at most register_iters (1..256) iterations of ICP with pairing distance D (file units), the point-to-plane
    metric ("point": point-to-point) and the relative RMS tolerance register_tol (in [0, 1)); a scan of whose rows less than
    register_min_overlap (in (0, 1]) end up paired is a ValueError.  -> (the merged rows, [(R, t)] float64 per scan).  Not one of STAGES: it
    takes several files and runs before a file's rows exist.
    coarse_radius=F (file units) on top of it: scans in UNKNOWN poses.  Scan j's ICP then starts from `pc_coarse.coarse_pose` against the union:
    coarse_points (64..4096) farthest-point keypoints a cloud, a feature histogram over the rows within F of each, matched both ways, and
    coarse_iters (256..65536) triples of matches scored by the matches within coarse_dist (None = F / 4) of where the triple's pose puts them.
    Off, `register_rows` gets exactly the call it got before the stage existed."""
    args = (scans, p.register_dist, p.register_iters, p.register_tol, p.register_metric, p.register_min_overlap, normal_k, uid)
    if not p.coarse_radius:
        return m.register_rows(*args, device=device, names=names)
    return m.register_rows(*args, device=device, names=names, coarse=(p.coarse_radius, p.coarse_points, p.coarse_iters, p.coarse_dist))


def check_cluster(m, p, n_points):
    m.check_split_args(p.cluster_radius, p.cluster_min_points, p.cluster_mode)
    if p.cluster_min_points < p.floor(n_points):
        raise ValueError(f"cluster_min_points = {p.cluster_min_points} is less than the {p.floor(n_points)} rows " +
                         ("upsampling takes" if p.upsample_radius else "the encoder takes"))


class Stage(NamedTuple):
    switch: str                                                  # the CloudPrep field that turns it on
    module: str
    check: Callable                                              # (module, options, n_points): the argument check, before any file is read
    apply: Callable
    mesh: str = "applies to pc_normal and pc_xyz inputs: the points of a mesh input are drawn from its surface"


STAGES = (                                                       # in the order they run; every stage sees what the one before it left
    Stage("voxel_size", "pc_voxel", lambda m, p, n: m.check_voxel_args(p.voxel_size), voxel),
    Stage("outlier_k", "pc_outliers", lambda m, p, n: m.check_filter_args(p.outlier_k, p.outlier_std), outliers),
    Stage("plane_threshold", "pc_plane", lambda m, p, n: m.check_remove_args(p.plane_threshold, p.plane_iters, p.plane_count, p.plane_min_fraction), plane),
    Stage("cluster_radius", "pc_cluster", check_cluster, cluster),
    Stage("smooth_radius", "pc_smooth", lambda m, p, n: m.check_smooth_args(p.smooth_radius, p.smooth_iters), smooth),
    Stage("upsample_radius", "pc_upsample", lambda m, p, n: m.check_upsample_args(p.upsample_radius, p.upsample_target(n), n), upsample),
)                                                                # then POSE, then the pick: the uniform draw, FPS, or the pc_xyz normal estimate (data.Dataset)
POSE = Stage("align_iters", "pc_align", lambda m, p, n: m.check_align_args(p.align_iters, p.align_rounds, p.align_min_gain), align)
SCANS = Stage("register_dist", "pc_register",
              lambda m, p, n: m.check_register_args(p.register_dist, p.register_iters, p.register_tol, p.register_metric, p.register_min_overlap), register)


@dataclass(frozen=True)
class CloudPrep:
    """The options of the input side.  normal_k: the neighbours of the pc_xyz normal estimate.  point_sampling "fps" (the reference has nothing
    like it): the n_points rows are the ones farthest-point sampling keeps (pc_fps.farthest_point_sample over the first three columns as
    float32, N <= 2^22, finite), in pick order, instead of a uniform draw: a scan's density follows the scanner, and a uniform draw leaves its
    thin parts a handful of points.  Such an input consumes no draws from the numpy RNG.  With "mesh" it is a ValueError.  The rest: STAGES."""
    normal_k: int = 16
    point_sampling: str = "random"
    outlier_k: int = 0
    outlier_std: float = 2.0
    plane_threshold: float = 0.0
    plane_iters: int = 1024
    plane_count: int = 1
    plane_min_fraction: float = 0.2
    cluster_radius: float = 0.0
    cluster_mode: str = "largest"
    cluster_min_points: int = 4096
    smooth_radius: float = 0.0
    smooth_iters: int = 1
    upsample_radius: float = 0.0
    upsample_points: Optional[int] = None
    voxel_size: float = 0.0
    align_iters: int = 0
    align_rounds: int = 4
    align_min_gain: float = 0.02
    register_dist: float = 0.0
    register_iters: int = 30
    register_tol: float = 1e-6
    register_metric: str = "plane"
    register_min_overlap: float = 0.3
    coarse_radius: float = 0.0
    coarse_points: int = 1024
    coarse_iters: int = 4096
    coarse_dist: Optional[float] = None

    @classmethod
    def from_args(cls, args) -> "CloudPrep":
        """From main.get_args' namespace, whose --upsample_points default is filled in even with upsampling off."""
        return cls(**{f.name: getattr(args, f.name) for f in fields(cls) if f.name != "upsample_points" or args.upsample_radius > 0})

    def on(self):
        """The stages that are on, each with its module."""
        return [(s, importlib.import_module(f".{s.module}", __package__)) for s in STAGES if getattr(self, s.switch)]

    def pose(self):
        """[(POSE, its module)] if alignment is on, else []."""
        return [(POSE, importlib.import_module(f".{POSE.module}", __package__))] if self.align_iters else []

    def scans(self):
        """[(SCANS, its module)] if registration is on, else []."""
        return [(SCANS, importlib.import_module(f".{SCANS.module}", __package__))] if self.register_dist else []

    def floor(self, n_points: int) -> int:
        """The fewest rows a file, and what a step leaves of it, may have."""
        return min(importlib.import_module(".pc_upsample", __package__).MIN_ROWS, n_points) if self.upsample_radius else n_points

    def upsample_target(self, n_points: int) -> int:
        return 4 * n_points if self.upsample_points is None else self.upsample_points

    def check(self, input_type: str, n_points: int) -> int:
        """Everything that can be refused before a file is read, upsampling's options first, then in stage order, then alignment's, then registration's -> the floor."""
        if self.point_sampling not in ("random", "fps"):
            raise ValueError(f'point_sampling must be "random" or "fps", got {self.point_sampling!r}')
        if self.point_sampling == "fps" and input_type == "mesh":
            raise ValueError('point_sampling="fps" applies to pc_normal and pc_xyz inputs: the points of a mesh input are already drawn from its surface')
        if not self.upsample_radius and self.upsample_points is not None:
            raise ValueError("upsample_points needs upsample_radius > 0")
        if not self.register_dist:
            for f in fields(self):
                if f.name.startswith("register_") and getattr(self, f.name) != f.default:
                    raise ValueError(f"{f.name} needs register_dist > 0")
        for f in fields(self):
            if f.name.startswith("coarse_") and getattr(self, f.name) != f.default:
                if input_type == "mesh":
                    raise ValueError(f"{f.name} applies to the scans of pc_normal and pc_xyz inputs, not to mesh inputs")
                if not self.coarse_radius:
                    raise ValueError(f"{f.name} needs coarse_radius > 0")
                if not self.register_dist:
                    raise ValueError(f"{f.name} needs register_dist > 0: the coarse pose is where a scan's registration starts")
        if self.coarse_radius:
            importlib.import_module(".pc_coarse", __package__).check_coarse_args(self.coarse_radius, self.coarse_points, self.coarse_iters, self.coarse_dist)
        for stage, module in sorted(self.on(), key=lambda sm: sm[0].switch != "upsample_radius") + self.pose() + self.scans():
            if input_type == "mesh":
                raise ValueError(f"{stage.switch} {stage.mesh}")
            stage.check(module, self, n_points)
        return self.floor(n_points)

    def parts(self, rows, uid: str, device, n_points: int = 4096):
        """The rows of one file -> [(rows, keys)] after every stage that is on and the alignment: the file itself, or its kept components."""
        parts = [(rows, {"uid": uid})]
        for stage, module in self.on() + self.pose():
            parts = stage.apply(module, self, parts, n_points, device)
        return parts
