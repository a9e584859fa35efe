"""The order of the input side's steps (`meshanything_amd/cloud_prep.py`, run by `data.Dataset`): outliers, plane, cluster, smooth, upsample,
pick.  Every GPU function on that path is replaced in its module by a stand-in that records its call and returns rows of the right shape, so
the test needs no GPU and goes through `Dataset` alone: all 32 on/off combinations, both cloud types, both cluster modes, two devices."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from meshanything_amd import pc_cluster, pc_fps, pc_normals, pc_outliers, pc_plane, pc_smooth, pc_upsample
from meshanything_amd.data import Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS, TARGET, MIN_ROWS = 4096, 4 * 4096, 64
DROP_OUTLIERS, DROP_PLANE, DROP_CLUSTER = 10, 100, 50             # rows the stand-ins drop, from the end
STEPS = ("outlier_k", "plane_threshold", "cluster_radius", "smooth_radius", "upsample_radius")
ON = dict(outlier_k=16, plane_threshold=0.05, cluster_radius=0.1, smooth_radius=0.1, upsample_radius=0.1)


def origin(rows):
    """(file, row of the file) of the first row: which part of which file these rows are"""
    return int(rows[0, 1]), int(rows[0, 0])


@pytest.fixture
def calls(monkeypatch):
    log = []

    def filter_rows(xyz, k, std_ratio, n_points, uid, device="cuda"):
        log.append(("outliers", uid, origin(xyz), xyz.shape[0], n_points, device))
        return xyz[:-DROP_OUTLIERS]

    def remove_planes(xyz, threshold, iters, count, min_fraction, n_points, uid, device="cuda"):
        log.append(("plane", uid, origin(xyz), xyz.shape[0], n_points, device))
        return np.arange(xyz.shape[0] - DROP_PLANE)

    def split_rows(xyz, radius, min_points, mode, uid, device="cuda"):
        log.append(("cluster", uid, origin(xyz), xyz.shape[0], None, device))
        half = xyz.shape[0] // 2
        return [np.arange(half), np.arange(half, xyz.shape[0] - DROP_CLUSTER)][:2 if mode == "split" else 1]

    def smooth_rows(rows, radius, iters, uid, device="cuda"):
        log.append(("smooth", uid, origin(rows), rows.shape[0], None, device))
        return rows.copy()

    def upsample_rows(rows, radius, target, uid, device="cuda"):
        log.append(("upsample", uid, origin(rows), rows.shape[0], target, device))
        return rows if rows.shape[0] >= target else np.concatenate([rows, rows[np.arange(target - rows.shape[0]) % rows.shape[0]]])

    def fps_rows(xyz, n_points, device="cuda"):
        log.append(("pick", None, origin(xyz), xyz.shape[0], n_points, device))
        return np.arange(n_points) % xyz.shape[0]

    def xyz_to_pc_normal(xyz, n_points=4096, k=16, device="cuda", sampling="random"):
        log.append(("pick", None, origin(xyz), xyz.shape[0], n_points, device))
        return np.concatenate([xyz[np.arange(n_points) % xyz.shape[0], :3], np.tile(np.float32([0, 0, 1]), (n_points, 1))], axis=1)

    for module, fn in ((pc_outliers, filter_rows), (pc_plane, remove_planes), (pc_cluster, split_rows), (pc_smooth, smooth_rows),
                       (pc_upsample, upsample_rows), (pc_fps, fps_rows), (pc_normals, xyz_to_pc_normal)):
        monkeypatch.setattr(module, fn.__name__, fn)
    return log


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A 5 000-row file, and a 1 500-row file that only upsampling lets in: column 0 = the row, column 1 = the file, unit normals"""
    d = tmp_path_factory.mktemp("cloud_prep")
    paths = []
    for f, (name, n) in enumerate((("full", 5000), ("sparse", 1500))):
        rows = np.zeros((n, 6), np.float32)
        rows[:, 0], rows[:, 1], rows[:, 5] = np.arange(n), f, 1.0
        paths.append(str(d / f"{name}.npy"))
        np.save(paths[-1], rows)
    return paths


def expected(on, mode, device, rows_of):
    """Today's order, restated: per file the calls and the items' keys"""
    floor = MIN_ROWS if "upsample_radius" in on else N_POINTS
    log, items = [], []
    for f, (uid, n) in enumerate(rows_of):
        if "outlier_k" in on:
            log.append(("outliers", uid, (f, 0), n, floor, device))
            n -= DROP_OUTLIERS
        if "plane_threshold" in on:
            log.append(("plane", uid, (f, 0), n, floor, device))
            n -= DROP_PLANE
        parts = [(uid, 0, n, {"uid": uid})]
        if "cluster_radius" in on:
            log.append(("cluster", uid, (f, 0), n, None, device))
            half, rest = n // 2, n - DROP_CLUSTER - n // 2
            parts = [(uid, 0, half, {"uid": uid})] if mode == "largest" else [(f"{uid}_part{j}", j * half, m, {"uid": f"{uid}_part{j}", "group": uid, "part": j})
                                                                                  for j, m in enumerate((half, rest))]
        if "smooth_radius" in on:
            log += [("smooth", part, (f, start), m, None, device) for part, start, m, _ in parts]
        if "upsample_radius" in on:
            log += [("upsample", part, (f, start), m, TARGET, device) for part, start, m, _ in parts]
            parts = [(part, start, max(m, TARGET), keys) for part, start, m, keys in parts]
        log += [("pick", None, (f, start), m, N_POINTS, device) for _, start, m, _ in parts]
        items += [keys for _, _, _, keys in parts]
    return log, items


@pytest.mark.parametrize("mode", ["largest", "split"])
@pytest.mark.parametrize("kind", ["pc_normal", "pc_xyz"])
def test_the_steps_run_in_one_order_per_part_with_the_floor_and_the_device(kind, mode, calls, files, capsys):
    for flags, sample_device in itertools.product(itertools.product((False, True), repeat=len(STEPS)), (None, "cuda:3")):
        on = {s for s, flag in zip(STEPS, flags) if flag}
        rows_of = [("full", 5000), ("sparse", 1500)] if "upsample_radius" in on else [("full", 5000)]
        del calls[:]
        ds = Dataset(kind, files[:len(rows_of)], sample_device=sample_device, point_sampling="fps", cluster_mode=mode, **{s: ON[s] for s in on})
        log, items = expected(on, mode, sample_device or "cuda", rows_of)
        assert calls == log, (sorted(on), sample_device)
        assert [{k: v for k, v in d.items() if k != "pc_normal"} for d in ds.data] == items
        assert all(d["pc_normal"].shape == (N_POINTS, 6) for d in ds.data)
        assert [sorted(ds[i]) for i in range(len(ds))] == [sorted([*keys, "pc_normal"] + (["frame"] if "group" in keys else [])) for keys in items]
    assert capsys.readouterr().out.splitlines().count("dataset total data samples: 1") > 0


def test_the_uniform_draw_is_made_once_per_part_after_every_step(calls, files):
    """point_sampling "random" with pc_normal: the global RNG gives one np.random.choice per kept part, over the rows the last step left"""
    np.random.seed(5)
    ds = Dataset("pc_normal", files, cluster_mode="split", **ON)
    after = np.random.get_state()
    assert [c[0] for c in calls] == ["outliers", "plane", "cluster", "smooth", "smooth", "upsample", "upsample"] * 2
    np.random.seed(5)
    want = [np.random.choice(TARGET, N_POINTS, replace=False) for _ in ds.data]
    replay = np.random.get_state()
    assert len(ds) == 4 and np.array_equal(after[1], replay[1]) and after[2:] == replay[2:]
    for d, idx, up in zip(ds.data, want, [c for c in calls if c[0] == "upsample"]):
        start, m = up[2][1], up[3]
        assert np.array_equal(d["pc_normal"][:, 0], (start + np.where(idx < m, idx, (idx - m) % m)).astype(np.float32))


def test_a_dataset_with_every_step_off_imports_no_step_and_data_imports_no_torch(files):
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "import meshanything_amd.data as data\n"
            "assert 'torch' not in sys.modules, 'import meshanything_amd.data loads torch'\n"
            "assert len(data.Dataset('pc_normal', [sys.argv[2]])) == 1\n"
            "loaded = sorted(m for m in sys.modules if m.startswith('meshanything_amd.pc_'))\n"
            "assert not loaded and 'torch' not in sys.modules, loaded\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT, files[0]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
