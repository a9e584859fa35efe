"""Times of Euclidean clustering (`--cluster_radius`, meshanything_amd/pc_cluster.py) (GPU box).

    python scripts/time_pc_cluster.py [--reps 20] [--sizes 14,16,18,20,22]
    python scripts/time_pc_cluster.py --cap [--cap_log2 22]

Sphere and torus clouds of N = 2^14 .. 2^22 points (seeded), clean and with 1 % of their rows replaced by strays uniform in [-2, 2]^3;
radii of 2, 4 and 8 times the median nearest-neighbour spacing (from `grid_knn`).  Per cloud and radius, over `choose_cluster_grid`'s
grid: ma_op_pc_cluster with HIP events on the current stream, the median over `reps` runs after warm-up (a call that takes longer than
100 ms is timed 5 times, one longer than 2 s once); its build, bound, hook and flatten kernels apart from the kernels' own times
(torch.profiler, the mean over 5 runs; null when the profiler reports no kernels); the whole `split_rows` call by the host's clock;
next to them `grid_knn(k = 16, want = "mean")` on the same cloud and grid, the same walk and the only yardstick in this tree; and, where
scipy imports and N <= 2^18, cKDTree.query_pairs + connected_components on the host, whose component count must agree.  One JSON line
per cloud and radius, printed and appended to profiles/time_pc_cluster.jsonl.

--cap: the time of one call whose pair bound sits just under a cap, for MA_PC_CLUSTER_MAX_PAIRS: a uniform cloud of 2^cap_log2 points in
the unit cube; per cap = 2^30, 2^31, ... 2^36 the radius is bisected on the bound the call reads back (max_pairs = 1: the call stops
after the bound), then that call is timed once with the cap lifted.  It stops at the first cap whose call takes more than 2 s, so the
machine is never given the longest job first.  DESIGN.md section 15 records the numbers; this script asserts nothing.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from meshanything_amd import _lib, pc_cluster, pc_outliers  # noqa: E402
import pc_normals_ref as R  # noqa: E402

RADII = (2, 4, 8)
STAGES = {"build": ("count_kernel", "tile_sum_kernel", "scan_kernel", "scatter_kernel"), "bound": ("init_kernel", "bound_kernel"), "hook": ("hook_kernel",),
          "flatten": ("flatten_kernel",)}
OUT = os.path.join(REPO, "profiles", "time_pc_cluster.jsonl")


def cloud_of(shape, N, stray_pct):
    n_out = N * stray_pct // 100
    g = np.random.default_rng(1)
    xyz = np.concatenate([R.CLOUDS[shape](N - n_out, seed=0)[0], g.uniform(-2, 2, (n_out, 3)).astype(np.float32)], 0)
    return xyz[g.permutation(N)].copy()


def once_ms(fn):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    fn()
    first = once_ms(fn)
    n = 1 if first > 2000 else 5 if first > 100 else reps
    times = [first] if n == 1 else [once_ms(fn) for _ in range(n)]
    return round(float(np.median(times)), 4), len(times)


def stage_ms(fn, reps=5):
    """stage -> mean device time per run of its kernels, or every stage None"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    except RuntimeError as e:                                        # a torch build without device tracing
        print(f"# no kernel times: {e}", file=sys.stderr)
        return {s: None for s in STAGES}
    got = {s: 0.0 for s in STAGES}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
        for s, names in STAGES.items():
            if any(n in e.key for n in names) and ("pcg" in e.key or "pcc" in e.key):
                got[s] += t
    if not got["hook"]:
        return {s: None for s in STAGES}
    return {s: round(t / reps, 4) for s, t in got.items()}


def cluster_call(lib, ref, N, radius, grid, cap, labels, bound):
    origin, cell, dims = grid
    nb = lib.ma_pc_cluster_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    o, d = (C.c_float * 3)(*origin.tolist()), (C.c_int32 * 3)(*dims.tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: lib.ma_op_pc_cluster(ref.data_ptr(), N, 3, float(radius), o, float(cell), d, cap, labels.data_ptr(), None, C.byref(bound), ws.data_ptr(), nb, stream)


def host_components(xyz, radius):
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
    except ImportError:
        return None, None
    t0 = time.perf_counter()
    pairs = cKDTree(xyz.astype(np.float64)).query_pairs(float(np.float32(radius)), output_type="ndarray")
    n = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(xyz),) * 2), directed=False)[0]
    return round((time.perf_counter() - t0) * 1e3, 2), int(n)


def sweep(args, lib):
    for log2 in args.sizes:
        N = 1 << log2
        for shape in ("sphere", "torus"):
            for stray_pct in (0, 1):
                xyz = cloud_of(shape, N, stray_pct)
                ref = torch.from_numpy(xyz).cuda()
                spacing = float(torch.sqrt(pc_outliers.grid_knn(ref, 3, want="d2")["d2"][:, 1]).median())
                labels = torch.empty(N, dtype=torch.int32, device="cuda")
                for mult in RADII:
                    radius = mult * spacing
                    grid = pc_cluster.choose_cluster_grid(xyz, radius)
                    bound = C.c_uint64(0)
                    call = cluster_call(lib, ref, N, radius, grid, 0, labels, bound)
                    assert call() == 0, lib.ma_last_error(None).decode()
                    total = median_ms(call, args.reps)
                    comps = int(torch.unique(labels).shape[0])
                    knn = median_ms(lambda: pc_outliers.grid_knn(ref, 16, grid, want="mean"), args.reps)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pc_cluster.split_rows(xyz, radius, 1, "largest", f"{shape}{log2}")
                    split_ms = round((time.perf_counter() - t0) * 1e3, 2)
                    host_ms, host_n = host_components(xyz, radius) if N <= 1 << 18 else (None, None)
                    line = {"shape": shape, "N": N, "stray_pct": stray_pct, "spacing": spacing, "radius_in_spacings": mult, "radius": radius,
                            "dims": grid[2].tolist(), "pairs_bound": int(bound.value), "components": comps, "cluster_ms": total[0], "reps": total[1],
                            "stage_ms": stage_ms(call), "grid_knn16_mean_ms": knn[0], "split_rows_ms": split_ms, "host_ckdtree_ms": host_ms,
                            "host_components": host_n}
                    emit(line)
                del ref, labels


def cap_run(args, lib):
    N = 1 << args.cap_log2
    xyz = np.random.default_rng(0).uniform(0, 1, (N, 3)).astype(np.float32)
    ref = torch.from_numpy(xyz).cuda()
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    bound = C.c_uint64(0)

    def bound_at(radius):
        cluster_call(lib, ref, N, radius, pc_cluster.choose_cluster_grid(xyz, radius), 1, labels, bound)()   # stops after the bound
        return int(bound.value)

    for log2 in range(30, 37):
        lo, hi = 1e-4, 0.5
        for _ in range(30):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if bound_at(mid) <= 1 << log2 else (lo, mid)
        got = bound_at(lo)
        call = cluster_call(lib, ref, N, lo, pc_cluster.choose_cluster_grid(xyz, lo), 1 << log2, labels, bound)
        ms = once_ms(lambda: call())
        emit({"cap_log2": log2, "N": N, "radius": lo, "pairs_bound": got, "cluster_ms": round(ms, 2), "components": int(torch.unique(labels).shape[0])})
        if ms > 2000:
            break


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[14, 16, 18, 20, 22])
    ap.add_argument("--cap", action="store_true")
    ap.add_argument("--cap_log2", type=int, default=22)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    (cap_run if args.cap else sweep)(args, lib)


if __name__ == "__main__":
    main()
