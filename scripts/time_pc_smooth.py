"""Times of input-cloud smoothing (`--smooth_radius`, meshanything_amd/pc_smooth.py) (GPU box).

    python scripts/time_pc_smooth.py [--reps 20] [--sizes 12,16,20]

Unit spheres of N = 2^12, 2^16 and 2^20 points (seeded) with Gaussian jitter of radius / 20, at the radius that gives about 30
neighbours, sqrt(120 / N).  Per cloud, over `choose_cluster_grid`'s grid: ma_op_pc_smooth (all four outputs) with HIP events on the
current stream, the median over `reps` runs after warm-up; next to it ma_op_pc_cluster on the same cloud, grid and radius, the same
walk and the same key evaluations, so that the ratio is the price of the float64 moments and the Jacobi solve; the smooth kernel and
the hook kernel apart from the kernels' own times (torch.profiler, the mean over 5 runs; null when the profiler reports no kernels); and
the whole `smooth_rows` call, one pass, by the host's clock.  One JSON line per cloud, printed and appended to
profiles/time_pc_smooth.jsonl.  DESIGN.md section 17 records the numbers; this script asserts nothing.
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
from meshanything_amd import _lib, pc_cluster, pc_smooth  # noqa: E402
import pc_normals_ref as R  # noqa: E402

OUT = os.path.join(REPO, "profiles", "time_pc_smooth.jsonl")
KERNELS = {"smooth_kernel": "smooth_kernel", "hook_kernel": "hook_kernel"}


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
    return round(float(np.median([once_ms(fn) for _ in range(reps)])), 4)


def kernel_ms(fn, reps=5):
    """kernel -> mean device time per run, or every kernel None"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    except RuntimeError as e:                                        # a torch build without device tracing
        print(f"# no kernel times: {e}", file=sys.stderr)
        return {k: None for k in KERNELS}
    got = {k: 0.0 for k in KERNELS}
    for e in prof.key_averages():
        for k, name in KERNELS.items():
            if name in e.key:
                got[k] += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
    return {k: round(t / reps, 4) if t else None for k, t in got.items()}


def calls(lib, ref, N, radius, grid):
    origin, cell, dims = grid
    o, d = (C.c_float * 3)(*origin.tolist()), (C.c_int32 * 3)(*dims.tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bound = C.c_uint64(0)
    ns = lib.ma_pc_smooth_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
    nc = lib.ma_pc_cluster_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
    ws = torch.empty(max(ns, nc), dtype=torch.uint8, device="cuda")
    f = [torch.empty((N, 3), dtype=torch.float64, device="cuda") for _ in range(3)]
    count = torch.empty(N, dtype=torch.int32, device="cuda")
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    smooth = lambda: lib.ma_op_pc_smooth(ref.data_ptr(), N, 3, float(radius), o, float(cell), d, pc_smooth.DEFAULT_MIN_COUNT, 0, f[0].data_ptr(),   # noqa: E731
                                         f[1].data_ptr(), f[2].data_ptr(), count.data_ptr(), C.byref(bound), ws.data_ptr(), ns, stream)
    cluster = lambda: lib.ma_op_pc_cluster(ref.data_ptr(), N, 3, float(radius), o, float(cell), d, 0, labels.data_ptr(), None, C.byref(bound),      # noqa: E731
                                           ws.data_ptr(), nc, stream)
    return smooth, cluster, count, bound


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[12, 16, 20])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for log2 in args.sizes:
        N = 1 << log2
        radius = float(np.sqrt(120.0 / N))
        xyz = (R.sphere(N, seed=0)[0] + np.random.default_rng(1).normal(size=(N, 3)) * (radius / 20)).astype(np.float32)
        ref = torch.from_numpy(xyz).cuda()
        grid = pc_cluster.choose_cluster_grid(xyz, radius)
        smooth, cluster, count, bound = calls(lib, ref, N, radius, grid)
        assert smooth() == 0 and cluster() == 0, lib.ma_last_error(None).decode()
        smooth_ms, cluster_ms = median_ms(smooth, args.reps), median_ms(cluster, args.reps)
        kernels = dict(kernel_ms(smooth), hook_kernel=kernel_ms(cluster)["hook_kernel"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pc_smooth.smooth_rows(xyz, radius, 1, f"sphere{log2}")
        rows_ms = round((time.perf_counter() - t0) * 1e3, 2)
        emit({"N": N, "radius": radius, "dims": grid[2].tolist(), "pairs_bound": int(bound.value), "mean_count": round(float(count.float().mean()), 2),
              "smooth_ms": smooth_ms, "cluster_ms": cluster_ms, "ratio": round(smooth_ms / cluster_ms, 3), "kernel_ms": kernels, "smooth_rows_ms": rows_ms,
              "reps": args.reps})
        del ref


if __name__ == "__main__":
    main()
