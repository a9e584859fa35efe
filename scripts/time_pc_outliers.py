"""Times of the all-points neighbour search behind statistical outlier removal (`--outlier_k`, meshanything_amd/pc_outliers.py) (GPU box).

    python scripts/time_pc_outliers.py [--reps 20] [--sizes 14,16,18,20,22]

A unit sphere of N = 2^14 .. 2^22 points (seeded), clean and with 1 % of its rows replaced by strays uniform in [-2, 2]^3, k = 16.  Per
cloud, with HIP events on the current stream, the median over `reps` runs after warm-up of: ma_op_pc_knn_grid writing mean_dist only
(grid build + search, the filter's path) over `choose_grid`'s grid and over grids of 16, 32, 64 and 128 cells along the longest axis;
and, for N <= 2^20, the brute force ma_op_pc_knn with every point a query (it writes the two lists).  The runs of one cloud alternate
in the same process.  A call that takes longer than 100 ms is timed 5 times, one longer than 2 s once ("reps" says how often).  The
build kernels and the search kernel of the automatic grid apart come from the kernels' own times (torch.profiler, the mean over 5 runs;
null when the profiler reports no kernels).  `mean_agree`: every grid gave the same mean_dist bits.  One JSON line per cloud, printed
and appended to profiles/time_pc_outliers.jsonl.  DESIGN.md section 14 records the numbers, the rule of `choose_grid` and the crossover
of form 0 taken from them; this script asserts neither.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from meshanything_amd import _lib, pc_outliers  # noqa: E402
import pc_normals_ref as R  # noqa: E402

K = 16
ALONG = (16, 32, 64, 128)
BUILD_KERNELS = ("count_kernel", "tile_sum_kernel", "scan_kernel", "scatter_kernel")


def cloud_of(N, stray_pct):
    n_out = N * stray_pct // 100
    g = np.random.default_rng(1)
    xyz = np.concatenate([R.sphere(N - n_out, seed=0)[0], g.uniform(-2, 2, (n_out, 3)).astype(np.float32)], 0)
    return xyz[g.permutation(N)].copy()


def once_ms(fn):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """name -> (median ms, runs): two warm-up runs each, then rounds in which every function still owed a run takes one"""
    owed, times = {}, {n: [] for n in fns}
    for n, fn in fns.items():
        fn()
        first = once_ms(fn)
        owed[n] = 1 if first > 2000 else 5 if first > 100 else reps
        if owed[n] == 1:
            times[n].append(first)
    for r in range(reps):
        for n, fn in fns.items():
            if r < owed[n] and not (owed[n] == 1):
                times[n].append(once_ms(fn))
    return {n: (round(float(np.median(t)), 4), len(t)) for n, t in times.items()}


def kernel_ms(fn, reps=5):
    """mean device time per run of the build kernels together and of the search kernel, or (None, None)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
    except RuntimeError as e:                                        # a torch build without device tracing
        print(f"# no kernel times: {e}", file=sys.stderr)
        return None, None
    build = search = 0.0
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
        if "pcg" in e.key and "search_kernel" in e.key:
            search += t
        elif "pcg" in e.key and any(b in e.key for b in BUILD_KERNELS):
            build += t
    if not search:
        return None, None
    return round(build / reps, 4), round(search / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[14, 16, 18, 20, 22])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for log2 in args.sizes:
        N = 1 << log2
        for stray_pct in (0, 1):
            xyz = cloud_of(N, stray_pct)
            ref = torch.from_numpy(xyz).cuda()
            mean = torch.empty(N, dtype=torch.float64, device="cuda")
            grids = {"auto": pc_outliers.choose_grid(xyz, K)}
            grids.update({f"along{a}": pc_outliers.choose_grid(xyz, K, along=a) for a in ALONG})
            keep, fns, means = [], {}, {}

            def grid_call(origin, cell, dims):
                nb = lib.ma_pc_knn_grid_workspace_bytes(N, K, int(dims[0]), int(dims[1]), int(dims[2]))
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                o, d = (C.c_float * 3)(*origin.tolist()), (C.c_int32 * 3)(*dims.tolist())
                keep.append(ws)
                return lambda: _lib.check(lib.ma_op_pc_knn_grid(ref.data_ptr(), N, 3, K, o, float(cell), d, None, None, mean.data_ptr(), ws.data_ptr(), nb, stream))

            for name, g in grids.items():
                fns[name] = grid_call(*g)
            if N <= 1 << 20:
                nb = lib.ma_pc_knn_workspace_bytes(N, N, K, 0)
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                idx = torch.empty((N, K), dtype=torch.int32, device="cuda")
                d2 = torch.empty((N, K), dtype=torch.float32, device="cuda")
                fns["brute"] = lambda: _lib.check(lib.ma_op_pc_knn(ref.data_ptr(), N, 3, None, N, K, 0, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nb, stream))
            got = alternate(fns, args.reps)
            for name in grids:
                fns[name]()
                means[name] = mean.cpu().numpy().tobytes()
            build, search = kernel_ms(fns["auto"])
            line = {"N": N, "stray_pct": stray_pct, "k": K, "auto_dims": grids["auto"][2].tolist(),
                    "grid_ms": {n: got[n][0] for n in grids}, "brute_ms": got["brute"][0] if "brute" in got else None,
                    "auto_build_kernels_ms": build, "auto_search_kernel_ms": search, "reps": {n: v[1] for n, v in got.items()},
                    "dims": {n: g[2].tolist() for n, g in grids.items()}, "mean_agree": len(set(means.values())) == 1}
            text = json.dumps(line)
            print(text, flush=True)
            with open(os.path.join(REPO, "profiles", "time_pc_outliers.jsonl"), "a") as f:
                f.write(text + "\n")
            del keep, fns, ref, mean


if __name__ == "__main__":
    main()
