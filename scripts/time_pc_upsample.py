"""Times of input-cloud upsampling (`--upsample_radius`, meshanything_amd/pc_upsample.py) (GPU box).

    python scripts/time_pc_upsample.py [--reps 20] [--sizes 1024,2048,65536]

Fibonacci unit spheres of N points at a radius of two point spacings, 2 * sqrt(4 pi / N), upsampled to max(16384, 4 N) rows.  Per
cloud, over `choose_cluster_grid`'s grid, with the normals of one `smooth_points` fit and at the m the ladder picks: a count-only
ma_op_pc_upsample call and a full call (count, scan, emit) with HIP events on the current stream, the median over `reps` runs after
warm-up (both calls include the grid build, the pair bound and their host read-backs); the count and the emit kernel apart from the
kernels' own times (torch.profiler, the mean over 5 runs; null when the profiler reports no kernels); the whole `upsample_rows` call by
the host's clock; and, for N <= 4096, the wall time of the numpy restatement on the same inputs, for scale.  One JSON line per cloud,
printed and appended to profiles/time_pc_upsample.jsonl.  DESIGN.md section 18 records the numbers; this script asserts nothing.
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
from meshanything_amd import _lib, pc_cluster, pc_smooth, pc_upsample  # noqa: E402
import pc_upsample_ref as UR  # noqa: E402

OUT = os.path.join(REPO, "profiles", "time_pc_upsample.jsonl")
KERNELS = {"count_kernel": "lattice_kernel<false>", "emit_kernel": "lattice_kernel<true>"}
REF_MAX_N = 4096


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


def calls(lib, ref, normals, active, N, radius, m, grid, capacity):
    origin, cell, dims = grid
    o, d = (C.c_float * 3)(*origin.tolist()), (C.c_int32 * 3)(*dims.tolist())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total, bound = C.c_uint64(0), C.c_uint64(0)
    nbytes = lib.ma_pc_upsample_workspace_bytes(N, int(dims[0]), int(dims[1]), int(dims[2]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = torch.empty(N, dtype=torch.int32, device="cuda")
    xyz = torch.empty((capacity, 3), dtype=torch.float32, device="cuda")
    seed = torch.empty(capacity, dtype=torch.int32, device="cuda")

    def call(full):
        return lib.ma_op_pc_upsample(ref.data_ptr(), N, 3, normals.data_ptr(), active.data_ptr(), m, radius / m, o, float(cell), d, 0, counts.data_ptr(),
                                     xyz.data_ptr() if full else None, seed.data_ptr() if full else None, capacity, C.byref(total), C.byref(bound),
                                     ws.data_ptr(), nbytes, stream)
    return (lambda: call(False)), (lambda: call(True)), total, bound


def emit(line):
    text = json.dumps(line)
    print(text, flush=True)
    with open(OUT, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[1024, 2048, 65536])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for N in args.sizes:
        radius = float(2.0 * np.sqrt(4.0 * np.pi / N))
        target = max(pc_upsample.DEFAULT_TARGET, 4 * N)
        xyz = UR.fibonacci(N)[0]
        ref = torch.from_numpy(xyz).cuda()
        grid = pc_cluster.choose_cluster_grid(xyz, radius)
        fit = pc_smooth.smooth_points(ref, radius, pc_smooth.DEFAULT_MIN_COUNT, grid, want=("normals", "eigvals", "count"))
        plane = ~pc_smooth.stayed(fit["count"].cpu().numpy(), fit["eigvals"].cpu().numpy())
        active = torch.from_numpy(plane.astype(np.uint8)).cuda()
        m, kept = pc_upsample.choose_m(lambda m: pc_upsample.upsample_points(ref, fit["normals"], radius, m, active, grid, count_only=True)["total"],
                                       N, target, radius)
        count, full, total, bound = calls(lib, ref, fit["normals"], active, N, radius, m, grid, kept)
        assert count() == 0 and full() == 0 and total.value == kept, lib.ma_last_error(None).decode()
        count_ms, full_ms = median_ms(count, args.reps), median_ms(full, args.reps)
        kernels = kernel_ms(full)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pc_upsample.upsample_rows(xyz, radius, target, f"sphere{N}")
        rows_ms = round((time.perf_counter() - t0) * 1e3, 2)
        numpy_ms = None
        if N <= REF_MAX_N:
            t0 = time.perf_counter()
            want = UR.upsample_ref(xyz, fit["normals"].cpu().numpy(), radius, m, plane)
            numpy_ms = round((time.perf_counter() - t0) * 1e3, 1)
            assert want["xyz"].shape[0] == kept
        emit({"N": N, "radius": radius, "target": target, "m": m, "kept": int(kept), "dims": grid[2].tolist(), "pairs_bound": int(bound.value),
              "count_call_ms": count_ms, "full_call_ms": full_ms, "kernel_ms": kernels, "upsample_rows_ms": rows_ms, "numpy_restatement_ms": numpy_ms,
              "reps": args.reps})
        del ref


if __name__ == "__main__":
    main()
