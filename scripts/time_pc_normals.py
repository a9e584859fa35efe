"""Stage times of the normal estimate for raw point clouds (`--input_type pc_xyz`, meshanything_amd/pc_normals.py) (GPU box).

    python scripts/time_pc_normals.py [--reps 20] [--sweep 2,4,8,16,32,64]

Q = 4096 queries against clouds of N = 4096, 65 536 and 2^20 points (a unit sphere), k = 16.  The median over `reps` runs (after
warm-up runs) with HIP events on the current stream of: ma_op_pc_knn with the automatic number of splits (search + merge) and with one
split (search alone, no merge), and ma_op_pc_normals (the eigen-solve).  The search and the merge of the automatic form apart come from
the kernels' own times (torch.profiler, the mean over the same runs; null when the profiler reports no kernels).  `xyz_to_pc_normal`
as a whole (the draw, upload, two searches, the eigen-solve, read-back and the host-side sign propagation) by wall clock.  For N = 4096
also the numpy brute force of tests/pc_normals_ref.py by wall clock, the only CPU figure there is.  --sweep: also ma_op_pc_knn at each of the given numbers of splits
("knn_splits_ms").  One JSON line per N, printed and appended to profiles/time_pc_normals.jsonl.  DESIGN.md section 11 records the numbers.
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
from meshanything_amd import _lib, pc_normals  # noqa: E402
import pc_normals_ref as R  # noqa: E402

Q, K = 4096, 16


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def kernel_ms(fn, reps):
    """mean device time per run of the search and the merge kernel, or (None, None)"""
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
    tot = {"knn_search_kernel": 0.0, "knn_merge_kernel": 0.0}
    for e in prof.key_averages():
        for name in tot:
            if name in e.key:
                tot[name] += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
    if not tot["knn_search_kernel"]:
        return None, None
    return round(tot["knn_search_kernel"] / reps, 4), round(tot["knn_merge_kernel"] / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", type=lambda t: [int(x) for x in t.split(",")], default=[])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for N in (4096, 65536, 1 << 20):
        xyz, _ = R.sphere(N, seed=0)
        ref = torch.from_numpy(xyz).cuda()
        qi = torch.from_numpy(np.random.default_rng(1).choice(N, Q, replace=False).astype(np.int32)).cuda()
        nbr = torch.empty((Q, K), dtype=torch.int32, device="cuda")
        d2 = torch.empty((Q, K), dtype=torch.float32, device="cuda")
        normals = torch.empty((Q, 3), dtype=torch.float64, device="cuda")
        eig = torch.empty((Q, 3), dtype=torch.float64, device="cuda")

        def search(splits):
            nb = lib.ma_pc_knn_workspace_bytes(N, Q, K, splits)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

            def run():
                _lib.check(lib.ma_op_pc_knn(ref.data_ptr(), N, 3, qi.data_ptr(), Q, K, splits, nbr.data_ptr(), d2.data_ptr(), ws.data_ptr(), nb, stream))
            return run, nb

        auto, auto_bytes = search(0)
        one, _ = search(1)
        t_auto, t_one = median_ms(auto, args.reps), median_ms(one, args.reps)
        k_search, k_merge = kernel_ms(auto, args.reps)

        def solve():
            _lib.check(lib.ma_op_pc_normals(ref.data_ptr(), N, 3, nbr.data_ptr(), Q, K, normals.data_ptr(), eig.data_ptr(), stream))
        t_solve = median_ms(solve, args.reps)
        whole = []
        for r in range(max(3, args.reps // 4) + 2):
            np.random.seed(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pc_normals.xyz_to_pc_normal(xyz, Q, K)
            whole.append((time.perf_counter() - t0) * 1e3)
        line = {"N": N, "Q": Q, "k": K, "auto_splits": int(auto_bytes // (2 * K * Q * 4)) if auto_bytes > 256 else 1,
                "knn_auto_ms": round(t_auto, 4), "knn_auto_search_kernel_ms": k_search, "knn_auto_merge_kernel_ms": k_merge,
                "knn_splits1_ms": round(t_one, 4), "normals_ms": round(t_solve, 4), "xyz_to_pc_normal_ms": round(float(np.median(whole[2:])), 2)}
        if args.sweep:
            line["knn_splits_ms"] = {str(sp): round(median_ms(search(sp)[0], args.reps), 4) for sp in args.sweep}
        if N == 4096:
            t0 = time.perf_counter()
            want, _ = R.knn_ref(xyz, qi.cpu().numpy(), K)
            line["numpy_brute_force_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["matches_numpy"] = bool(np.array_equal(want, nbr.cpu().numpy()))
        text = json.dumps(line)
        print(text, flush=True)
        with open(os.path.join(REPO, "profiles", "time_pc_normals.jsonl"), "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
