"""Times of the coarse registration ops (`--coarse_radius`, meshanything_amd/pc_coarse.py) (GPU box).

    python scripts/time_pc_coarse.py [--reps 20] [--out profiles/time_pc_coarse.jsonl]

`ma_op_pc_spfh` over 2^20 samples of the test ellipsoid's surface (tests/pc_coarse_ref.py; the unit vector from the centre stands in for
the normal, the kernel does the same work for any), at the radius that gives about 100 neighbours a row, over `choose_cluster_grid`'s
grid; `ma_op_pc_smooth` on the same cloud, radius and grid, which does the same walk with more arithmetic per pair; `ma_op_pc_spfh_gather`
at 4 096 farthest-point queries; `ma_op_pc_desc_match` at 4 096 x 4 096; `ma_op_pc_pose_score` at 65 536 x 4 096.  Every figure is the
median over `reps` calls after warm-up, timed with HIP events on the current stream, workspace and outputs allocated once.  spfh, smooth
and gather are whole calls: build, pair bound and its read-back included, the same prologue in all three; the two long kernels apart come
from torch.profiler.  One JSON line per measurement.  DESIGN.md section 22 records the numbers.
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
from meshanything_amd import _lib, pc_coarse  # noqa: E402
from meshanything_amd.pc_cluster import choose_cluster_grid  # noqa: E402
from meshanything_amd.pc_fps import farthest_point_sample  # noqa: E402
import pc_coarse_ref as CR  # noqa: E402


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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def radius_for(xyz, neighbours, probe=0.05, sample=1 << 14, rows=1024):
    """The radius at which a row of xyz has about `neighbours` rows around it: the count at `probe` over a subsample, scaled as a surface's"""
    sub = xyz[:: max(xyz.shape[0] // sample, 1)].astype(np.float64)
    d2 = ((sub[:rows, None, :] - sub[None, :, :]) ** 2).sum(-1)
    mean = ((d2 <= probe * probe).sum(1) - 1).mean() * xyz.shape[0] / sub.shape[0]
    return float(probe * np.sqrt(neighbours / mean))


def kernel_us(fn, name, calls=3):
    """The mean device time of the kernel whose name contains `name` over `calls` calls of fn"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    hits = [e for e in prof.key_averages() if name in e.key]
    if not hits:
        raise RuntimeError(f"the profile holds no kernel named {name}")
    return sum(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total") for e in hits) / sum(e.count for e in hits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows_log2", type=int, default=20)
    ap.add_argument("--neighbours", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    sink = open(args.out, "w") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if sink:
            sink.write(json.dumps(line) + "\n")
            sink.flush()

    N = 1 << args.rows_log2
    xyz = CR.ellipsoid(N, 0)
    cloud_h = np.concatenate([xyz, xyz / np.linalg.norm(xyz, axis=1, keepdims=True)], 1).astype(np.float32)
    radius = radius_for(cloud_h[:, :3], args.neighbours)
    origin, cell, dims = choose_cluster_grid(cloud_h[:, :3], radius)
    cloud = torch.from_numpy(cloud_h).cuda()
    ga = ((C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist()))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = lib.ma_pc_spfh_workspace_bytes(N, *[int(d) for d in dims])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    hist = torch.empty((N, pc_coarse.COLS), dtype=torch.int32, device="cuda")
    bound = C.c_uint64(0)

    def spfh():
        _lib.check(lib.ma_op_pc_spfh(cloud.data_ptr(), N, 6, cloud.data_ptr() + 12, 6, radius, *ga, 0, hist.data_ptr(), C.byref(bound), None, ws.data_ptr(), need, stream))
    ms = median_ms(spfh, args.reps)
    used = hist[:, pc_coarse.DESC].to(torch.int64)
    common = {"rows": N, "radius": round(radius, 6), "cell": round(float(cell), 6), "dims": dims.tolist()}
    emit({"what": "spfh", **common, "ms": round(ms[0], 3), "min_ms": round(ms[1], 3), "max_ms": round(ms[2], 3), "kernel_us": round(kernel_us(spfh, "spfh_kernel"), 1),
          "pairs_used": int(used.sum()), "mean_neighbours": round(float(used.double().mean()), 2), "most_neighbours": int(used.max()), "pair_bound": bound.value})

    need_s = lib.ma_pc_smooth_workspace_bytes(N, *[int(d) for d in dims])
    ws_s = torch.empty(need_s, dtype=torch.uint8, device="cuda")
    moved = torch.empty((N, 3), dtype=torch.float64, device="cuda")

    def smooth():
        _lib.check(lib.ma_op_pc_smooth(cloud.data_ptr(), N, 6, radius, *ga, 6, 0, moved.data_ptr(), None, None, None, None, ws_s.data_ptr(), need_s, stream))
    ms = median_ms(smooth, args.reps)
    emit({"what": "smooth", **common, "ms": round(ms[0], 3), "min_ms": round(ms[1], 3), "max_ms": round(ms[2], 3), "kernel_us": round(kernel_us(smooth, "smooth_kernel"), 1)})
    del ws_s, moved

    K = pc_coarse.MAX_KEYPOINTS
    query = farthest_point_sample(cloud, K)[0]
    desc = torch.empty((K, pc_coarse.DESC), dtype=torch.int32, device="cuda")

    def gather():
        _lib.check(lib.ma_op_pc_spfh_gather(cloud.data_ptr(), N, 6, radius, *ga, 0, hist.data_ptr(), query.data_ptr(), K, desc.data_ptr(), None, ws.data_ptr(), need, stream))
    ms = median_ms(gather, args.reps)
    emit({"what": "spfh_gather", **common, "queries": K, "ms": round(ms[0], 3), "min_ms": round(ms[1], 3), "max_ms": round(ms[2], 3),
          "kernel_us": round(kernel_us(gather, "gather_kernel"), 1)})

    other = torch.roll(desc, 1, 0).contiguous()
    idx, dist = torch.empty(K, dtype=torch.int32, device="cuda"), torch.empty(K, dtype=torch.float32, device="cuda")

    def match():
        _lib.check(lib.ma_op_pc_desc_match(desc.data_ptr(), K, other.data_ptr(), K, idx.data_ptr(), dist.data_ptr(), stream))
    ms = median_ms(match, args.reps)
    emit({"what": "desc_match", "rows_a": K, "rows_b": K, "ms": round(ms[0], 3), "min_ms": round(ms[1], 3), "max_ms": round(ms[2], 3),
          "matched_its_copy": int((idx.cpu().numpy() == (np.arange(K) + 1) % K).sum())})

    H = pc_coarse.MAX_HYPOTHESES
    poses_h, P_h, Q_h, T = CR.score_case(4096, K)
    poses = torch.from_numpy(np.tile(poses_h, (H // 4096, 1))).cuda()
    P, Q = torch.from_numpy(P_h).cuda(), torch.from_numpy(Q_h).cuda()
    counts, best = torch.empty(H, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")

    def score():
        _lib.check(lib.ma_op_pc_pose_score(poses.data_ptr(), H, P.data_ptr(), Q.data_ptr(), K, T, counts.data_ptr(), best.data_ptr(), stream))
    ms = median_ms(score, args.reps)
    emit({"what": "pose_score", "hypotheses": H, "pairs": K, "ms": round(ms[0], 3), "min_ms": round(ms[1], 3), "max_ms": round(ms[2], 3),
          "tests_per_s": round(H * K / (ms[0] * 1e-3), 0), "best": int(best.cpu()[0]), "best_count": int(counts.max())})


if __name__ == "__main__":
    main()
