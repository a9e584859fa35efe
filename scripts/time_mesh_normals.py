"""Times of the normal agreement between candidate meshes and their cloud (`--normal_weight`, `--orient cloud`,
meshanything_amd/csrc/mesh_normals.hpp) next to the score op's, on the same inputs in the same run (GPU box).

    python scripts/time_mesh_normals.py [--reps 20] [--out profiles/time_mesh_normals.jsonl]

64 and 8 candidates of 800 random faces against clouds of 4 096 points (one cloud per 4 candidates).  The median over `reps` runs (after
warm-up runs) with HIP events on the current stream of ma_op_mesh_normals and of ma_op_score_meshes as a whole, and every kernel's own
time (torch.profiler, the mean over the same runs; null when the profiler reports no kernels).  The yardstick of the search kernel is
the score op's mesh-to-cloud launch, which does the same search without the index: "search_over_mesh_to_cloud" is the ratio of the two
kernel times.  One JSON line per batch size, printed and appended to --out.  DESIGN.md section 12 records the numbers.
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
from meshanything_amd import _lib  # noqa: E402
import mesh_score_ref as S  # noqa: E402

F, P, N_PER_CLOUD = 800, 4096, 4
KERNELS = ("face_normals_kernel", "reduce_normals_kernel", "cloud_to_mesh_kernel", "mesh_to_cloud_kernel", "reduce_kernel")


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
    """kernel name -> mean device time per run in ms, or None for each"""
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
    tot = {k: 0.0 for k in KERNELS}
    for e in prof.key_averages():
        for name in KERNELS:
            if ("::" + name) in e.key or e.key.startswith(name):
                tot[name] += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
    return {k: (round(v / reps, 4) if v else None) for k, v in tot.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "time_mesh_normals.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for B in (64, 8):
        coords = torch.from_numpy(np.stack([S.soup(F, 1000 + b) for b in range(B)])).cuda()
        cloud = torch.from_numpy(np.stack([S.points(P, 2000 + g, 6) for g in range(B // N_PER_CLOUD)])).cuda()
        nb_n, nb_s = lib.ma_mesh_normals_workspace_bytes(B, F), lib.ma_score_meshes_workspace_bytes(B, F, P)
        ws_n, ws_s = torch.empty(nb_n, dtype=torch.uint8, device="cuda"), torch.empty(nb_s, dtype=torch.uint8, device="cuda")
        agree = torch.empty((B, F), dtype=torch.float32, device="cuda")
        nscores = torch.empty((B, 4), dtype=torch.float32, device="cuda")
        scores = torch.empty((B, 4), dtype=torch.float32, device="cuda")

        def normals():
            _lib.check(lib.ma_op_mesh_normals(coords.data_ptr(), B, F, cloud.data_ptr(), 6, P, N_PER_CLOUD, 2.0, agree.data_ptr(), nscores.data_ptr(),
                                              ws_n.data_ptr(), nb_n, stream))

        def score():
            _lib.check(lib.ma_op_score_meshes(coords.data_ptr(), B, F, cloud.data_ptr(), 6, P, N_PER_CLOUD, 2.0, scores.data_ptr(), ws_s.data_ptr(), nb_s,
                                              stream))

        def both():
            normals()
            score()

        # alternate the two ops so that neither has the quieter half of the run
        t_n1, t_s1 = median_ms(normals, args.reps), median_ms(score, args.reps)
        t_s2, t_n2 = median_ms(score, args.reps), median_ms(normals, args.reps)
        k = kernel_ms(both, args.reps)
        ratio = round(k["face_normals_kernel"] / k["mesh_to_cloud_kernel"], 3) if k["face_normals_kernel"] and k["mesh_to_cloud_kernel"] else None
        line = {"B": B, "F": F, "P": P, "n_per_cloud": N_PER_CLOUD, "reps": args.reps,
                "mesh_normals_ms": [round(t_n1, 4), round(t_n2, 4)], "score_meshes_ms": [round(t_s1, 4), round(t_s2, 4)],
                "kernel_ms": k, "search_over_mesh_to_cloud": ratio,
                "nc_mean": round(float(nscores[:, 0].mean()), 6), "finite": bool(torch.isfinite(nscores).all() and torch.isfinite(scores).all())}
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
