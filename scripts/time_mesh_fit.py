"""Time of one pairing plus sums of the mesh fit (`--fit_iters`, meshanything_amd/mesh_fit.py; ma_op_mesh_fit_pairs) (GPU box).

    python scripts/time_mesh_fit.py [--reps 20]

An 800-face torus (25 x 16 quads, major radius 0.6, minor 0.25 in cloud units) whose vertices were each moved by up to one lattice step
per axis, against P exact points of the torus with their normals, P = 4096 (the rows the CLI fits against) and 2^22 (the limit of the
Python API), at the defaults (dist 4 steps, no normal test).  Per shape the median over `reps` calls after warm-up of the whole call --
the two memsets, the pair kernel, the sum kernel and the read-back of the status word, which synchronises the stream inside the call --
timed with HIP events on the current stream, its minimum and maximum, the share of paired points, and the wall time of a whole
`fit_mesh` of 4 iterations (uploads, host solves and the two scorings included).  One JSON line per shape.  DESIGN.md section 23 records
the numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from meshanything_amd import mesh_fit  # noqa: E402
import watertight_ref as W  # noqa: E402

STEP = 2.0 / 128.0
R_MAJOR, R_MINOR = 0.6, 0.25


def torus_cloud(P, seed=0):
    rng = np.random.default_rng(seed)
    u, w = rng.uniform(0, 2 * np.pi, P), rng.uniform(0, 2 * np.pi, P)
    n = np.stack([np.cos(w) * np.cos(u), np.cos(w) * np.sin(u), np.sin(w)], -1)
    c = np.stack([R_MAJOR * np.cos(u), R_MAJOR * np.sin(u), np.zeros(P)], -1)
    return np.concatenate([c + R_MINOR * n, n], 1).astype(np.float32)


def times_ms(fn, reps, warm=3):
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, nargs="*", default=[4096, 1 << 22])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    v, f = W.torus(n_major=25, n_minor=16, R=R_MAJOR, r=R_MINOR)
    v = v + np.random.default_rng(1).uniform(-STEP, STEP, v.shape)
    mesh_units = (v / 2.0).astype(np.float32)
    x32 = torch.from_numpy(v.astype(np.float32)).cuda()
    f32 = torch.from_numpy(f.astype(np.int32)).cuda()
    for P in args.points:
        cloud = torus_cloud(P)
        c32 = torch.from_numpy(cloud).cuda()
        last = {}

        def call():
            last.update(mesh_fit._pairs(x32, f32, c32, 4 * STEP, 0.0))
        t = times_ms(call, args.reps)
        paired = int(last["sums"][:, 0].sum())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, rep = mesh_fit.fit_mesh(mesh_units, f, c32, 4)
        wall = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "points": P, "reps": args.reps, "pairs_call_ms_median": round(float(np.median(t)), 4),
                          "pairs_call_ms_min": round(min(t), 4), "pairs_call_ms_max": round(max(t), 4), "paired_share": round(paired / P, 4),
                          "point_face_tests_per_s": round(P * f.shape[0] / (float(np.median(t)) * 1e-3), 0),
                          "fit_mesh_4_iterations_wall_ms": round(wall, 2), "fit_iterations_run": len(rep["iterations"]), "fit_kept": rep["kept"],
                          "rms_before": rep["iterations"][0]["rms"], "rms_after": rep["rms_after"]}), flush=True)


if __name__ == "__main__":
    main()
