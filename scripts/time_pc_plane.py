"""Times of dominant-plane removal (`--plane_threshold`, meshanything_amd/pc_plane.py) (GPU box).

    python scripts/time_pc_plane.py [--reps 20] [--sizes 16,20,22] [--hyps 256,1024,4096] [--out profiles/time_pc_plane.jsonl]

A table with a sphere on it (`cloud_of`: 40 % of the rows uniform in [-1, 1]^2 within 0.2 t of the plane z = 0, the others on a sphere of
radius 0.4 that touches it; tilted, shifted, shuffled; t = 0.02), N = 2^16, 2^20, 2^22 rows.  Per N and H = 256, 1 024, 4 096 hypotheses from
`draw_triples`: ma_op_pc_plane_score (its three launches) with HIP events on the current stream, buffers allocated once, the median over
`reps` runs after warm-up, and N * H point-plane tests per second.  Per N: ma_op_pc_plane_apply with mask, count and moments, the same
way; and the whole `remove_planes` call (upload, 1 024 draws, score, two applies, the refit, the rows back) by the host's clock, the
median of 5.  Once: the numpy restatement `pc_plane_ref.score_ref` on the host at N = 2^16, H = 256, the only baseline there is, whose
counts must equal the kernel's.  One JSON line per measurement, printed and appended to --out.  DESIGN.md section 16 records the numbers;
this script asserts nothing but that equality.
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
from meshanything_amd import _lib, pc_plane  # noqa: E402
import pc_plane_ref as PR  # noqa: E402

T = 0.02


def cloud_of(N):
    g = np.random.default_rng(N)
    n_table = N * 2 // 5
    table = np.concatenate([g.uniform(-1, 1, (n_table, 2)), g.uniform(-0.2 * T, 0.2 * T, (n_table, 1))], 1)
    d = g.normal(size=(N - n_table, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = np.concatenate([table, d * 0.4 + [0.0, 0.0, 0.4]], 0)
    c, s = np.cos(0.3), np.sin(0.3)
    xyz = xyz @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]).T + [3.0, -2.0, 5.0]
    return xyz[g.permutation(N)].astype(np.float32)


def median_ms(fn, reps):
    st = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4), round(float(np.max(times)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[16, 20, 22])
    ap.add_argument("--hyps", type=lambda t: [int(x) for x in t.split(",")], default=[256, 1024, 4096])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "time_pc_plane.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for log2 in args.sizes:
        N = 1 << log2
        xyz = cloud_of(N)
        ref = torch.from_numpy(xyz).cuda()
        plane = None
        for H in args.hyps:
            tri = torch.from_numpy(pc_plane.draw_triples(N, H, 0)).cuda()
            nb = lib.ma_pc_plane_workspace_bytes(N, H)
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            planes = torch.empty((H, 6), dtype=torch.float32, device="cuda")
            counts, best = torch.empty(H, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
            call = lambda: lib.ma_op_pc_plane_score(ref.data_ptr(), N, 3, tri.data_ptr(), H, T, planes.data_ptr(), counts.data_ptr(), best.data_ptr(),  # noqa: E731
                                                    ws.data_ptr(), nb, stream)
            assert call() == 0, lib.ma_last_error(None).decode()
            med, lo, hi = median_ms(call, args.reps)
            b = int(best.item())
            plane = planes[b].cpu().numpy()
            emit({"what": "score", "N": N, "H": H, "ms": med, "min_ms": lo, "max_ms": hi, "reps": args.reps, "pairs_per_s": round(N * H / (med * 1e-3), 1),
                  "best": b, "best_count": int(counts[b].item())})
            if (log2, H) == (16, 256):
                t0 = time.perf_counter()
                _, want, want_best = PR.score_ref(xyz, tri.cpu().numpy(), T)
                host_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(want, counts.cpu().numpy()) and want_best == b
                emit({"what": "numpy_restatement", "N": N, "H": H, "ms": round(host_ms, 1), "pairs_per_s": round(N * H / (host_ms * 1e-3), 1), "threads": torch.get_num_threads()})
        nb = lib.ma_pc_plane_workspace_bytes(N, 1)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        mask, count, moments = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(10, dtype=torch.float64, device="cuda")
        host_plane = (C.c_float * 6)(*plane.tolist())
        call = lambda: lib.ma_op_pc_plane_apply(ref.data_ptr(), N, 3, host_plane, T, mask.data_ptr(), count.data_ptr(), moments.data_ptr(), ws.data_ptr(), nb, stream)  # noqa: E731
        assert call() == 0, lib.ma_last_error(None).decode()
        med, lo, hi = median_ms(call, args.reps)
        emit({"what": "apply_with_moments", "N": N, "ms": med, "min_ms": lo, "max_ms": hi, "reps": args.reps, "count": int(count.item())})
        walls = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = pc_plane.remove_planes(xyz, T, 1024, 1, 0.2, 1, f"n2^{log2}")
            walls.append((time.perf_counter() - t0) * 1e3)
        emit({"what": "remove_planes_wall", "N": N, "iters": 1024, "ms": round(float(np.median(walls[1:])), 2), "first_ms": round(walls[0], 2), "kept": int(kept.shape[0])})
        del ref, mask


if __name__ == "__main__":
    main()
