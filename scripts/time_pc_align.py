"""Times of the alignment step (`--align_iters`, meshanything_amd/pc_align.py) (GPU box).

    python scripts/time_pc_align.py [--reps 20] [--iters 4096]

One `box_extents` call (ma_op_pc_align_extents: init, extents, finish, best) on a turned box's surface of 2^20 and of 2^22 rows against
`iters` hypotheses: the median over `reps` calls after warm-up, timed with HIP events on the current stream; the same with the workspace
and outputs allocated once (the C call alone); and its share of the fp32 VALU peak, taking the rule's 21 lane-operations per (row,
hypothesis) pair (9 products, 6 sums, 6 min / max) as the work and 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 plain lane-operations
per second as the peak (the 157.3 TFLOPS of the data sheet count a packed FMA as four).  A whole `align_rows` of the 2^20-row cloud, by
wall clock (the draws, the uploads, 1 + rounds calls, the read-backs, the float64 turn of the rows on the host).  The restatement
(tests/pc_align_ref.py) on the CPU for 64 of the hypotheses, scaled to `iters`.  One JSON line per size.  DESIGN.md section 20 records
the numbers.
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
from meshanything_amd import _lib, pc_align  # noqa: E402
import pc_align_ref as R  # noqa: E402

PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
OPS_PER_PAIR = 21


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    H = args.iters
    rot = torch.from_numpy(pc_align.draw_rotations(H, 0).reshape(H, 9).astype(np.float32)).cuda()
    for log2 in (20, 22):
        N = 1 << log2
        xyz, normals = R.box_surface(N, 1)
        rows = np.concatenate([R.turn(xyz, R.R_25, (3.0, -2.0, 5.0)), normals @ R.R_25.T], 1).astype(np.float32)
        pts = torch.from_numpy(np.ascontiguousarray(rows[:, :3])).cuda()
        centre = (rows[:, :3].min(0) + rows[:, :3].max(0)) / np.float32(2)
        t_op = median_ms(lambda: pc_align.box_extents(pts, rot, centre), args.reps)
        nbytes = lib.ma_pc_align_workspace_bytes(N, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        vol, best = torch.empty(H, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
        c3, stream = (C.c_float * 3)(*centre.tolist()), C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            _lib.check(lib.ma_op_pc_align_extents(pts.data_ptr(), N, 3, c3, rot.data_ptr(), H, None, vol.data_ptr(), best.data_ptr(), ws.data_ptr(), nbytes, stream))
        t_call = median_ms(call, args.reps)
        line = {"rows": N, "hypotheses": H, "box_extents_ms": round(t_op, 3), "c_call_ms": round(t_call, 3),
                "valu_share": round(OPS_PER_PAIR * N * H / (t_call * 1e-3) / PEAK_LANE_OPS, 4)}
        if log2 == 20:
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pc_align.align_rows(rows, H, args.rounds, 0.02, "timed")
                walls.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            R.extents_ref(rows, rot[:64].cpu().numpy(), centre)
            line.update(align_rows_ms=round(float(np.median(walls)), 1), restatement_cpu_ms=round((time.perf_counter() - t0) * 1e3 * H / 64, 0))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
