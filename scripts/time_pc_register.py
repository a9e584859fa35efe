"""Times of the registration step (`--register_dist`, meshanything_amd/pc_register.py) (GPU box).

    python scripts/time_pc_register.py [--reps 20] [--out profiles/time_pc_register.jsonl]

One `ma_op_pc_register_step` (count, bound, read-back, search, moments, sum) of 2^20 source rows against 2^22 target rows, both samples of
the test solid's surface (tests/pc_register_ref.py), the source turned by 0.5 degrees and shifted by a third of a cell, over a grid of 128
cells along the solid's longest side, at D = 1 cell and D = 4 cells, plane and point metric: the median over `reps` calls after warm-up,
timed with HIP events on the current stream, the workspace and outputs allocated once.  The build (both clouds binned) the same way.  The
pairs found, the pair bound, and the keys a brute force would evaluate.  Then a whole `register_rows` of three scans of 2^20 rows each at
D = 0.01, by wall clock (uploads, three grids, the normals of pc_xyz scans if --xyz, every iteration's read-back of 32 doubles, the
float64 motion of the rows on the host).  One JSON line per measurement.  DESIGN.md section 21 records the numbers.
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
from meshanything_amd import _lib, pc_register  # noqa: E402
import pc_register_ref as R  # noqa: E402


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


def cloud(rows, seed):
    xyz, nrm = R.solid_surface(rows, seed)
    return np.concatenate([xyz, nrm], 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--target_log2", type=int, default=22)
    ap.add_argument("--source_log2", type=int, default=20)
    ap.add_argument("--scan_log2", type=int, default=20)
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

    N, M = 1 << args.target_log2, 1 << args.source_log2
    cell = np.float32(1.0 / 126)
    origin, dims = np.full(3, -float(cell), np.float32), np.array([128, 78, 78], np.int32)
    tgt_h, src_h = cloud(N, 1), cloud(M, 2)
    Rm, tm = R.rotation((1, 2, 3), 0.5), np.full(3, float(cell) / 3 / np.sqrt(3))
    src_h[:, :3] = ((src_h[:, :3].astype(np.float64) - tm) @ Rm).astype(np.float32)
    tgt, src = torch.from_numpy(tgt_h).cuda(), torch.from_numpy(src_h).cuda()
    need = lib.ma_pc_register_workspace_bytes(N, M, *[int(d) for d in dims])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ga = ((C.c_float * 3)(*origin.tolist()), float(cell), (C.c_int32 * 3)(*dims.tolist()))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pose = (C.c_float * 12)(*np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).tolist())
    centre = (C.c_float * 3)(*src_h[:, :3].mean(0).tolist())
    sums, idx = torch.empty(32, dtype=torch.float64, device="cuda"), torch.empty(M, dtype=torch.int32, device="cuda")

    def build():
        _lib.check(lib.ma_op_pc_register_build(tgt.data_ptr(), N, 6, src.data_ptr(), M, 6, *ga, ws.data_ptr(), need, stream))
    emit({"what": "build", "target_rows": N, "source_rows": M, "dims": dims.tolist(), "ms": round(median_ms(build, args.reps), 3)})
    for cells in (1, 4):
        dist = float(cell) * cells
        for metric in ("plane", "point"):
            bound = C.c_uint64(0)

            def step():
                _lib.check(lib.ma_op_pc_register_step(tgt.data_ptr(), N, 6, src.data_ptr(), M, 6, *ga, pose, centre, dist, tgt.data_ptr() + 12 if metric == "plane" else None, 6,
                                                      0, idx.data_ptr(), None, C.byref(bound), sums.data_ptr(), ws.data_ptr(), need, stream))
            ms = median_ms(step, args.reps)
            s = sums.cpu().numpy()
            emit({"what": "step", "metric": metric, "dist_in_cells": cells, "dist": round(dist, 6), "target_rows": N, "source_rows": M, "ms": round(ms, 3),
                  "pairs": int(s[0]), "skipped": int(s[30]), "rms": float(np.sqrt((s[2] if metric == "plane" else s[1]) / max(s[0], 1))), "pair_bound": bound.value,
                  "brute_force_keys": N * M})
    del tgt, src, ws
    rows = 1 << args.scan_log2
    scans = []
    poses = (pc_register.IDENTITY, (R.rotation((1, 2, 3), 0.3), np.array([0.002, -0.001, 0.002])), (R.rotation((-2, 1, 1), 0.3), np.array([-0.001, 0.002, 0.002])))
    for j, (cut, (Rj, tj)) in enumerate(zip(R.CUTS, poses)):
        c = cloud(2 * rows, 10 + j)
        c = c[cut(c[:, :3])][:rows]
        assert c.shape[0] == rows
        scans.append(np.concatenate([(c[:, :3].astype(np.float64) - tj) @ Rj, c[:, 3:].astype(np.float64) @ Rj], 1).astype(np.float32))
    for kind, normal_k in (("pc_normal", None), ("pc_xyz", 16)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, got = pc_register.register_rows(scans if normal_k is None else [s[:, :3] for s in scans], 0.01, normal_k=normal_k, uid="timed")
        wall = (time.perf_counter() - t0) * 1e3
        errs = [R.pose_errors(g, p, s[:, :3]) for g, p, s in zip(got[1:], poses[1:], scans[1:])]
        emit({"what": "register_rows", "kind": kind, "scans": 3, "rows_per_scan": rows, "dist": 0.01, "wall_ms": round(wall, 1),
              "rotation_error_rad": [float(e[0]) for e in errs], "displacement": [float(e[1]) for e in errs]})


if __name__ == "__main__":
    main()
