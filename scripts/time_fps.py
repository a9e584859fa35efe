"""Times of farthest-point sampling (`--point_sampling fps`, meshanything_amd/pc_fps.py) (GPU box).

    python scripts/time_fps.py [--reps 20] [--also 1024,8192]

n = 4 096 picks from N = 4 096, 16 384, 65 536, 2^20 and 2^22 points (uniform in a cube, seeded; --also: further N).  Per N the
median over `reps` runs (after warm-up runs) with HIP events on the current stream of ma_op_pc_fps in the one-workgroup form (where N
allows it), the many-workgroup form and the automatic choice, each with the automatic start (two more small launches); whether the
forms returned the same bits; the wall clock of `Dataset("pc_normal", [file], point_sampling="fps")` on an (N, 6) float32 .npy (load,
checks, upload, sampling, gather: median of 3 after one warm-up); and for N = 65 536 the numpy restatement of tests/pc_fps_ref.py by
wall clock, the only CPU figure there is.  One JSON line per N, printed and appended to profiles/time_fps.jsonl.  DESIGN.md section 13
records the numbers and the threshold of the automatic choice taken from them.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from meshanything_amd import _lib, pc_fps  # noqa: E402
from meshanything_amd.data import Dataset  # noqa: E402
import pc_fps_ref as R  # noqa: E402

PICKS = 4096


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
    ap.add_argument("--also", type=lambda t: [int(x) for x in t.split(",")], default=[])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for N in sorted(set([4096, 16384, 65536, 1 << 20, 1 << 22] + args.also)):
        n = min(PICKS, N)
        cloud = R.uniform_cloud(N, 6, seed=0)
        ref = torch.from_numpy(cloud).cuda()
        nb = lib.ma_pc_fps_workspace_bytes(N, n, 0)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        line = {"N": N, "n": n, "workspace_bytes": int(nb)}
        results = {}
        for form, tag in ((1, "one_workgroup"), (2, "many_workgroups"), (0, "auto")):
            if form == 1 and N > pc_fps.ONE_MAX_POINTS:
                line[tag + "_ms"] = None
                continue
            idx = torch.empty(n, dtype=torch.int32, device="cuda")
            d2 = torch.empty(n, dtype=torch.float32, device="cuda")

            def run():
                _lib.check(lib.ma_op_pc_fps(ref.data_ptr(), N, 6, n, -1, form, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nb, stream))
            line[tag + "_ms"] = round(median_ms(run, args.reps), 4)
            results[tag] = (idx.cpu().numpy(), d2.cpu().numpy())
        base = results["many_workgroups"]
        line["forms_agree"] = all(np.array_equal(base[0], r[0]) and base[1].tobytes() == r[1].tobytes() for r in results.values())
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "cloud.npy")
            np.save(path, cloud)
            wall = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ds = Dataset("pc_normal", [path], n_points=n, point_sampling="fps")
                wall.append((time.perf_counter() - t0) * 1e3)
            line["dataset_fps_wall_ms"] = round(float(np.median(wall[1:])), 2)
            line["dataset_rows_match"] = bool(np.array_equal(ds.data[0]["pc_normal"], cloud[base[0]]))
        if N == 65536:
            t0 = time.perf_counter()
            want_idx, want_d2, _ = R.fps_ref(cloud, n)
            line["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["matches_numpy"] = bool(np.array_equal(want_idx, base[0]) and want_d2.tobytes() == base[1].tobytes())
        text = json.dumps(line)
        print(text, flush=True)
        with open(os.path.join(REPO, "profiles", "time_fps.jsonl"), "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
