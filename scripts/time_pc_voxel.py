"""Times of voxel thinning (`--voxel_size`, meshanything_amd/pc_voxel.py) (GPU box).

    python scripts/time_pc_voxel.py [--reps 10] [--sizes 20,22,24,26] [--out profiles/time_pc_voxel.jsonl]

Two clouds in random row order, N = 2^20, 2^22, 2^24, 2^26 rows: the surface of the unit sphere and the uniformly filled unit box, each at
two leaves, chosen so that a dense cloud occupies about 2^16 and about 2^21 voxels (the line records the count).  Per cloud and leaf, with
the whole cloud on the device in chunks of 2^22 rows and the table allocated once: ma_op_pc_voxel_reset (not timed), then every chunk's
ma_op_pc_voxel_insert, then ma_op_pc_voxel_mark (which zeroes the mask, counts and copies the state back), each between HIP events on the
current stream, the median over `reps` runs after warm-up; every run starts from an empty table, since a second insert into a filled table
would time the plain-load filter alone.  Then the whole `voxel_keep` call (checks, minimum, uploads, table, mask back) by the host's
clock, the median of 3.  Once, at N = 2^20: the numpy restatement `pc_voxel_ref.voxel_ref` on the host, the only baseline there is,
whose mask must equal the kernel's.  One JSON line per measurement, printed and appended to --out.  DESIGN.md section 19 records the
numbers; this script asserts nothing but that equality.
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
from meshanything_amd import _lib, pc_voxel  # noqa: E402
import pc_voxel_ref as VR  # noqa: E402

LEAVES = {"sphere": (0.019, 0.0033), "box": (1 / 40, 1 / 128)}      # about 2^16 and 2^21 occupied voxels once the cloud is dense


def cloud_of(kind, N):
    g = np.random.default_rng(N)
    if kind == "box":
        return g.random((N, 3), dtype=np.float32)
    d = g.standard_normal((N, 3), dtype=np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[20, 22, 24, 26])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "time_pc_voxel.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")

    st = torch.cuda.current_stream()
    stream = C.c_void_p(st.cuda_stream)
    for log2 in args.sizes:
        N = 1 << log2
        for kind in ("sphere", "box"):
            xyz = cloud_of(kind, N)
            origin = xyz.min(axis=0)
            c_origin = (C.c_float * 3)(*origin.tolist())
            chunks = [torch.from_numpy(xyz[r:r + pc_voxel.MAX_CHUNK]).cuda() for r in range(0, N, pc_voxel.MAX_CHUNK)]
            capacity = pc_voxel.default_capacity(N)
            table = torch.empty(lib.ma_pc_voxel_table_bytes(capacity), dtype=torch.uint8, device="cuda")
            keep = torch.empty(N, dtype=torch.uint8, device="cuda")
            state = (C.c_uint32 * 4)()
            for leaf in LEAVES[kind]:
                ins, mk = [], []
                for rep in range(args.reps + 2):
                    assert lib.ma_op_pc_voxel_reset(table.data_ptr(), capacity, stream) == 0, lib.ma_last_error(None).decode()
                    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    a.record(st)
                    for j, chunk in enumerate(chunks):
                        assert lib.ma_op_pc_voxel_insert(chunk.data_ptr(), chunk.shape[0], 3, j * pc_voxel.MAX_CHUNK, c_origin, leaf, table.data_ptr(), capacity,
                                                         stream) == 0, lib.ma_last_error(None).decode()
                    b.record(st)
                    assert lib.ma_op_pc_voxel_mark(table.data_ptr(), capacity, keep.data_ptr(), N, state, stream) == 0, lib.ma_last_error(None).decode()
                    c.record(st)
                    c.synchronize()
                    if rep >= 2:
                        ins.append(a.elapsed_time(b))
                        mk.append(b.elapsed_time(c))
                assert state[1] == 0 and state[2] == 0, list(state)
                line = {"what": "insert_mark", "cloud": kind, "N": N, "leaf": round(leaf, 6), "voxels": int(state[3]), "capacity": capacity, "reps": args.reps,
                        "insert_ms": round(float(np.median(ins)), 4), "insert_min_ms": round(min(ins), 4), "insert_max_ms": round(max(ins), 4),
                        "mark_ms": round(float(np.median(mk)), 4), "rows_per_s": round(N / (float(np.median(ins)) * 1e-3), 1)}
                emit(line)
                walls = []
                for _ in range(4 if log2 < 26 else 2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got, voxels = pc_voxel.voxel_keep(xyz, leaf)
                    walls.append((time.perf_counter() - t0) * 1e3)
                assert voxels == int(state[3]) and got.tobytes() == keep.cpu().numpy().astype(bool).tobytes()
                emit({"what": "voxel_keep_wall", "cloud": kind, "N": N, "leaf": round(leaf, 6), "voxels": voxels, "ms": round(float(np.median(walls[1:])), 2),
                      "first_ms": round(walls[0], 2)})
                if log2 == 20:
                    t0 = time.perf_counter()
                    want, want_voxels, _ = VR.voxel_ref(xyz, leaf)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    assert want_voxels == voxels and want.tobytes() == got.tobytes()
                    emit({"what": "numpy_restatement", "cloud": kind, "N": N, "leaf": round(leaf, 6), "voxels": want_voxels, "ms": round(host_ms, 1)})
            del chunks, table, keep


if __name__ == "__main__":
    main()
