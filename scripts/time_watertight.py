"""Stage times of the watertight remeshing step (`--mc`, meshanything_amd/watertight.py) at size 128 (GPU box).

    python scripts/time_watertight.py [--reps 20]

For three procedural meshes up to ~200k faces, the median over `reps` runs (after warm-up runs) of: the narrow-band distance
(ma_op_mesh_udf), the marching-cubes count (ma_op_marching_cubes without outputs: classify + two scans + the count read-back), the
marching-cubes count + emit (the same call with outputs; emit alone = the difference), each timed with HIP events on the current stream
(the count read-back synchronises the stream inside the call, so those two are host-synchronous anyway), and the host-side sampling
of 4096 points on the result (numpy, wall clock).  The GPU sampling stage (surface_sample.py) of the same 4096 points: its kernels
(frame + cdf + draw, on draws already on the device) with HIP events, and the whole call as `process_mesh_to_pc(..., device=...)` makes
it (frame, cdf, total read-back, draws taken and uploaded, sample, cloud and mesh read back) by wall clock; the cloud is checked
against the host one on the same seed.  One JSON line per mesh.  DESIGN.md section 8 records the numbers.
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
from meshanything_amd import _lib, surface_sample, watertight  # noqa: E402
from meshanything_amd.mesh_input import mesh_to_pc_normal  # noqa: E402
import watertight_ref as W  # noqa: E402


def meshes():
    yield "icosphere_20k", W.icosphere(subdiv=5)                   # 20480 faces
    yield "torus_131k", W.torus(n_major=512, n_minor=128)          # 131072 faces
    yield "sliver_soup_200k", W.sliver_soup(n=200000, seed=3)      # 200003 thin faces all over the grid


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
    ap.add_argument("--size", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    size, level = args.size, 2 / args.size
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, (v, f) in meshes():
        v32 = W.normalized32(v)
        dv = torch.from_numpy(v32).cuda()
        df = torch.from_numpy(f.astype(np.int32)).cuda()
        field = torch.empty((size,) * 3, dtype=torch.float32, device="cuda")
        nb = lib.ma_mesh_udf_workspace_bytes(f.shape[0])
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

        def udf():
            _lib.check(lib.ma_op_mesh_udf(dv.data_ptr(), v32.shape[0], df.data_ptr(), f.shape[0], size, field.data_ptr(), ws.data_ptr(), nb, stream))
        t_udf = median_ms(udf, args.reps)
        mnb = lib.ma_marching_cubes_workspace_bytes(size, size, size)
        mws = torch.empty(mnb, dtype=torch.uint8, device="cuda")
        counts = (C.c_int64 * 2)()

        def count():
            _lib.check(lib.ma_op_marching_cubes(field.data_ptr(), size, size, size, level, None, 0, None, 0, counts, mws.data_ptr(), mnb, stream))
        t_count = median_ms(count, args.reps)
        nv, nt = int(counts[0]), int(counts[1])
        mv = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        mt = torch.empty((nt, 3), dtype=torch.int32, device="cuda")

        def full():
            _lib.check(lib.ma_op_marching_cubes(field.data_ptr(), size, size, size, level, mv.data_ptr(), nv, mt.data_ptr(), nt, counts,
                                                mws.data_ptr(), mnb, stream))
        t_full = median_ms(full, args.reps)
        verts = mv.cpu().numpy().astype(np.float64) / size * 2 - 1          # sampled in this frame on the host (the area weights only scale)
        tris = mt.cpu().numpy().astype(np.int64)
        hs = []
        for r in range(max(3, args.reps // 4)):
            np.random.seed(r)
            t0 = time.perf_counter()
            mesh_to_pc_normal(verts, tris, 4096)
            hs.append((time.perf_counter() - t0) * 1e3)
        # GPU sampling of the same surface, in the input's frame as export_to_watertight gives it
        _, center, scale = watertight.normalize_vertices(v)
        cen = np.ascontiguousarray(center, dtype=np.float64)
        fverts = torch.empty((nv, 3), dtype=torch.float64, device="cuda")
        count = 4096
        draws = torch.from_numpy(np.random.default_rng(0).random(3 * count)).cuda()

        def kernels():
            _lib.check(lib.ma_op_mc_vertices_to_frame(mv.data_ptr(), nv, size, float(scale), cen.ctypes.data, fverts.data_ptr(), stream))
            normals, cum = surface_sample.surface_cdf(fverts, mt)
            surface_sample.sample_draws(fverts, mt, normals, cum, draws, count)
        t_kern = median_ms(kernels, args.reps)
        gs = []
        for r in range(max(3, args.reps // 4) + 2):
            np.random.seed(r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pc, _ = surface_sample.watertight_pc_normal(mv, mt, size, center, scale, count)
            gs.append((time.perf_counter() - t0) * 1e3)
        np.random.seed(r)
        host_pc = mesh_to_pc_normal(verts / scale + center, tris, count)
        same = bool(np.array_equal(pc.view(np.uint16), host_pc.view(np.uint16)))
        print(json.dumps({"mesh": name, "faces": int(f.shape[0]), "size": size, "mc_vertices": nv, "mc_triangles": nt,
                          "udf_ms": round(t_udf, 3), "mc_count_ms": round(t_count, 3), "mc_count_emit_ms": round(t_full, 3),
                          "mc_emit_ms": round(t_full - t_count, 3), "host_sample_ms": round(float(np.median(hs)), 3),
                          "gpu_sample_kernels_ms": round(t_kern, 3), "gpu_sample_call_ms": round(float(np.median(gs[2:])), 3),
                          "gpu_sample_matches_host": same}), flush=True)


if __name__ == "__main__":
    main()
