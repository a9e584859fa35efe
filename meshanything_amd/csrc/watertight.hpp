// Watertight remeshing of a mesh input: export_to_watertight of mesh_to_pc.py:13-40 (mesh2sdf distances on a size^3 grid, then
// scikit-image marching cubes of |sdf| at level 2 / size).  Only |sdf| is ever used, so the grid holds an UNSIGNED distance, and only
// where it can reach the surface: a narrow band of 2 cells around every triangle's bounding box (the band argument: DESIGN.md
// section 8).  Then marching cubes with the generated 256-case table of mc_table.hpp.  No float atomics, no order dependence: the
// distance is reduced with an integer atomicMin on its bit pattern (distances are >= 0), the surface is written in cell-linear order
// after two exclusive scans, so both outputs are bitwise reproducible.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mc_table.hpp"

namespace ma {
namespace wt {

// ---- exclusive scan (int64, in place): one 1024-element tile per 256-thread block, tile sums scanned recursively ------------
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__global__ __launch_bounds__(SCAN_THREADS) void scan_tile_kernel(int64_t* __restrict__ data, int64_t n, int64_t* __restrict__ tile_sums) {
    __shared__ long long wave_sum[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    long long x[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { x[i] = base + i < n ? (long long)data[base + i] : 0; s += x[i]; }
    long long inc = s;                                           // inclusive scan of the per-thread sums inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    long long run = inc - s, tot = 0;
#pragma unroll
    for (int i = 0; i < SCAN_THREADS / 64; ++i) { if (i < w) run += wave_sum[i]; tot += wave_sum[i]; }
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { if (base + i < n) data[base + i] = run; run += x[i]; }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_add_kernel(int64_t* __restrict__ data, int64_t n, const int64_t* __restrict__ tile_offsets) {
    const int64_t add = tile_offsets[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const int64_t idx = (int64_t)blockIdx.x * SCAN_TILE + i * SCAN_THREADS + threadIdx.x;
        if (idx < n) data[idx] += add;
    }
}

inline int64_t scan_tiles(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

// int64 elements of workspace scan_exclusive(n) needs
inline int64_t scan_ws_elems(int64_t n) {
    const int64_t nb = scan_tiles(n);
    return nb + (nb > 1 ? scan_ws_elems(nb) : 0);
}

inline hipError_t scan_exclusive(int64_t* data, int64_t n, int64_t* ws, hipStream_t s) {
    const int64_t nb = scan_tiles(n);
    hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, data, n, ws);
    if (nb > 1) {
        hipError_t r = scan_exclusive(ws, nb, ws + nb, s);
        if (r != hipSuccess) return r;
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, data, n, ws);
    }
    return hipGetLastError();
}

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// ---- narrow-band unsigned distance ------------------------------------------------------------------------------------------
constexpr int UDF_BAND = 2;          // cells the index-space bounding box of a triangle is widened by
constexpr int UDF_CHUNK = 256;       // voxels per work item: one block of 256 threads
constexpr int UDF_GRID = 8192;       // blocks of the grid-stride band kernel

struct F3 { float x, y, z; };
__device__ inline F3 sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline F3 cross(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline F3 axpy(float t, F3 d, F3 a) { return {a.x + t * d.x, a.y + t * d.y, a.z + t * d.z}; }

// |q| for q = the point of segment a .. a + e closest to the origin (a relative to the query point, e the edge vector)
__device__ inline float seg_dist(F3 a, F3 e) {
    const float l2 = dot(e, e);
    float t = l2 > 0.f ? -dot(a, e) / l2 : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    const F3 q = axpy(t, e, a);
    return sqrtf(dot(q, q));
}

// Distance from p to triangle A, B, C: the least of its three edge distances, and the plane distance when p projects inside the
// triangle (every edge sees p on its inner side).  The distance is 1-Lipschitz in the vertices, so the arithmetic is kept stable as
// the area goes to 0: edge vectors come from the vertex coordinates (not from the p-relative ones), the normal from the two shorter
// edges (the pair at the largest angle), and a triangle whose inradius |n| / perimeter is at most `flat` -- a collinear or
// near-collinear face, whose plane fp32 cannot resolve -- is its three edges only; that answer is off by at most the inradius,
// i.e. by at most `flat`.  No Voronoi-region products (their cancellation picks a random region on such faces).
__device__ inline float tri_dist(F3 A, F3 B, F3 C, F3 p, float flat) {
    const F3 e0 = sub(B, A), e1 = sub(C, B), e2 = sub(A, C);
    const F3 a = sub(A, p), b = sub(B, p), c = sub(C, p);
    const float dseg = fminf(seg_dist(a, e0), fminf(seg_dist(b, e1), seg_dist(c, e2)));
    const float l0 = dot(e0, e0), l1 = dot(e1, e1), l2 = dot(e2, e2);
    const F3 n = (l0 >= l1 && l0 >= l2) ? cross(e1, e2) : (l1 >= l2 ? cross(e2, e0) : cross(e0, e1));   // = e0 x e1 in exact arithmetic
    const float n2 = dot(n, n);
    const float fp = flat * (sqrtf(l0) + sqrtf(l1) + sqrtf(l2));
    if (!(n2 > fp * fp)) return dseg;
    // edge i from vertex v_i sees p on its inner side when (e_i x (p - v_i)) . n >= 0, and p - v_i = -(v_i - p)
    const float s0 = dot(cross(a, e0), n), s1 = dot(cross(b, e1), n), s2 = dot(cross(c, e2), n);
    if (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f) return fminf(dseg, fabsf(dot(a, n)) / sqrtf(n2));
    return dseg;
}

// inradius below which a face counts as its edges (tri_dist): 1/128 of a grid cell
constexpr float UDF_FLAT_CELLS = 1.0f / 128.0f;

// per triangle: its index-space bounding box widened by UDF_BAND cells and clamped to the grid (boxes[6t .. 6t+5] = lo xyz, hi xyz,
// inclusive) and its number of UDF_CHUNK-voxel chunks (chunks[t]; chunks[nf] = 0, so that the exclusive scan ends in the total).
// A face that names a vertex outside [0, nv) gets no chunks (the host refuses such input; this keeps the kernel in bounds anyway).
__global__ __launch_bounds__(256) void udf_boxes_kernel(const float* __restrict__ verts, int nv, const int* __restrict__ faces, int nf, int size,
                                                        int* __restrict__ boxes, int64_t* __restrict__ chunks) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > nf) return;
    if (t == nf) { chunks[nf] = 0; return; }
    const int64_t t3 = 3 * (int64_t)t, t6 = 6 * (int64_t)t;
    const int i0 = faces[t3], i1 = faces[t3 + 1], i2 = faces[t3 + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        for (int a = 0; a < 3; ++a) { boxes[t6 + a] = 0; boxes[t6 + 3 + a] = -1; }
        chunks[t] = 0;
        return;
    }
    const float half = 0.5f * (float)size;
    int64_t count = 1;
    for (int a = 0; a < 3; ++a) {
        // grid point i sits at -1 + 2 i / size, so x maps to index (x + 1) * size / 2
        const float g0 = (verts[3 * (int64_t)i0 + a] + 1.0f) * half, g1 = (verts[3 * (int64_t)i1 + a] + 1.0f) * half,
                    g2 = (verts[3 * (int64_t)i2 + a] + 1.0f) * half;
        const float lim = (float)(size + 4);
        const float mn = fminf(fmaxf(fminf(g0, fminf(g1, g2)), -4.f), lim), mx = fminf(fmaxf(fmaxf(g0, fmaxf(g1, g2)), -4.f), lim);
        const int lo = max(0, (int)floorf(mn) - UDF_BAND), hi = min(size - 1, (int)ceilf(mx) + UDF_BAND);
        boxes[t6 + a] = lo;
        boxes[t6 + 3 + a] = hi;
        count *= hi >= lo ? (int64_t)(hi - lo + 1) : 0;
    }
    chunks[t] = (count + UDF_CHUNK - 1) / UDF_CHUNK;
}

__global__ __launch_bounds__(256) void fill_inf_kernel(float* __restrict__ field, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) field[i] = INFINITY;
}

// one block per (triangle, chunk) work item, grid-stride over the flattened list: offs = exclusive scan of the chunk counts
// (offs[nf] = total).  Every voxel of the widened box gets min(current, fp32 distance) by an integer atomicMin on the bits.
__global__ __launch_bounds__(UDF_CHUNK) void udf_band_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int nf, int size,
                                                             const int* __restrict__ boxes, const int64_t* __restrict__ offs, float* __restrict__ field) {
    const int64_t total = offs[nf];
    const float step = 2.0f / (float)size;
    const float flat = step * UDF_FLAT_CELLS;
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = nf - 1;                                   // the last triangle whose first chunk is <= c
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= c) lo = mid; else hi = mid - 1;
        }
        const int t = lo;
        const int64_t t6 = 6 * (int64_t)t;
        const int bx = boxes[t6], by = boxes[t6 + 1], bz = boxes[t6 + 2];
        const int64_t nx = boxes[t6 + 3] - bx + 1, ny = boxes[t6 + 4] - by + 1, nz = boxes[t6 + 5] - bz + 1;
        const int64_t local = (c - offs[t]) * UDF_CHUNK + threadIdx.x;
        if (local >= nx * ny * nz) continue;
        const int64_t k = local % nz, r = local / nz, j = r % ny, i = r / ny;
        const int gi = bx + (int)i, gj = by + (int)j, gk = bz + (int)k;
        const F3 p = {(float)gi * step - 1.0f, (float)gj * step - 1.0f, (float)gk * step - 1.0f};
        const int64_t i0 = faces[3 * (int64_t)t], i1 = faces[3 * (int64_t)t + 1], i2 = faces[3 * (int64_t)t + 2];
        const F3 a = {verts[3 * i0], verts[3 * i0 + 1], verts[3 * i0 + 2]};
        const F3 b = {verts[3 * i1], verts[3 * i1 + 1], verts[3 * i1 + 2]};
        const F3 cc = {verts[3 * i2], verts[3 * i2 + 1], verts[3 * i2 + 2]};
        const float d = tri_dist(a, b, cc, p, flat);
        const int64_t idx = ((int64_t)gi * size + gj) * size + gk;
        atomicMin(reinterpret_cast<unsigned int*>(field) + idx, __float_as_uint(d));
    }
}

struct UdfWs { int* boxes; int64_t* chunks; int64_t* scan; };

inline size_t udf_ws_bytes(int nf, UdfWs* ws = nullptr, void* base = nullptr) {
    const size_t b_boxes = align256((size_t)nf * 6 * sizeof(int));
    const size_t b_chunks = align256(((size_t)nf + 1) * sizeof(int64_t));
    const size_t b_scan = align256((size_t)scan_ws_elems((int64_t)nf + 1) * sizeof(int64_t));
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->boxes = reinterpret_cast<int*>(p);
        ws->chunks = reinterpret_cast<int64_t*>(p + b_boxes);
        ws->scan = reinterpret_cast<int64_t*>(p + b_boxes + b_chunks);
    }
    return b_boxes + b_chunks + b_scan;
}

inline hipError_t launch_mesh_udf(const float* verts, int nv, const int* faces, int nf, int size, float* field, void* workspace, hipStream_t s) {
    UdfWs ws;
    udf_ws_bytes(nf, &ws, workspace);
    const int64_t ncell = (int64_t)size * size * size;
    hipLaunchKernelGGL(fill_inf_kernel, dim3((unsigned)std::min<int64_t>((ncell + 255) / 256, 4096)), dim3(256), 0, s, field, ncell);
    hipLaunchKernelGGL(udf_boxes_kernel, dim3((unsigned)(((int64_t)nf + 1 + 255) / 256)), dim3(256), 0, s, verts, nv, faces, nf, size, ws.boxes, ws.chunks);
    hipError_t r = scan_exclusive(ws.chunks, (int64_t)nf + 1, ws.scan, s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(udf_band_kernel, dim3(UDF_GRID), dim3(UDF_CHUNK), 0, s, verts, faces, nf, size, ws.boxes, ws.chunks, field);
    return hipGetLastError();
}

// ---- marching cubes ---------------------------------------------------------------------------------------------------------
// pass 1, one thread per grid point p = (i * ny + j) * nz + k (index nv = nx*ny*nz writes the zero that ends both scans):
// emask[p] = its crossing +x/+y/+z edges (bits 0..2), vcount[p] = their number; for a cell origin, cube[p] = the cube index
// (bit c set when corner c is >= level) and tcount[p] = the table's triangle count, 0 for the other points.
__global__ __launch_bounds__(256) void mc_classify_kernel(const float* __restrict__ field, int nx, int ny, int nz, float level,
                                                          int64_t* __restrict__ vcount, int64_t* __restrict__ tcount,
                                                          uint8_t* __restrict__ cube, uint8_t* __restrict__ emask) {
    const int64_t np = (int64_t)nx * ny * nz;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > np) return;
    if (p == np) { vcount[np] = 0; tcount[np] = 0; return; }
    const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / ((int64_t)nz * ny));
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const bool up0 = field[p] >= level;
    int m = 0;
    if (i + 1 < nx && (field[p + sx] >= level) != up0) m |= 1;
    if (j + 1 < ny && (field[p + sy] >= level) != up0) m |= 2;
    if (k + 1 < nz && (field[p + 1] >= level) != up0) m |= 4;
    emask[p] = (uint8_t)m;
    vcount[p] = __popc(m);
    int ci = 0;
    if (i + 1 < nx && j + 1 < ny && k + 1 < nz) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (field[p + (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1)] >= level) ci |= 1 << c;
    }
    cube[p] = (uint8_t)ci;
    tcount[p] = MC_NTRIS[ci];
}

// pass 2: vertices in index space (float32, x y z = array axes 0 1 2), one per crossing edge at its owner's scanned offset in
// x, y, z order, placed by linear interpolation t = (level - a) / (b - a) (correctly rounded division: the host restatement
// reproduces it bit for bit); triangles as int32 vertex ids at the cell's scanned offset, in table order.  Writes past
// max_verts / max_tris are dropped (the caller has already been told the counts).
__global__ __launch_bounds__(256) void mc_emit_kernel(const float* __restrict__ field, int nx, int ny, int nz, float level,
                                                      const int64_t* __restrict__ voff, const int64_t* __restrict__ toff,
                                                      const uint8_t* __restrict__ cube, const uint8_t* __restrict__ emask,
                                                      float* __restrict__ verts, int64_t max_verts, int* __restrict__ tris, int64_t max_tris) {
    const int64_t np = (int64_t)nx * ny * nz;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int k = (int)(p % nz), j = (int)((p / nz) % ny), i = (int)(p / ((int64_t)nz * ny));
    const int64_t sx = (int64_t)ny * nz, sy = nz;
    const int m = emask[p];
    if (m) {
        int64_t id = voff[p];
        const float a = field[p];
        for (int axis = 0; axis < 3; ++axis) {
            if (!((m >> axis) & 1)) continue;
            const float b = field[p + (axis == 0 ? sx : axis == 1 ? sy : 1)];
            float t = !isfinite(a) ? 1.f : !isfinite(b) ? 0.f : __fdiv_rn(level - a, b - a);
            float pos[3] = {(float)i, (float)j, (float)k};
            pos[axis] += t;
            if (id < max_verts) { verts[3 * id] = pos[0]; verts[3 * id + 1] = pos[1]; verts[3 * id + 2] = pos[2]; }
            ++id;
        }
    }
    const int ci = cube[p];
    const int nt = MC_NTRIS[ci];
    const int64_t t0 = toff[p];
    for (int t = 0; t < nt; ++t) {
        if (t0 + t >= max_tris) break;
        for (int c = 0; c < 3; ++c) {
            const int e = MC_TRIS[ci][3 * t + c];
            const int axis = MC_EDGES[e][3];
            const int64_t owner = p + MC_EDGES[e][0] * sx + MC_EDGES[e][1] * sy + MC_EDGES[e][2];
            tris[3 * (t0 + t) + c] = (int)(voff[owner] + __popc(emask[owner] & ((1 << axis) - 1)));
        }
    }
}

struct McWs { int64_t* vcount; int64_t* tcount; int64_t* scan; uint8_t* cube; uint8_t* emask; };

inline size_t mc_ws_bytes(int64_t np, McWs* ws = nullptr, void* base = nullptr) {
    const size_t b_cnt = align256(((size_t)np + 1) * sizeof(int64_t));
    const size_t b_scan = align256((size_t)scan_ws_elems(np + 1) * sizeof(int64_t));
    const size_t b_u8 = align256((size_t)np);
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->vcount = reinterpret_cast<int64_t*>(p);
        ws->tcount = reinterpret_cast<int64_t*>(p + b_cnt);
        ws->scan = reinterpret_cast<int64_t*>(p + 2 * b_cnt);
        ws->cube = reinterpret_cast<uint8_t*>(p + 2 * b_cnt + b_scan);
        ws->emask = reinterpret_cast<uint8_t*>(p + 2 * b_cnt + b_scan + b_u8);
    }
    return 2 * b_cnt + b_scan + 2 * b_u8;
}

// classify + both scans; afterwards vcount[np] / tcount[np] hold the vertex / triangle totals (device)
inline hipError_t launch_mc_count(const float* field, int nx, int ny, int nz, float level, const McWs& ws, hipStream_t s) {
    const int64_t np = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)((np + 1 + 255) / 256)), dim3(256), 0, s, field, nx, ny, nz, level, ws.vcount, ws.tcount, ws.cube, ws.emask);
    hipError_t r = scan_exclusive(ws.vcount, np + 1, ws.scan, s);
    if (r != hipSuccess) return r;
    return scan_exclusive(ws.tcount, np + 1, ws.scan, s);
}

inline hipError_t launch_mc_emit(const float* field, int nx, int ny, int nz, float level, const McWs& ws, float* verts, int64_t max_verts,
                                 int* tris, int64_t max_tris, hipStream_t s) {
    const int64_t np = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, field, nx, ny, nz, level, ws.vcount, ws.tcount, ws.cube,
                       ws.emask, verts, max_verts, tris, max_tris);
    return hipGetLastError();
}

}  // namespace wt
}  // namespace ma
