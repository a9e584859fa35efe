// Area-weighted surface sampling of a triangle mesh: mesh_to_pc_normal of mesh_to_pc.py:42-57 (`mesh.sample(n, return_index=True)`
// + `face_normals[face_idx]`), i.e. what meshanything_amd/mesh_input.py computes in numpy, on the device.  The uniform draws are
// inputs (the caller takes them from the global numpy RNG), so for the same draws the (count, 6) float16 cloud is the host's bit for
// bit: every operation below is float64 in numpy's order, with no contraction into FMAs (`#pragma clang fp contract(off)` in every
// function), IEEE division and square root, and one correctly rounded float64 -> float16 conversion at the end.
//
// The one step that is not numpy's is the cumulative sum of the areas: np.cumsum is sequential, this is a parallel tile scan, so a
// partial sum may differ in its last bits and a draw within that rounding of a face boundary may land on the neighbouring face
// (DESIGN.md section 8).  A second, exact pass (a running maximum that skips zero-area faces) keeps the result non-decreasing and
// gives a zero-area face the same value as the face before it, so such a face is never drawn, as on the host.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "watertight.hpp"

namespace ma {
namespace ss {

// float64 -> float16 bits, round to nearest even, in one step (numpy's astype(float16)); converting through float32 would round
// twice: 1 + 2^-11 + 2^-40 is 1.000977 directly and 1.0 through float32.  NaN keeps its top payload bits, as numpy's does.
__host__ __device__ inline uint16_t f64_to_f16_rne(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, sizeof b);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const uint64_t mant = b & ((uint64_t(1) << 52) - 1);
    const int ef = (int)((b >> 52) & 0x7ff);
    if (ef == 0x7ff) {
        if (!mant) return sign | 0x7c00u;
        const uint16_t h = (uint16_t)(0x7c00u + (mant >> 42));
        return sign | (h == 0x7c00u ? 0x7c01u : h);
    }
    const int e = ef - 1023;                                     // |x| in [2^e, 2^(e+1))
    if (e > 15) return sign | 0x7c00u;                           // >= 2^16: infinity
    if (e < -25) return sign;                                    // < 2^-25: below half the least subnormal, rounds to 0
    uint64_t m, base;
    int shift;
    if (e >= -14) { m = mant; shift = 42; base = (uint64_t)(e + 15) << 10; }                 // normal: 10 of 52 mantissa bits
    else { m = mant | (uint64_t(1) << 52); shift = 42 + (-14 - e); base = 0; }             // subnormal: units of 2^-24
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((uint64_t(1) << shift) - 1), half = uint64_t(1) << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;             // a carry moves into the exponent, up to infinity
    return sign | (uint16_t)(base + q);
}

// ---- frame: marching-cubes vertices (float32, index space) -> float64 in the input's frame -----------------------------------
// watertight.export_to_watertight: ((double(x) / size) * 2 - 1) / to_orig_scale + center[axis]
__global__ __launch_bounds__(256) void frame_kernel(const float* __restrict__ iv, int64_t n3, double size, double to_orig_scale, double cx,
                                                    double cy, double cz, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const int axis = (int)(i % 3);
    const double c = axis == 0 ? cx : axis == 1 ? cy : cz;
    const double x = (double)iv[i] / size * 2.0 - 1.0;
    out[i] = x / to_orig_scale + c;
}

// ---- per face: unit normal and area, as face_normals_and_areas -------------------------------------------------------------
// np.cross(t1 - t0, t2 - t0) (each product rounded, then subtracted), np.linalg.norm = sqrt((c0^2 + c1^2) + c2^2), area = 0.5 * norm,
// normal = cross / norm where norm > 0, else 0.  A face naming a vertex outside [0, nv) (the host refuses such input) gets area 0.
__global__ __launch_bounds__(256) void face_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                   double* __restrict__ normals, double* __restrict__ areas) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nf) return;
    const int64_t t3 = 3 * (int64_t)t;
    const int i0 = faces[t3], i1 = faces[t3 + 1], i2 = faces[t3 + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) {
        normals[t3] = normals[t3 + 1] = normals[t3 + 2] = 0.0;
        areas[t] = 0.0;
        return;
    }
    const double* a = verts + 3 * (int64_t)i0;
    const double* b = verts + 3 * (int64_t)i1;
    const double* c = verts + 3 * (int64_t)i2;
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    const double c0 = e1y * e2z - e1z * e2y, c1 = e1z * e2x - e1x * e2z, c2 = e1x * e2y - e1y * e2x;
    const double n = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    const bool ok = n > 0.0;
    normals[t3] = ok ? c0 / n : 0.0;
    normals[t3 + 1] = ok ? c1 / n : 0.0;
    normals[t3 + 2] = ok ? c2 / n : 0.0;
    areas[t] = 0.5 * n;
}

// ---- inclusive float64 scan: one 1024-element tile per 256-thread block, 4 consecutive elements per thread, tile totals scanned
// recursively (the layout of wt::scan_exclusive).  Op = Sum (the cumulative areas) or Max (the exact monotone pass).
struct SumOp { __device__ static double apply(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
} };
struct MaxOp { __device__ static double apply(double a, double b) { return fmax(a, b); } };   // operands are >= 0

using wt::SCAN_THREADS;
using wt::SCAN_ITEMS;
using wt::SCAN_TILE;

// out[i] = in[0] op ... op in[i], where an element whose mask is not > 0 counts as 0 (mask may be NULL).  in may equal out: every
// thread reads its own elements before it writes them.  tile_sums (may be NULL): the total of each tile.
template <class Op>
__global__ __launch_bounds__(SCAN_THREADS) void cdf_scan_tile_kernel(const double* in, const double* __restrict__ mask, double* out, int64_t n,
                                                                      double* __restrict__ tile_sums) {
    __shared__ double wave_sum[SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    double x[SCAN_ITEMS], s = 0.0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        x[i] = base + i < n && (!mask || mask[base + i] > 0.0) ? in[base + i] : 0.0;
        s = i ? Op::apply(s, x[i]) : x[i];
    }
    double inc = s;                                              // inclusive scan of the per-thread totals inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(inc, o, 64); if (lane >= o) inc = Op::apply(t, inc); }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    double run = 0.0, tot = wave_sum[0];
#pragma unroll
    for (int i = 0; i < SCAN_THREADS / 64; ++i) if (i < w) run = i ? Op::apply(run, wave_sum[i]) : wave_sum[i];
#pragma unroll
    for (int i = 1; i < SCAN_THREADS / 64; ++i) tot = Op::apply(tot, wave_sum[i]);
    if (lane > 0) run = w ? Op::apply(run, exc) : exc;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        run = Op::apply(run, x[i]);
        if (base + i < n) out[base + i] = run;
    }
    if (tile_sums && threadIdx.x == 0) tile_sums[blockIdx.x] = tot;
}

// tile b > 0: data[i] = incl[b - 1] op data[i], incl = the inclusive scan of the tile totals
template <class Op>
__global__ __launch_bounds__(SCAN_THREADS) void cdf_scan_add_kernel(double* __restrict__ data, int64_t n, const double* __restrict__ incl) {
    if (blockIdx.x == 0) return;
    const double add = incl[blockIdx.x - 1];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const int64_t idx = (int64_t)blockIdx.x * SCAN_TILE + i * SCAN_THREADS + threadIdx.x;
        if (idx < n) data[idx] = Op::apply(add, data[idx]);
    }
}

// ws: wt::scan_ws_elems(n) doubles
template <class Op>
inline hipError_t cdf_scan(const double* in, const double* mask, double* out, int64_t n, double* ws, hipStream_t s) {
    const int64_t nb = wt::scan_tiles(n);
    hipLaunchKernelGGL(cdf_scan_tile_kernel<Op>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, in, mask, out, n, nb > 1 ? ws : nullptr);
    if (nb > 1) {
        hipError_t r = cdf_scan<Op>(ws, nullptr, ws, nb, ws + nb, s);
        if (r != hipSuccess) return r;
        hipLaunchKernelGGL(cdf_scan_add_kernel<Op>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, out, n, ws);
    }
    return hipGetLastError();
}

struct CdfWs { double* areas; double* scan; };

inline size_t cdf_ws_bytes(int nf, CdfWs* ws = nullptr, void* base = nullptr) {
    const size_t b_areas = wt::align256((size_t)nf * sizeof(double));
    const size_t b_scan = wt::align256((size_t)wt::scan_ws_elems(nf) * sizeof(double));
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->areas = reinterpret_cast<double*>(p);
        ws->scan = reinterpret_cast<double*>(p + b_areas);
    }
    return b_areas + b_scan;
}

// normals (nf, 3) and cum (nf): the cumulative areas, non-decreasing, equal across a zero-area face; cum[nf - 1] is the total
inline hipError_t launch_surface_cdf(const double* verts, int nv, const int* faces, int nf, double* normals, double* cum, void* workspace,
                                     hipStream_t s) {
    CdfWs ws;
    cdf_ws_bytes(nf, &ws, workspace);
    hipLaunchKernelGGL(face_kernel, dim3((unsigned)(((int64_t)nf + 255) / 256)), dim3(256), 0, s, verts, nv, faces, nf, normals, ws.areas);
    hipError_t r = cdf_scan<SumOp>(ws.areas, nullptr, cum, nf, ws.scan, s);
    if (r != hipSuccess) return r;
    return cdf_scan<MaxOp>(cum, ws.areas, cum, nf, ws.scan, s);
}

// ---- draws: one thread per point, as mesh_input.sample_surface + the normal of the face under the point ----------------------
// pick = u * cum[nf - 1]; face = the first j with cum[j] > pick (np.searchsorted(side="right")), at most nf - 1; (a, b) -> (1 - a,
// 1 - b) when a + b > 1; point = (t0 + a * (t1 - t0)) + b * (t2 - t0); out row = point, normal as float16.
__global__ __launch_bounds__(256) void draw_kernel(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                   const double* __restrict__ normals, const double* __restrict__ cum,
                                                   const double* __restrict__ u, const double* __restrict__ uv, int count,
                                                   uint16_t* __restrict__ out, int64_t* __restrict__ face_idx) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    const double pick = u[p] * cum[nf - 1];
    int lo = 0, hi = nf;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > pick) hi = mid; else lo = mid + 1;
    }
    const int f = lo < nf ? lo : nf - 1;
    double a = uv[2 * (int64_t)p], b = uv[2 * (int64_t)p + 1];
    if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
    const int64_t f3 = 3 * (int64_t)f;
    int ix[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { const int v = faces[f3 + k]; ix[k] = v < 0 ? 0 : v >= nv ? nv - 1 : v; }   // in bounds on any input
    const double* t0 = verts + 3 * (int64_t)ix[0];
    const double* t1 = verts + 3 * (int64_t)ix[1];
    const double* t2 = verts + 3 * (int64_t)ix[2];
    uint16_t* o = out + 6 * (int64_t)p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = (t0[k] + a * (t1[k] - t0[k])) + b * (t2[k] - t0[k]);
        o[k] = f64_to_f16_rne(x);
        o[3 + k] = f64_to_f16_rne(normals[f3 + k]);
    }
    if (face_idx) face_idx[p] = f;
}

inline hipError_t launch_frame(const float* iv, int nv, int size, double to_orig_scale, const double* center, double* out, hipStream_t s) {
    const int64_t n3 = 3 * (int64_t)nv;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, iv, n3, (double)size, to_orig_scale, center[0], center[1],
                       center[2], out);
    return hipGetLastError();
}

inline hipError_t launch_draw(const double* verts, int nv, const int* faces, int nf, const double* normals, const double* cum, const double* u,
                              const double* uv, int count, uint16_t* out, int64_t* face_idx, hipStream_t s) {
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)(((int64_t)count + 255) / 256)), dim3(256), 0, s, verts, nv, faces, nf, normals, cum, u, uv, count,
                       out, face_idx);
    return hipGetLastError();
}

}  // namespace ss
}  // namespace ma
