// The tightest box of a point cloud (`--align_iters`): the axis-aligned extents of every row under up to 2^16 candidate
// rotations, their box volumes and the least of them.  Has no reference counterpart.
//
// The rule, with no FMA contraction.  c is the centre (three host floats), r the row-major 3x3 of hypothesis h, p a row:
//     q   = fl32(p - c)                                                    per axis
//     u_a = fl32(fl32(fl32(r_a0*qx) + fl32(r_a1*qy)) + fl32(r_a2*qz)) + 0.0f
// lo_a = min over the rows of u_a, hi_a = max.  Min and max do not depend on the order the rows are met in, and the + 0.0f, which turns
// -0 into +0, takes away the one case in which they would (a -0 against a +0): a numpy float32 restatement gives the same bits.  The
// kernel adds the 0.0f ONCE, to the finished lo and hi: a min or max that is a zero of either sign becomes +0 either way, every other
// value is unchanged.  A hypothesis is BAD iff one of its nine entries or one u_a of one row is not finite.
//
// `init_kernel`, one thread per hypothesis: the eight words of h in the workspace = the keys of +inf (lo, three), of -inf (hi, three), a
// bad flag (1 iff an entry of r is not finite) and a spare.  A key is the monotone map of the float's bits to uint32 (sign bit flipped for
// a positive float, every bit for a negative one), so unsigned integer order is float order and integer atomicMin / atomicMax combine
// workgroups in any order to the same value; no floating-point atomics.
//
// `extent_kernel`: workgroup (x, y) of 256 threads owns the ROWS rows from x * ROWS and the TILE hypotheses from y * TILE.  The 9 * TILE
// entries are read at wave-uniform addresses (scalar loads) and stay in registers; the rows stream through, one per lane and step,
// coalesced (the compiled loop waits for a row as soon as it has asked for it; the other waves of the SIMD, four at 103 VGPRs, cover the
// wait); a lane keeps 6 running min / max and one poison accumulator per
// hypothesis of the tile.  v_min_f32 / v_max_f32 skip a NaN, so non-finite u are caught apart from the extents: an infinite u shows in lo
// or hi; a NaN u is caught by poison = fma(u_a, 0.0f, poison), which is NaN from then on iff some u_a was infinite or NaN; a row with a
// non-finite q makes every u of every hypothesis non-finite and is caught once per row.  After the last row: a wave reduction by
// __shfl_xor, then lane 0 of each wave combines into an LDS table of keys with LDS integer atomics, then 7 * TILE threads do one global
// integer atomic each.  Rows past N are skipped (the lane's accumulators keep their start values, the identities of min and max); the
// hypotheses past H of the last tile compute h = H - 1 again and write nothing.
//
// `finish_kernel`, one thread per hypothesis: keys back to floats, + 0.0f, bad iff the flag is set or a lo or hi is not finite; extents
// (six NaN if bad), the volume ((double)hi0 - (double)lo0) * ((double)hi1 - (double)lo1) * ((double)hi2 - (double)lo2) in float64, each
// operation rounded once (+inf if bad), to `volumes` or, without it, to the workspace.  A hypothesis that is not bad has a finite volume,
// so +inf marks the bad ones.  `best_kernel`, one workgroup: the h of the least finite volume, the lowest index among equals, -1 if none.
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "watertight.hpp"

namespace ma {
namespace pca {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int STEPS = 32;                              // rows per lane of one workgroup
constexpr int ROWS = THREADS * STEPS;                  // rows of one workgroup: 8 192
constexpr int TILE = 8;                                // hypotheses of one workgroup: 72 scalars of rotation, 56 VGPRs of running values
constexpr int WORDS = 8;                               // per hypothesis in the workspace: lo (3), hi (3), bad, spare

struct Layout {
    size_t keys, vol, bytes;
};

// the keys (H, 8) uint32 | the volumes (H) float64, used when the caller takes none
inline Layout layout(int N, int H) {
    (void)N;
    Layout l;
    size_t o = 0;
    l.keys = o; o += wt::align256((size_t)H * WORDS * sizeof(uint32_t));
    l.vol = o;  o += wt::align256((size_t)H * sizeof(double));
    l.bytes = o;
    return l;
}

__device__ inline uint32_t key_of(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ inline bool finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(THREADS) void init_kernel(const float* __restrict__ rot, int H, uint32_t* __restrict__ keys) {
    const int h = blockIdx.x * THREADS + threadIdx.x;
    if (h >= H) return;
    bool bad = false;
    for (int k = 0; k < 9; ++k) bad |= !finite(rot[(size_t)h * 9 + k]);
    uint32_t* o = keys + (size_t)h * WORDS;
    const uint32_t lo = key_of(__uint_as_float(0x7f800000u)), hi = key_of(__uint_as_float(0xff800000u));
    o[0] = lo; o[1] = lo; o[2] = lo; o[3] = hi; o[4] = hi; o[5] = hi; o[6] = bad ? 1u : 0u; o[7] = 0u;
}

__global__ __launch_bounds__(THREADS) void extent_kernel(const float* __restrict__ ref, int N, int ref_ld, float cx, float cy, float cz,
                                                         const float* __restrict__ rot, int H, uint32_t* __restrict__ keys) {
#pragma clang fp contract(off)
    __shared__ uint32_t sh[TILE * 7];
    const int tid = threadIdx.x, lane = tid & 63;
    const int h0 = blockIdx.y * TILE;
    const float inf = __uint_as_float(0x7f800000u);
    float r[TILE][9], lo[TILE][3], hi[TILE][3], poison[TILE];
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
        const float* m = rot + (size_t)min(h0 + t, H - 1) * 9;       // the same address in every lane
#pragma unroll
        for (int k = 0; k < 9; ++k) r[t][k] = m[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[t][a] = inf; hi[t][a] = -inf; }
        poison[t] = 0.f;
    }
    if (tid < TILE * 7) sh[tid] = (tid % 7) < 3 ? 0xffffffffu : 0u;  // identities of the unsigned min (lo), max (hi) and or (bad)
    const long long first = (long long)blockIdx.x * ROWS + tid;
    const long long end = min((long long)N, (long long)(blockIdx.x + 1) * ROWS);
    bool row_bad = false;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (first < end) {
        const float* p = ref + (size_t)first * ref_ld;
        nx = p[0]; ny = p[1]; nz = p[2];
    }
    for (long long row = first; row < end; row += THREADS) {
        const float qx = nx - cx, qy = ny - cy, qz = nz - cz;
        if (row + THREADS < end) {                                   // the next row of this lane
            const float* p = ref + (size_t)(row + THREADS) * ref_ld;
            nx = p[0]; ny = p[1]; nz = p[2];
        }
        row_bad |= !(finite(qx) && finite(qy) && finite(qz));
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float u = (r[t][3 * a] * qx + r[t][3 * a + 1] * qy) + r[t][3 * a + 2] * qz;
                lo[t][a] = fminf(lo[t][a], u);
                hi[t][a] = fmaxf(hi[t][a], u);
                poison[t] = __builtin_fmaf(u, 0.f, poison[t]);
            }
        }
    }
    __syncthreads();                                                 // sh holds its identities
    const bool any_row_bad = __ballot(row_bad) != 0ull;
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float l = lo[t][a], g = hi[t][a];
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                l = fminf(l, __shfl_xor(l, w));
                g = fmaxf(g, __shfl_xor(g, w));
            }
            if (lane == 0) {
                atomicMin(&sh[t * 7 + a], key_of(l));
                atomicMax(&sh[t * 7 + 3 + a], key_of(g));
            }
        }
        const bool bad = any_row_bad || __ballot(poison[t] != poison[t]) != 0ull;
        if (lane == 0 && bad) atomicOr(&sh[t * 7 + 6], 1u);
    }
    __syncthreads();
    if (tid < TILE * 7) {
        const int t = tid / 7, w = tid % 7;
        if (h0 + t < H) {
            uint32_t* o = keys + (size_t)(h0 + t) * WORDS + w;
            const uint32_t v = sh[tid];
            if (w < 3) atomicMin(o, v);
            else if (w < 6) atomicMax(o, v);
            else if (v) atomicOr(o, 1u);
        }
    }
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const uint32_t* __restrict__ keys, int H, float* __restrict__ extents, double* __restrict__ volumes) {
#pragma clang fp contract(off)
    const int h = blockIdx.x * THREADS + threadIdx.x;
    if (h >= H) return;
    const uint32_t* k = keys + (size_t)h * WORDS;
    float e[6];
    bool bad = k[6] != 0u;
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        e[w] = float_of(k[w]) + 0.0f;
        bad |= !finite(e[w]);
    }
    if (extents) {
        const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
        for (int w = 0; w < 6; ++w) extents[(size_t)h * 6 + w] = bad ? nan : e[w];
    }
    double v = ((double)e[3] - (double)e[0]) * ((double)e[4] - (double)e[1]);
    v = v * ((double)e[5] - (double)e[2]);
    volumes[h] = bad ? (double)__uint_as_float(0x7f800000u) : v;
}

__global__ __launch_bounds__(THREADS) void best_kernel(const double* __restrict__ volumes, int H, int* __restrict__ best) {
    __shared__ double sh_v[THREADS];
    __shared__ int sh_h[THREADS];
    const double inf = (double)__uint_as_float(0x7f800000u);
    double bv = inf;
    int bh = -1;
    for (int h = threadIdx.x; h < H; h += THREADS) {                 // ascending h per thread: a strict < keeps the lowest index
        const double v = volumes[h];
        if (v < bv) { bv = v; bh = h; }
    }
    sh_v[threadIdx.x] = bv; sh_h[threadIdx.x] = bh;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double ov = sh_v[threadIdx.x + w], mv = sh_v[threadIdx.x];
            const int oh = sh_h[threadIdx.x + w], mh = sh_h[threadIdx.x];
            if (oh >= 0 && (mh < 0 || ov < mv || (ov == mv && oh < mh))) { sh_v[threadIdx.x] = ov; sh_h[threadIdx.x] = oh; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[0] = sh_h[0];
}

inline hipError_t launch_extents(const float* ref, int N, int ref_ld, const float* centre, const float* rot, int H, float* extents, double* volumes,
                                 int* best, void* workspace, hipStream_t s) {
    const Layout l = layout(N, H);
    char* ws = static_cast<char*>(workspace);
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws + l.keys);
    double* vol = volumes ? volumes : reinterpret_cast<double*>(ws + l.vol);
    const unsigned hyp_groups = (unsigned)((H + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(init_kernel, dim3(hyp_groups), dim3(THREADS), 0, s, rot, H, keys);
    hipLaunchKernelGGL(extent_kernel, dim3((unsigned)((N + ROWS - 1) / ROWS), (unsigned)((H + TILE - 1) / TILE)), dim3(THREADS), 0, s, ref, N, ref_ld,
                       centre[0], centre[1], centre[2], rot, H, keys);
    hipLaunchKernelGGL(finish_kernel, dim3(hyp_groups), dim3(THREADS), 0, s, keys, H, extents, vol);
    if (best) hipLaunchKernelGGL(best_kernel, dim3(1), dim3(THREADS), 0, s, vol, H, best);
    return hipGetLastError();
}

}  // namespace pca
}  // namespace ma
