// Dominant planes of a point cloud (`--plane_threshold`): score RANSAC plane hypotheses against every row, and apply
// one plane.  Has no reference counterpart.
//
// The inlier rule (one device function, `inlier`, used by both entry points).  A plane is six float32, a point a and a normal n of any
// length; t2 = fl32(threshold * threshold) is computed once on the host.  With no FMA contraction:
//     len2 = fl32(fl32(nx*nx + ny*ny) + nz*nz),  rhs = fl32(t2 * len2)                        (`plane_rhs`, host and device)
//     d = fl32(p - a) per axis,  s = fl32(fl32(fl32(nx*dx) + fl32(ny*dy)) + fl32(nz*dz))
//     row p is an INLIER iff fl32(s*s) <= rhs
// equality included; no square root and no division, so a numpy float32 restatement gives the same bits.  A plane is DEGENERATE iff
// !(len2 > 0) or rhs is not finite; `plane_rhs` then returns -1, and fl32(s*s) <= -1 holds for no row.  A NaN or infinite row makes s*s
// NaN or +inf, and rhs is finite: never an inlier.
//
// Score.  `plane_kernel`, one thread per hypothesis h with rows (i, j, k) of `tri`: a = p_i, e1 = fl32(p_j - p_i), e2 = fl32(p_k - p_i),
// n = e1 x e2 with every product and the difference rounded separately; an index outside [0, N) makes h degenerate without a read (its
// plane is six zeros).  It writes the eight floats (a, n, rhs, 0) of h to the workspace, `planes` if given, and counts[h] = 0, or -1 for
// a degenerate h.  `score_kernel`: a workgroup of 256 threads owns a tile of 256 * PTS rows, PTS per lane, held in registers for the
// whole launch (rows past N are NaN: never inliers).  The hypotheses pass through LDS in chunks of CHUNK: every lane of a wave reads the
// same address, which broadcasts; per hypothesis a wave sums __popcll(__ballot(inlier)) over its PTS slots and lane 0 stores the sum to
// the wave's row of an LDS table; after the chunk thread c adds the four waves' entries and, where the sum is not 0, does ONE global
// integer atomicAdd on counts[c].  A degenerate h collects no inlier, so its -1 is never touched.  Integer adds commute: counts is a
// function of the inputs alone.  `best_kernel`, one workgroup: the h of the greatest count, the lowest index among equals, -1 if every
// count is -1.
//
// Apply.  `apply_kernel`: a workgroup owns 256 * APPLY_PTS rows; mask[i] = inlier; per thread the count and, if asked for, the ten
// float64 moments over its inliers in row order with q = (double)p - (double)a (n, Sqx, Sqy, Sqz, Sqxqx, Sqxqy, Sqxqz, Sqyqy, Sqyqz,
// Sqzqz), no FMA contraction; then a tree over the 256 threads in LDS, of fixed shape, to one partial per workgroup.  `finish_kernel`:
// one thread per moment adds the partials in index order.  No atomics at all: two runs give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "watertight.hpp"

namespace ma {
namespace pcp {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PTS = 8;                                 // rows per lane of the score kernel: 24 VGPRs of coordinates
constexpr int CHUNK = 256;                             // hypotheses in LDS at a time: 8 KB of planes + 4 KB of wave counts
constexpr int APPLY_PTS = 4;
constexpr int MOMENTS = 10;

struct Layout {
    size_t partial, partial_count, hyp, bytes;
};

inline int apply_groups(int N) { return (N + THREADS * APPLY_PTS - 1) / (THREADS * APPLY_PTS); }

// the apply partials (groups, 10) float64 | their counts (groups) int32 | the hypotheses (H, 8) float32
inline Layout layout(int N, int H) {
    Layout l;
    size_t o = 0;
    const size_t groups = (size_t)apply_groups(N);
    l.partial = o;       o += wt::align256(groups * MOMENTS * sizeof(double));
    l.partial_count = o; o += wt::align256(groups * sizeof(int));
    l.hyp = o;           o += wt::align256((size_t)H * 8 * sizeof(float));
    l.bytes = o;
    return l;
}

// rhs of the inlier rule, -1 for a degenerate plane
__host__ __device__ inline float plane_rhs(float nx, float ny, float nz, float t2) {
#pragma clang fp contract(off)
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    const float rhs = t2 * len2;
    return (len2 > 0.f && rhs <= 3.402823466e+38f) ? rhs : -1.f;    // rhs >= 0 here, so "finite" is rhs <= FLT_MAX (false for NaN)
}

__device__ inline bool inlier(float px, float py, float pz, float ax, float ay, float az, float nx, float ny, float nz, float rhs) {
#pragma clang fp contract(off)
    const float dx = px - ax, dy = py - ay, dz = pz - az;
    const float s = (nx * dx + ny * dy) + nz * dz;
    return s * s <= rhs;
}

// ---- score --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void plane_kernel(const float* __restrict__ ref, int N, int ref_ld, const int* __restrict__ tri, int H, float t2,
                                                        float4* __restrict__ hyp, float* __restrict__ planes, int* __restrict__ counts) {
#pragma clang fp contract(off)
    const int h = blockIdx.x * THREADS + threadIdx.x;
    if (h >= H) return;
    const int i = tri[3 * h], j = tri[3 * h + 1], k = tri[3 * h + 2];
    float ax = 0.f, ay = 0.f, az = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, rhs = -1.f;
    if (i >= 0 && i < N && j >= 0 && j < N && k >= 0 && k < N) {
        const float* pi = ref + (size_t)i * ref_ld;
        const float* pj = ref + (size_t)j * ref_ld;
        const float* pk = ref + (size_t)k * ref_ld;
        ax = pi[0]; ay = pi[1]; az = pi[2];
        const float e1x = pj[0] - ax, e1y = pj[1] - ay, e1z = pj[2] - az;
        const float e2x = pk[0] - ax, e2y = pk[1] - ay, e2z = pk[2] - az;
        nx = e1y * e2z - e1z * e2y;
        ny = e1z * e2x - e1x * e2z;
        nz = e1x * e2y - e1y * e2x;
        rhs = plane_rhs(nx, ny, nz, t2);
    }
    hyp[2 * h] = make_float4(ax, ay, az, nx);
    hyp[2 * h + 1] = make_float4(ny, nz, rhs, 0.f);
    if (planes) {
        float* o = planes + (size_t)h * 6;
        o[0] = ax; o[1] = ay; o[2] = az; o[3] = nx; o[4] = ny; o[5] = nz;
    }
    counts[h] = rhs < 0.f ? -1 : 0;
}

__global__ __launch_bounds__(THREADS) void score_kernel(const float* __restrict__ ref, int N, int ref_ld, const float4* __restrict__ hyp, int H,
                                                        int* __restrict__ counts) {
    __shared__ float4 sh_hyp[2 * CHUNK];
    __shared__ int sh_cnt[WAVES * CHUNK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float nan = __int_as_float(0x7fc00000);
    float px[PTS], py[PTS], pz[PTS];
#pragma unroll
    for (int u = 0; u < PTS; ++u) {
        const long long row = ((long long)blockIdx.x * PTS + u) * THREADS + tid;
        const bool in = row < N;
        const float* p = ref + (size_t)(in ? row : 0) * ref_ld;
        px[u] = in ? p[0] : nan; py[u] = in ? p[1] : nan; pz[u] = in ? p[2] : nan;
    }
    for (int base = 0; base < H; base += CHUNK) {
        const int n = min(CHUNK, H - base);
        if (tid < n) {
            sh_hyp[2 * tid] = hyp[2 * (base + tid)];
            sh_hyp[2 * tid + 1] = hyp[2 * (base + tid) + 1];
        }
        __syncthreads();
        for (int c = 0; c < n; ++c) {
            const float4 a = sh_hyp[2 * c], b = sh_hyp[2 * c + 1];   // one address for the wave: a broadcast
            int sum = 0;
#pragma unroll
            for (int u = 0; u < PTS; ++u) sum += __popcll(__ballot(inlier(px[u], py[u], pz[u], a.x, a.y, a.z, a.w, b.x, b.y, b.z)));
            if (lane == 0) sh_cnt[wave * CHUNK + c] = sum;
        }
        __syncthreads();
        if (tid < n) {
            int sum = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) sum += sh_cnt[w * CHUNK + tid];
            if (sum != 0) atomicAdd(&counts[base + tid], sum);
        }
        // the next chunk's planes overwrite sh_hyp only after the barrier above, its counts overwrite sh_cnt only after the barrier below
    }
}

__global__ __launch_bounds__(THREADS) void best_kernel(const int* __restrict__ counts, int H, int* __restrict__ best) {
    __shared__ int sh_c[THREADS], sh_h[THREADS];
    int bc = -1, bh = -1;
    for (int h = threadIdx.x; h < H; h += THREADS) {                 // ascending h per thread: a strict > keeps the lowest index
        const int c = counts[h];
        if (c > bc) { bc = c; bh = h; }
    }
    sh_c[threadIdx.x] = bc; sh_h[threadIdx.x] = bh;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int oc = sh_c[threadIdx.x + w], oh = sh_h[threadIdx.x + w];
            const int mc = sh_c[threadIdx.x], mh = sh_h[threadIdx.x];
            if (oc > mc || (oc == mc && oh >= 0 && oh < mh)) { sh_c[threadIdx.x] = oc; sh_h[threadIdx.x] = oh; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[0] = sh_c[0] >= 0 ? sh_h[0] : -1;
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------
struct Plane {
    float ax, ay, az, nx, ny, nz, rhs;
};

__global__ __launch_bounds__(THREADS) void apply_kernel(const float* __restrict__ ref, int N, int ref_ld, Plane pl, uint8_t* __restrict__ mask,
                                                        double* __restrict__ partial, int* __restrict__ partial_count, int want_moments) {
#pragma clang fp contract(off)
    __shared__ double sh[THREADS];
    __shared__ int sh_n[THREADS];
    const int tid = threadIdx.x;
    double m[MOMENTS];
#pragma unroll
    for (int q = 0; q < MOMENTS; ++q) m[q] = 0.0;
    int mine = 0;
    for (int u = 0; u < APPLY_PTS; ++u) {
        const long long row = ((long long)blockIdx.x * APPLY_PTS + u) * THREADS + tid;
        if (row >= N) break;
        const float* p = ref + (size_t)row * ref_ld;
        const float x = p[0], y = p[1], z = p[2];
        const bool in = inlier(x, y, z, pl.ax, pl.ay, pl.az, pl.nx, pl.ny, pl.nz, pl.rhs);
        if (mask) mask[row] = in ? 1 : 0;
        if (in) {
            ++mine;
            if (want_moments) {
                const double qx = (double)x - (double)pl.ax, qy = (double)y - (double)pl.ay, qz = (double)z - (double)pl.az;
                m[0] += 1.0; m[1] += qx; m[2] += qy; m[3] += qz;
                m[4] += qx * qx; m[5] += qx * qy; m[6] += qx * qz; m[7] += qy * qy; m[8] += qy * qz; m[9] += qz * qz;
            }
        }
    }
    sh_n[tid] = mine;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) sh_n[tid] += sh_n[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial_count[blockIdx.x] = sh_n[0];
    if (!want_moments) return;
#pragma unroll
    for (int q = 0; q < MOMENTS; ++q) {                              // the same tree for every moment and every run
        sh[tid] = m[q];
        __syncthreads();
        for (int w = THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) sh[tid] += sh[tid + w];
            __syncthreads();
        }
        if (tid == 0) partial[(size_t)blockIdx.x * MOMENTS + q] = sh[0];
        __syncthreads();
    }
}

// thread q < 10: moment q, thread 10: the count; the partials in index order
__global__ __launch_bounds__(64) void finish_kernel(const double* __restrict__ partial, const int* __restrict__ partial_count, int groups,
                                                    int* __restrict__ count, double* __restrict__ moments) {
#pragma clang fp contract(off)
    const int q = threadIdx.x;
    if (q < MOMENTS && moments) {
        double s = 0.0;
        for (int g = 0; g < groups; ++g) s += partial[(size_t)g * MOMENTS + q];
        moments[q] = s;
    } else if (q == MOMENTS && count) {
        int s = 0;
        for (int g = 0; g < groups; ++g) s += partial_count[g];
        count[0] = s;
    }
}

inline hipError_t launch_score(const float* ref, int N, int ref_ld, const int* tri, int H, float t2, float* planes, int* counts, int* best,
                               void* workspace, hipStream_t s) {
    float4* hyp = reinterpret_cast<float4*>(static_cast<char*>(workspace) + layout(N, H).hyp);
    hipLaunchKernelGGL(plane_kernel, dim3((unsigned)((H + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, ref, N, ref_ld, tri, H, t2, hyp, planes, counts);
    const int tile = THREADS * PTS;
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((N + tile - 1) / tile)), dim3(THREADS), 0, s, ref, N, ref_ld, hyp, H, counts);
    hipLaunchKernelGGL(best_kernel, dim3(1), dim3(THREADS), 0, s, counts, H, best);
    return hipGetLastError();
}

inline hipError_t launch_apply(const float* ref, int N, int ref_ld, const Plane& pl, uint8_t* mask, int* count, double* moments, void* workspace,
                               hipStream_t s) {
    const Layout l = layout(N, 1);
    char* ws = static_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(ws + l.partial);
    int* partial_count = reinterpret_cast<int*>(ws + l.partial_count);
    const int groups = apply_groups(N);
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)groups), dim3(THREADS), 0, s, ref, N, ref_ld, pl, mask, partial, partial_count, moments ? 1 : 0);
    if (count || moments) hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, s, partial, partial_count, groups, count, moments);
    return hipGetLastError();
}

}  // namespace pcp
}  // namespace ma
