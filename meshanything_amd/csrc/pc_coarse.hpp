// The device side of coarse registration from unknown poses, for `--coarse_radius`: a sign-free point feature
// histogram over every row's radius neighbourhood, its second pass at chosen rows, descriptor matching and the scoring of pose
// hypotheses; PCL's FPFHEstimation + SampleConsensusPrerejective and Open3D's compute_fpfh_feature +
// registration_ransac_based_on_feature_matching do the same job.  Has no reference counterpart.  Every op is a pure function of its
// inputs with integer outputs that a numpy float32 restatement gives byte for byte: no FMA contraction anywhere, IEEE sqrt and /, no
// floating-point atomics.
//
// SPFH (spfh_kernel), for row p at position x_p with normal n_p, r2 = fl32(F * F) computed once on the host:
//   neighbours: every row q with 0 < d <= r2, d = fl32(fl32(dx*dx + dy*dy) + dz*dz), dx = fl32(x_p.x - x_q.x), ...: the key of ma_op_pc_knn;
//     equality with r2 is included, a NaN key is no neighbour, and d = 0 (the row itself, a duplicate) has no direction and is skipped.
//   dot(u, v) = fl32(fl32(fl32(u_x*v_x) + fl32(u_y*v_y)) + fl32(u_z*v_z));  len = fl32(sqrt(d));  D = (dx, dy, dz)
//   a = fl32(|dot(n_p, D)| / len)    b = fl32(|dot(n_q, D)| / len)    c = |dot(n_p, n_q)|
//   bin(v) = 10 if fl32(v * 11) >= 10, else (int)fl32(v * 11): min(10, (int)fl32(v * 11)) without the overflowing cast
//   hist[p] = 34 uint32: [0..10] the counts of bin(a), [11..21] of bin(b), [22..32] of bin(c), [33] the pairs used.
//   A pair is SKIPPED, and counted nowhere, when either normal has a component that is not finite or is (0, 0, 0), or when a, b or c is
//   NaN.  The features carry no sign: the normals of a scan are unoriented, and a Darboux frame would need an orientation nobody has.
//   More than MAX_USED = 65 535 used pairs in one row is refused by the host after the kernel (the largest [33] goes to a word of the
//   workspace): under that limit the sums of the second pass cannot overflow 32 bits.
// Shape: one WAVE per row, rows in cell order (wave w owns record w) so that the waves of a workgroup walk the same cells; the ring and
// segment walk of pc_register.hpp (`pcreg::ring_walk`) with the radius stop rule, wave-uniform; the 64 lanes take the records of every
// range the walk hands out; the 34 counters of the row live in LDS (a data-dependent index into registers would go to scratch) and take
// integer ds atomics.  No neighbour list reaches memory.
//
// Gather (gather_kernel): desc[j] (33 uint32) = hist[p] + sum over the neighbours q of p = query[j] (the rule above: 0 < d <= r2, nothing
// else) of hist[q], columns 0..32, modulo 2^32: FPFH's second pass without the 1/d weights, so that the sums are integers, need no order
// and stay testable bit for bit.  A query outside [0, N) gives a zero row.  One wave per query, the 33 sums in each lane's registers
// (static indices), added up over the lanes in LDS.
//
// Match (match_kernel): A (Ka, 33), B (Kb, 33) uint32.  Every block of 11 is normalised by its integer sum S (64-bit):
// x = fl32(fl32(h) / fl32(S)), a zero block stays zero; dist(a, b) = the SEQUENTIAL float32 sum over bins 0..32 of fl32(fl32(x - y)^2), from 0.
// For every row of A: the row of B least in (dist, index), and that dist.  64 rows of A per workgroup, one per lane, normalised in
// registers; tiles of 256 normalised rows of B in LDS, each of the four waves scanning a quarter of the tile with broadcast reads; the
// waves' candidates are merged in LDS by the same order.
//
// Score (score_kernel): poses (H, 12) R row-major then t, P and Q (C, 3), t2 = fl32(T * T): counts[h] = the number of pairs i with
// key(p', Q_i) <= t2, p' = pcreg::transform(pose_h, P_i), the key as above between p' and Q_i; a NaN key agrees with nothing.  One
// thread per hypothesis, the pairs in LDS tiles read as broadcasts; then pc_plane's best_kernel: the highest count, the lowest index
// among equals.
//
// Non-finite values through the raw ABI: every read stays inside the records, the cell starts and the arrays given; row indices read
// from records are range-checked; a row whose position is not finite has no neighbour and walks nothing.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"
#include "pc_plane.hpp"
#include "pc_radius.hpp"
#include "pc_register.hpp"

namespace ma {
namespace pcf {

constexpr int THREADS = pcg::THREADS;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;                  // rows (spfh) or queries (gather) per workgroup
constexpr int BINS = 11;                               // MA_PC_SPFH_BINS
constexpr int DESC = 3 * BINS;                         // MA_PC_SPFH_DESC
constexpr int COLS = DESC + 1;                         // MA_PC_SPFH_COLS: the histogram and the pairs used
constexpr unsigned MAX_USED = 65535;                   // MA_PC_SPFH_MAX_USED
constexpr int MAX_KEYPOINTS = 4096;                    // MA_PC_COARSE_MAX_KEYPOINTS: rows of A and B, pairs of the score
constexpr int MAX_HYPOTHESES = 1 << 16;                // MA_PC_COARSE_MAX_HYPOTHESES
constexpr int MAX_QUERIES = 1 << 20;                   // MA_PC_SPFH_MAX_QUERIES
constexpr int MATCH_ROWS = WAVE;                       // rows of A per match workgroup
constexpr int MATCH_TILE = THREADS;                    // rows of B per LDS tile
constexpr int SCORE_TILE = THREADS;                    // pairs per LDS tile of the score

struct Layout {
    size_t most, bytes;
};

// pcr::layout(N, cells): the grid and the pair total | the largest number of used pairs of a row
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = pcr::layout(N, cells).bytes;
    l.most = o; o += wt::align256(sizeof(unsigned));
    l.bytes = o;
    return l;
}

__device__ inline float dot3(float ux, float uy, float uz, float vx, float vy, float vz) {
#pragma clang fp contract(off)
    return (ux * vx + uy * vy) + uz * vz;
}

__device__ inline bool usable(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.f && y == 0.f && z == 0.f); }

__device__ inline int bin_of(float v) {
#pragma clang fp contract(off)
    const float w = v * (float)BINS;
    return w >= (float)(BINS - 1) ? BINS - 1 : (int)w;
}

// the six side tests of the radius stop rule: no unsearched row can have a key <= r2
__device__ inline bool beyond(const pcg::Grid& g, float qx, float qy, float qz, float r2, int lx, int hx, int ly, int hy, int lz, int hz) {
#pragma clang fp contract(off)
    bool out = true;
    const auto side = [&](float b) { out = out && b * b > r2; };
    if (lx > 0) side(qx - pcg::face(g.ox, g.cell, lx));
    if (hx < g.nx - 1) side(qx - pcg::face(g.ox, g.cell, hx + 1));
    if (ly > 0) side(qy - pcg::face(g.oy, g.cell, ly));
    if (hy < g.ny - 1) side(qy - pcg::face(g.oy, g.cell, hy + 1));
    if (lz > 0) side(qz - pcg::face(g.oz, g.cell, lz));
    if (hz < g.nz - 1) side(qz - pcg::face(g.oz, g.cell, hz + 1));
    return out;
}

__device__ inline void cell_xyz(int id, const pcg::Grid& g, int& cx, int& cy, int& cz) {
    id = min(max(id, 0), g.nx * g.ny * g.nz - 1);
    cx = id % g.nx; cy = (id / g.nx) % g.ny; cz = id / (g.nx * g.ny);
}

__global__ __launch_bounds__(THREADS) void spfh_kernel(const float4* __restrict__ sorted, const int* __restrict__ start, const int* __restrict__ cell_id,
                                                       int N, const float* __restrict__ normals, int normals_ld, float r2, pcg::Grid g,
                                                       unsigned* __restrict__ hist, unsigned* __restrict__ most) {
#pragma clang fp contract(off)
    __shared__ unsigned sh[WAVES][COLS];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int t = blockIdx.x * WAVES + wave;                        // the wave's record: the same in all its lanes
    if (lane < COLS) sh[wave][lane] = 0u;
    __syncthreads();
    int qi = -1;
    if (t < N) {
        const float4 me = sorted[t];
        const float qx = me.x, qy = me.y, qz = me.z;
        qi = __float_as_int(me.w);
        if (qi < 0 || qi >= N) qi = -1;                             // a record the build did not write: no row to answer for
        if (qi >= 0 && isfinite(qx) && isfinite(qy) && isfinite(qz)) {
            const float* np = normals + (int64_t)qi * normals_ld;
            const float px = np[0], py = np[1], pz = np[2];
            if (usable(px, py, pz)) {                               // otherwise every pair of this row is skipped
                int cx, cy, cz;
                cell_xyz(cell_id[qi], g, cx, cy, cz);
                unsigned used = 0;
                pcreg::ring_walk(
                    g, start, N, cx, cy, cz,
                    [&](int p0, int p1) {
                        for (int p = p0 + lane; p < p1; p += WAVE) {
                            const float4 c = sorted[p];
                            const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                            const float d = (dx * dx + dy * dy) + dz * dz;
                            const int i = __float_as_int(c.w);
                            if (!(d > 0.f && d <= r2) || i < 0 || i >= N) continue;
                            const float* nq = normals + (int64_t)i * normals_ld;
                            const float ox = nq[0], oy = nq[1], oz = nq[2];
                            if (!usable(ox, oy, oz)) continue;
                            const float len = sqrtf(d);
                            const float fa = fabsf(dot3(px, py, pz, dx, dy, dz)) / len;
                            const float fb = fabsf(dot3(ox, oy, oz, dx, dy, dz)) / len;
                            const float fc = fabsf(dot3(px, py, pz, ox, oy, oz));
                            if (fa != fa || fb != fb || fc != fc) continue;
                            atomicAdd(&sh[wave][bin_of(fa)], 1u);
                            atomicAdd(&sh[wave][BINS + bin_of(fb)], 1u);
                            atomicAdd(&sh[wave][2 * BINS + bin_of(fc)], 1u);
                            ++used;
                        }
                    },
                    [&](int lx, int hx, int ly, int hy, int lz, int hz) { return beyond(g, qx, qy, qz, r2, lx, hx, ly, hy, lz, hz); });
                if (used) atomicAdd(&sh[wave][DESC], used);
            }
        }
    }
    __syncthreads();
    if (qi >= 0 && lane < COLS) {
        const unsigned v = sh[wave][lane];
        hist[(int64_t)qi * COLS + lane] = v;
        if (lane == DESC && v > MAX_USED) atomicMax(most, v);
    }
}

__global__ __launch_bounds__(THREADS) void gather_kernel(const float* __restrict__ ref, int N, int ref_ld, const float4* __restrict__ sorted,
                                                         const int* __restrict__ start, const int* __restrict__ cell_id, float r2, pcg::Grid g,
                                                         const unsigned* __restrict__ hist, const int* __restrict__ query, int Q,
                                                         unsigned* __restrict__ desc) {
#pragma clang fp contract(off)
    __shared__ unsigned sh[WAVES][DESC];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int j = blockIdx.x * WAVES + wave;
    if (lane < DESC) sh[wave][lane] = 0u;
    __syncthreads();
    if (j < Q) {
        const int qi = query[j];
        if (qi >= 0 && qi < N) {
            unsigned acc[DESC];
#pragma unroll
            for (int k = 0; k < DESC; ++k) acc[k] = lane == 0 ? hist[(int64_t)qi * COLS + k] : 0u;
            const float* me = ref + (int64_t)qi * ref_ld;
            const float qx = me[0], qy = me[1], qz = me[2];
            if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
                int cx, cy, cz;
                cell_xyz(cell_id[qi], g, cx, cy, cz);
                pcreg::ring_walk(
                    g, start, N, cx, cy, cz,
                    [&](int p0, int p1) {
                        for (int p = p0 + lane; p < p1; p += WAVE) {
                            const float4 c = sorted[p];
                            const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                            const float d = (dx * dx + dy * dy) + dz * dz;
                            const int i = __float_as_int(c.w);
                            if (!(d > 0.f && d <= r2) || i < 0 || i >= N) continue;
                            const unsigned* h = hist + (int64_t)i * COLS;
#pragma unroll
                            for (int k = 0; k < DESC; ++k) acc[k] += h[k];
                        }
                    },
                    [&](int lx, int hx, int ly, int hy, int lz, int hz) { return beyond(g, qx, qy, qz, r2, lx, hx, ly, hy, lz, hz); });
            }
#pragma unroll
            for (int k = 0; k < DESC; ++k) {
                if (acc[k]) atomicAdd(&sh[wave][k], acc[k]);
            }
        }
    }
    __syncthreads();
    if (j < Q && lane < DESC) desc[(int64_t)j * DESC + lane] = sh[wave][lane];
}

// row (33 uint32) -> x (33 float): every block of 11 over its 64-bit integer sum, a zero block stays zero
__device__ inline void normalise(const unsigned* __restrict__ row, float (&x)[DESC]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        unsigned long long S = 0;
#pragma unroll
        for (int k = 0; k < BINS; ++k) S += row[b * BINS + k];
        const float fs = (float)S;
#pragma unroll
        for (int k = 0; k < BINS; ++k) x[b * BINS + k] = S ? (float)row[b * BINS + k] / fs : 0.f;
    }
}

__global__ __launch_bounds__(THREADS) void match_kernel(const unsigned* __restrict__ A, int Ka, const unsigned* __restrict__ B, int Kb,
                                                        int* __restrict__ idx, float* __restrict__ dist) {
#pragma clang fp contract(off)
    __shared__ float tile[MATCH_TILE][DESC];                        // 33 words a row: an odd stride, a row per lane without conflicts
    __shared__ float sh_d[WAVES][MATCH_ROWS];
    __shared__ int sh_i[WAVES][MATCH_ROWS];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int a = blockIdx.x * MATCH_ROWS + lane;
    float x[DESC];
    normalise(A + (int64_t)min(a, Ka - 1) * DESC, x);
    float bd = INFINITY;
    int bi = INT_MAX;
    for (int base = 0; base < Kb; base += MATCH_TILE) {
        const int n = min(MATCH_TILE, Kb - base);
        if ((int)threadIdx.x < n) {
            float y[DESC];
            normalise(B + (int64_t)(base + threadIdx.x) * DESC, y);
#pragma unroll
            for (int k = 0; k < DESC; ++k) tile[threadIdx.x][k] = y[k];
        }
        __syncthreads();
        const int r1 = min((wave + 1) * (MATCH_TILE / WAVES), n);
        for (int r = wave * (MATCH_TILE / WAVES); r < r1; ++r) {     // one address for the wave: a broadcast
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < DESC; ++k) {
                const float e = x[k] - tile[r][k];
                s = s + e * e;
            }
            if (s < bd) { bd = s; bi = base + r; }                  // ascending index per wave: a strict < keeps the lowest
        }
        __syncthreads();
    }
    sh_d[wave][lane] = bd;
    sh_i[wave][lane] = bi;
    __syncthreads();
    if (wave == 0 && a < Ka) {
        for (int w = 1; w < WAVES; ++w) {
            const float od = sh_d[w][lane];
            const int oi = sh_i[w][lane];
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        idx[a] = bi == INT_MAX ? -1 : bi;
        if (dist) dist[a] = bd;
    }
}

__global__ __launch_bounds__(THREADS) void score_kernel(const float* __restrict__ poses, int H, const float* __restrict__ P, const float* __restrict__ Q,
                                                        int C, float t2, int* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ float sp[SCORE_TILE][3], sq[SCORE_TILE][3];
    const int h = blockIdx.x * THREADS + threadIdx.x;
    pcreg::Pose pose;
    const float* src = poses + (int64_t)min(h, H - 1) * 12;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose.r[k] = src[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose.t[k] = src[9 + k];
    int count = 0;
    for (int base = 0; base < C; base += SCORE_TILE) {
        const int n = min(SCORE_TILE, C - base);
        if ((int)threadIdx.x < n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sp[threadIdx.x][k] = P[(int64_t)(base + threadIdx.x) * 3 + k];
                sq[threadIdx.x][k] = Q[(int64_t)(base + threadIdx.x) * 3 + k];
            }
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {                               // one address for the wave: a broadcast
            float px, py, pz;
            pcreg::transform(pose, sp[i][0], sp[i][1], sp[i][2], px, py, pz);
            const float dx = px - sq[i][0], dy = py - sq[i][1], dz = pz - sq[i][2];
            const float d = (dx * dx + dy * dy) + dz * dz;
            count += d <= t2 ? 1 : 0;                               // a NaN key agrees with nothing
        }
        __syncthreads();
    }
    if (h < H) counts[h] = count;
}

inline unsigned* most_of(int N, const pcg::Grid& g, void* workspace) {
    return reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + layout(N, pcg::cells_of(g)).most);
}

// over the grid pcr::launch_bound built
inline hipError_t launch_spfh(int N, const float* normals, int normals_ld, float r2, const pcg::Grid& g, unsigned* hist, void* workspace, hipStream_t s) {
    const pcg::Layout gl = pcg::layout(N, pcg::cells_of(g));
    char* ws = static_cast<char*>(workspace);
    unsigned* most = most_of(N, g, workspace);
    const hipError_t e = hipMemsetAsync(most, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)((N + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, reinterpret_cast<const float4*>(ws + gl.sorted),
                       reinterpret_cast<const int*>(ws + gl.start), reinterpret_cast<const int*>(ws + gl.cell_id), N, normals, normals_ld, r2, g, hist, most);
    return hipGetLastError();
}

inline hipError_t launch_gather(const float* ref, int N, int ref_ld, float r2, const pcg::Grid& g, const unsigned* hist, const int* query, int Q,
                                unsigned* desc, void* workspace, hipStream_t s) {
    const pcg::Layout gl = pcg::layout(N, pcg::cells_of(g));
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((Q + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, ref, N, ref_ld,
                       reinterpret_cast<const float4*>(ws + gl.sorted), reinterpret_cast<const int*>(ws + gl.start),
                       reinterpret_cast<const int*>(ws + gl.cell_id), r2, g, hist, query, Q, desc);
    return hipGetLastError();
}

inline hipError_t launch_match(const unsigned* A, int Ka, const unsigned* B, int Kb, int* idx, float* dist, hipStream_t s) {
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)((Ka + MATCH_ROWS - 1) / MATCH_ROWS)), dim3(THREADS), 0, s, A, Ka, B, Kb, idx, dist);
    return hipGetLastError();
}

// counts (H) and, if given, best (1): the h of the highest count, the lowest index among equals
inline hipError_t launch_score(const float* poses, int H, const float* P, const float* Q, int C, float t2, int* counts, int* best, hipStream_t s) {
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)((H + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, poses, H, P, Q, C, t2, counts);
    if (best) hipLaunchKernelGGL(pcp::best_kernel, dim3(1), dim3(pcp::THREADS), 0, s, counts, H, best);
    return hipGetLastError();
}

}  // namespace pcf
}  // namespace ma
