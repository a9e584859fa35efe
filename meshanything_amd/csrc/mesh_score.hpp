// Scores of candidate meshes against the point cloud they were generated from (best-of-N sampling).  Has no
// reference counterpart: the reference draws one mesh per cloud and leaves re-running with other seeds to the user.
//
// Per candidate b of coords (B, F, 3, 3) -- the detokenizer's output, a face with any non-finite coordinate is invalid and skipped,
// every vertex is multiplied by mesh_scale first -- against cloud b / n_per_cloud of cloud (B / n_per_cloud, P, cloud_ld), xyz in the
// first three columns:
//   [0] cloud to mesh: the mean over the P points of the distance to the nearest valid face (wt::tri_dist, flat = 2^-20: a face fp32
//       cannot resolve counts as its three edges)
//   [1] mesh to cloud: sum_f area_f * (1/7) sum_k nn(q_fk) / sum_f area_f, q_f = the 3 vertices, 3 edge midpoints and centroid of
//       face f, nn = the distance to the nearest cloud point
//   [2] sum_f area_f      [3] the number of valid faces
// [0] = [1] = +inf without a valid face, [1] = +inf when every valid face has zero area; never NaN.
//
// Three launches.  The per-point distances and per-face terms go to workspace in fp32; one block per candidate then sums them in
// fp64 in a fixed order: points by index, faces by their index AMONG THE VALID ONES, so that NaN rows between valid faces do not
// change a bit of the result.  No float atomics, nothing depends on B: bitwise reproducible.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "watertight.hpp"

namespace ma {
namespace score {

using wt::F3;

constexpr int PT_THREADS = 256;      // cloud-to-mesh: points per workgroup, one per thread
constexpr int TRI_TILE = 256;        // ... and faces staged per pass: 9 KB of LDS
constexpr int FACE_THREADS = 64;     // mesh-to-cloud: faces per workgroup, one per thread
constexpr int CLOUD_TILE = 1024;     // ... and cloud points staged per pass: 12 KB of LDS
constexpr int RED_THREADS = 256;     // the reduction's block
constexpr int MAX_GRID_Y = 65535;    // candidates per launch (grid.y); more are scored in several rounds
constexpr float FLAT = 1.0f / 1048576.0f;
static_assert(TRI_TILE == PT_THREADS && RED_THREADS == 256, "block_rank and the staging loops assume 256 threads");

// the face at c9 (3 vertices x xyz), scaled; false when any coordinate is not finite
__device__ inline bool load_face(const float* __restrict__ c9, float scale, F3& A, F3& B, F3& C) {
    float v[9];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) { v[i] = c9[i]; ok = ok && isfinite(v[i]); }
    A = {v[0] * scale, v[1] * scale, v[2] * scale};
    B = {v[3] * scale, v[4] * scale, v[5] * scale};
    C = {v[6] * scale, v[7] * scale, v[8] * scale};
    return ok;
}

// 256 threads: the number of flagged threads before this one, in thread order, and their total.  cnt: 4 ints of LDS, free again
// after the caller's next barrier.
__device__ inline int block_rank(bool flag, int* cnt, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) cnt[w] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { if (i < w) before += cnt[i]; total += cnt[i]; }
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// grid (tiles of PT_THREADS points, candidates): the candidate's faces pass through LDS in tiles of TRI_TILE, NaN rows dropped while
// staging; every lane then reads the same triangle (a broadcast).  pt_dist[b * P + p] = the least distance, +inf without a valid face.
__global__ __launch_bounds__(PT_THREADS) void cloud_to_mesh_kernel(const float* __restrict__ coords, int b0, int F, const float* __restrict__ cloud,
                                                                   int cloud_ld, int P, int n_per_cloud, float scale, float* __restrict__ pt_dist) {
    __shared__ float tri[TRI_TILE * 9];
    __shared__ int cnt[4];
    const int b = b0 + blockIdx.y;
    const int p = blockIdx.x * PT_THREADS + threadIdx.x;
    const bool live = p < P;
    F3 q = {0.f, 0.f, 0.f};
    if (live) {
        const float* c = cloud + ((int64_t)(b / n_per_cloud) * P + p) * cloud_ld;
        q = {c[0], c[1], c[2]};
    }
    const float* cf = coords + (int64_t)b * F * 9;
    float d = INFINITY;
    for (int f0 = 0; f0 < F; f0 += TRI_TILE) {
        const int f = f0 + threadIdx.x;
        F3 A, B, C;
        const bool ok = f < F && load_face(cf + (int64_t)f * 9, scale, A, B, C);
        int total;
        const int r = block_rank(ok, cnt, total);
        if (ok) {
            float* t = tri + r * 9;                              // stride 9 dwords: no bank conflict
            t[0] = A.x; t[1] = A.y; t[2] = A.z; t[3] = B.x; t[4] = B.y; t[5] = B.z; t[6] = C.x; t[7] = C.y; t[8] = C.z;
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < total; ++i) {
                const float* t = tri + i * 9;
                // fminf drops a NaN (coordinates near FLT_MAX overflow inside tri_dist): the distance stays +inf or what it was
                d = fminf(d, wt::tri_dist(F3{t[0], t[1], t[2]}, F3{t[3], t[4], t[5]}, F3{t[6], t[7], t[8]}, q, FLAT));
            }
        }
        __syncthreads();
    }
    if (live) pt_dist[(int64_t)b * P + p] = d;
}

// grid (tiles of FACE_THREADS faces, candidates): a thread keeps its face's 7 quadrature points, the cloud's xyz passes through LDS
// in tiles of CLOUD_TILE.  face_nn[b * F + f] = (1/7) sum_k nn(q_fk), face_area[b * F + f] = the area; an invalid face: 0 and -1.
__global__ __launch_bounds__(FACE_THREADS) void mesh_to_cloud_kernel(const float* __restrict__ coords, int b0, int F, const float* __restrict__ cloud,
                                                                     int cloud_ld, int P, int n_per_cloud, float scale, float* __restrict__ face_nn,
                                                                     float* __restrict__ face_area) {
    __shared__ float pts[CLOUD_TILE * 3];
    const int b = b0 + blockIdx.y;
    const int f = blockIdx.x * FACE_THREADS + threadIdx.x;
    const bool live = f < F;
    F3 A = {0.f, 0.f, 0.f}, B = A, C = A;
    const bool ok = live && load_face(coords + ((int64_t)b * F + f) * 9, scale, A, B, C);
    const F3 q[7] = {A, B, C,
                     {0.5f * (A.x + B.x), 0.5f * (A.y + B.y), 0.5f * (A.z + B.z)},
                     {0.5f * (B.x + C.x), 0.5f * (B.y + C.y), 0.5f * (B.z + C.z)},
                     {0.5f * (C.x + A.x), 0.5f * (C.y + A.y), 0.5f * (C.z + A.z)},
                     {(A.x + B.x + C.x) * (1.0f / 3.0f), (A.y + B.y + C.y) * (1.0f / 3.0f), (A.z + B.z + C.z) * (1.0f / 3.0f)}};
    float d2[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) d2[k] = INFINITY;
    const float* cb = cloud + (int64_t)(b / n_per_cloud) * P * cloud_ld;
    for (int p0 = 0; p0 < P; p0 += CLOUD_TILE) {
        const int n = min(CLOUD_TILE, P - p0);
        for (int i = threadIdx.x; i < n; i += FACE_THREADS) {
            const float* c = cb + (int64_t)(p0 + i) * cloud_ld;
            pts[3 * i] = c[0]; pts[3 * i + 1] = c[1]; pts[3 * i + 2] = c[2];   // stride 3 dwords: no bank conflict
        }
        __syncthreads();
        if (ok) {
            for (int i = 0; i < n; ++i) {
                const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const float dx = q[k].x - x, dy = q[k].y - y, dz = q[k].z - z;
                    d2[k] = fminf(d2[k], dx * dx + dy * dy + dz * dz);
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    float nn = 0.f, area = -1.f;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 7; ++k) nn += sqrtf(d2[k]);
        nn *= 1.0f / 7.0f;
        const F3 n = wt::cross(wt::sub(B, A), wt::sub(C, A));
        area = 0.5f * sqrtf(wt::dot(n, n));
        if (!(area >= 0.f)) area = INFINITY;                     // NaN from an overflow: the reduction turns it into a +inf score
    }
    face_nn[(int64_t)b * F + f] = nn;
    face_area[(int64_t)b * F + f] = area;
}

// one block per candidate.  Thread t sums the points t, t + 256, ... in fp64; the valid faces are numbered in face order and face
// number c goes to accumulator c mod 256, in increasing c; then one fixed tree over the 256 accumulators.
__global__ __launch_bounds__(RED_THREADS) void reduce_kernel(const float* __restrict__ pt_dist, const float* __restrict__ face_nn,
                                                             const float* __restrict__ face_area, int b0, int F, int P, float* __restrict__ scores) {
    __shared__ double acc[3][RED_THREADS];
    __shared__ int cnt[4];
    const int b = b0 + blockIdx.x, t = threadIdx.x;
    const float* pd = pt_dist + (int64_t)b * P;
    double s = 0.0;
    for (int p = t; p < P; p += RED_THREADS) s += (double)pd[p];
    acc[0][t] = s; acc[1][t] = 0.0; acc[2][t] = 0.0;
    __syncthreads();
    const float* fn = face_nn + (int64_t)b * F;
    const float* fa = face_area + (int64_t)b * F;
    int nvalid = 0;
    for (int f0 = 0; f0 < F; f0 += RED_THREADS) {
        const int f = f0 + t;
        const float a = f < F ? fa[f] : -1.f, m = f < F ? fn[f] : 0.f;
        const bool ok = a >= 0.f;
        int total;
        const int r = block_rank(ok, cnt, total);
        if (ok) {
            const int slot = (nvalid + r) & (RED_THREADS - 1);   // total <= 256: the slots of one pass are distinct
            acc[1][slot] += (double)a * (double)m;
            acc[2][slot] += (double)a;
        }
        nvalid += total;
        __syncthreads();
    }
    for (int o = RED_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j][t] += acc[j][t + o];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double area = acc[2][0];
    float c2m = nvalid > 0 ? (float)(acc[0][0] / (double)P) : INFINITY;
    float m2c = nvalid > 0 && area > 0.0 ? (float)(acc[1][0] / area) : INFINITY;
    float ar = (float)area;
    if (!(c2m == c2m)) c2m = INFINITY;                           // inf - inf and inf * 0 of overflowed coordinates: no NaN leaves
    if (!(m2c == m2c)) m2c = INFINITY;
    if (!(ar == ar)) ar = INFINITY;
    float* o = scores + 4 * (int64_t)b;
    o[0] = c2m; o[1] = m2c; o[2] = ar; o[3] = (float)nvalid;
}

// workspace: pt_dist (B, P) | face_nn (B, F) | face_area (B, F), fp32, each part 256-byte aligned
struct ScoreWs { float* pt_dist; float* face_nn; float* face_area; };

inline size_t score_ws_bytes(int B, int F, int P, ScoreWs* ws = nullptr, void* base = nullptr) {
    const size_t b_pt = wt::align256((size_t)B * P * sizeof(float)), b_face = wt::align256((size_t)B * F * sizeof(float));
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->pt_dist = reinterpret_cast<float*>(p);
        ws->face_nn = reinterpret_cast<float*>(p + b_pt);
        ws->face_area = reinterpret_cast<float*>(p + b_pt + b_face);
    }
    return b_pt + 2 * b_face;
}

inline hipError_t launch_score_meshes(const float* coords, int B, int F, const float* cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale,
                                      float* scores, void* workspace, hipStream_t s) {
    ScoreWs ws;
    score_ws_bytes(B, F, P, &ws, workspace);
    for (int b0 = 0; b0 < B; b0 += MAX_GRID_Y) {
        const unsigned nb = (unsigned)std::min(MAX_GRID_Y, B - b0);
        hipLaunchKernelGGL(cloud_to_mesh_kernel, dim3((unsigned)((P + PT_THREADS - 1) / PT_THREADS), nb), dim3(PT_THREADS), 0, s, coords, b0, F, cloud,
                           cloud_ld, P, n_per_cloud, mesh_scale, ws.pt_dist);
        hipLaunchKernelGGL(mesh_to_cloud_kernel, dim3((unsigned)((F + FACE_THREADS - 1) / FACE_THREADS), nb), dim3(FACE_THREADS), 0, s, coords, b0, F, cloud,
                           cloud_ld, P, n_per_cloud, mesh_scale, ws.face_nn, ws.face_area);
        hipLaunchKernelGGL(reduce_kernel, dim3(nb), dim3(RED_THREADS), 0, s, ws.pt_dist, ws.face_nn, ws.face_area, b0, F, P, scores);
        const hipError_t r = hipGetLastError();
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

}  // namespace score
}  // namespace ma
