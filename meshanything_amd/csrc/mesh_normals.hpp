// Agreement of a candidate mesh's face normals with the normals of the cloud it was generated from: the normal-consistency term of
// best-of-N sampling and the winding of the written faces.  Has no reference counterpart: the reference
// passes the cloud's normals to the encoder and never looks at them again.
//
// Inputs as in mesh_score.hpp: coords (B, F, 3, 3), a face with any non-finite coordinate is invalid, every vertex is multiplied by
// mesh_scale first (score::load_face); cloud (B / n_per_cloud, P, 6), xyz then the normal, used as given.  Per valid face f, in fp32
// without FMA contraction (every expression below is written out in the kernel, under the pragma), so that a numpy float32 restatement
// gives the same bits:
//   n = (B - A) x (C - A) (wt::cross's expression), l2 = fl(fl(n.x*n.x + n.y*n.y) + n.z*n.z); the face is MEASURABLE when l2 is finite and > 0, then nh = n / sqrtf(l2)
//   q_0..q_6 = the 3 vertices, the midpoints AB, BC, CA and the centroid (mesh_to_cloud_kernel's expressions)
//   j_k = the cloud index that minimises the pair (d, p), d = fl(fl(dx*dx + dy*dy) + dz*dz), dx = fl(q_k.x - x_p): a total order, the
//         lowest index wins ties; the search starts from (+inf, 0) and replaces on strictly less only, so a NaN or +inf key never
//         replaces and j_k is always in 0..P-1
//   t_k = fl(fl(nh.x*m.x + nh.y*m.y) + nh.z*m.z), m = the normal of cloud row j_k
//   a_f = (t_0 + ... + t_6) * fl(1/7)      signed agreement: < 0 = the face is wound against the cloud
//   u_f = (|t_0| + ... + |t_6|) * fl(1/7)  unsigned consistency: independent of the winding
//   area_f = 0.5 * sqrtf(l2): score::mesh_to_cloud_kernel's expression, whose value it equals up to the contraction that kernel is compiled
//   with (a few units in the last place); a face that is not measurable has a_f = u_f = area_f = 0 here (the score kernel turns an
//   overflowed area into +inf) and adds nothing to the sums
// nscores (B, 4): [0] NC = sum area*u / sum area over the measurable faces, [1] the share of that area with a_f < 0, [2] sum area
// (at most FLT_MAX), [3] the number of valid faces; [0] = [1] = 0 without a measurable face.  With a finite cloud no output is NaN
// or infinite.
//
// Two launches.  Search: grid (tiles of FACE_THREADS faces, candidates), one face per thread, its seven (d, index) pairs in registers
// (compile-time indices only: nothing goes to scratch); the cloud's xyz passes through LDS in tiles of CLOUD_TILE points, x / y / z
// apart, read four points at a time as broadcasts; points are visited in index order, so "strictly less" keeps the lowest index.
// The seven normals are gathered from global memory once, after the search.  Reduction: one block per candidate, fp64, the c-th
// valid face into accumulator c mod 256, then one tree -- score::reduce_kernel's order, so NaN rows between valid faces change no
// bit.  No float atomics, nothing depends on B.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mesh_score.hpp"

namespace ma {
namespace mnorm {

using wt::F3;

constexpr int FACE_THREADS = 64;     // faces per workgroup, one per thread
constexpr int CLOUD_TILE = 1024;     // cloud points staged per pass: 12 KB of LDS
constexpr int RED_THREADS = score::RED_THREADS;
constexpr int MAX_GRID_Y = score::MAX_GRID_Y;
static_assert(CLOUD_TILE % FACE_THREADS == 0 && CLOUD_TILE % 4 == 0, "the staging loop and the float4 reads");

// face_agree[b * F + f] = a_f, face_abs = u_f, face_area = the area (-1: invalid face, 0: not measurable), nn_idx[(b * F + f) * 7 + k] = j_k (-1: invalid face)
__global__ __launch_bounds__(FACE_THREADS) void face_normals_kernel(const float* __restrict__ coords, int b0, int F, const float* __restrict__ cloud,
                                                                    int cloud_ld, int P, int n_per_cloud, float scale, float* __restrict__ face_agree,
                                                                    float* __restrict__ face_abs, float* __restrict__ face_area,
                                                                    int* __restrict__ nn_idx) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float xs[CLOUD_TILE];
    __shared__ __attribute__((aligned(16))) float ys[CLOUD_TILE];
    __shared__ __attribute__((aligned(16))) float zs[CLOUD_TILE];
    const int b = b0 + blockIdx.y;
    const int f = blockIdx.x * FACE_THREADS + threadIdx.x;
    const bool live = f < F;
    F3 A = {0.f, 0.f, 0.f}, B = A, C = A;
    const bool ok = live && score::load_face(coords + ((int64_t)b * F + f) * 9, scale, A, B, C);
    const F3 q[7] = {A, B, C,
                     {0.5f * (A.x + B.x), 0.5f * (A.y + B.y), 0.5f * (A.z + B.z)},
                     {0.5f * (B.x + C.x), 0.5f * (B.y + C.y), 0.5f * (B.z + C.z)},
                     {0.5f * (C.x + A.x), 0.5f * (C.y + A.y), 0.5f * (C.z + A.z)},
                     {(A.x + B.x + C.x) * (1.0f / 3.0f), (A.y + B.y + C.y) * (1.0f / 3.0f), (A.z + B.z + C.z) * (1.0f / 3.0f)}};
    float bd[7];
    int bi[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { bd[k] = INFINITY; bi[k] = 0; }
    const float* cb = cloud + (int64_t)(b / n_per_cloud) * P * cloud_ld;
    for (int p0 = 0; p0 < P; p0 += CLOUD_TILE) {
        const int n = min(CLOUD_TILE, P - p0);
        for (int i = threadIdx.x; i < CLOUD_TILE; i += FACE_THREADS) {
            float x = INFINITY, y = INFINITY, z = INFINITY;         // past the cloud: a key of +inf, which never replaces
            if (i < n) {
                const float* c = cb + (int64_t)(p0 + i) * cloud_ld;
                x = c[0]; y = c[1]; z = c[2];
            }
            xs[i] = x; ys[i] = y; zs[i] = z;
        }
        __syncthreads();
        if (ok) {
            for (int i = 0; i < n; i += 4) {
                const float4 X = *reinterpret_cast<const float4*>(xs + i);
                const float4 Y = *reinterpret_cast<const float4*>(ys + i);
                const float4 Z = *reinterpret_cast<const float4*>(zs + i);
                const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int p = p0 + i + j;
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        const float dx = q[k].x - px[j], dy = q[k].y - py[j], dz = q[k].z - pz[j];
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        const bool lt = d < bd[k];                  // false for NaN and for +inf against +inf
                        bd[k] = lt ? d : bd[k];
                        bi[k] = lt ? p : bi[k];
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const int64_t o = (int64_t)b * F + f;
    float agree = 0.f, uns = 0.f, area = ok ? 0.f : -1.f;
    if (ok) {
        // wt::cross and wt::dot written out: inlined helpers keep the default contraction, here every product and sum rounds on its own
        const F3 e1 = wt::sub(B, A), e2 = wt::sub(C, A);
        const F3 n = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
        const float l2 = (n.x * n.x + n.y * n.y) + n.z * n.z;
        if (l2 > 0.f && l2 < INFINITY) {
            const float len = sqrtf(l2);
            area = 0.5f * len;
            const float nx = n.x / len, ny = n.y / len, nz = n.z / len;
            float s = 0.f, sa = 0.f;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const float* m = cb + (int64_t)bi[k] * cloud_ld + 3;
                const float t = (nx * m[0] + ny * m[1]) + nz * m[2];
                s = s + t;
                sa = sa + fabsf(t);
            }
            agree = s * (1.0f / 7.0f);
            uns = sa * (1.0f / 7.0f);
        }
    }
    face_agree[o] = agree;
    face_abs[o] = uns;
    face_area[o] = area;
#pragma unroll
    for (int k = 0; k < 7; ++k) nn_idx[o * 7 + k] = ok ? bi[k] : -1;
}

// one block per candidate.  The valid faces are numbered in face order and face number c goes to accumulator c mod 256, in increasing
// c; then one fixed tree over the 256 accumulators (score::reduce_kernel's order).  acc: area * u | area where a_f < 0 | area.
__global__ __launch_bounds__(RED_THREADS) void reduce_normals_kernel(const float* __restrict__ face_agree, const float* __restrict__ face_abs,
                                                                     const float* __restrict__ face_area, int b0, int F, float* __restrict__ nscores) {
    __shared__ double acc[3][RED_THREADS];
    __shared__ int cnt[4];
    const int b = b0 + blockIdx.x, t = threadIdx.x;
    acc[0][t] = 0.0; acc[1][t] = 0.0; acc[2][t] = 0.0;
    __syncthreads();
    const float* fg = face_agree + (int64_t)b * F;
    const float* fu = face_abs + (int64_t)b * F;
    const float* fa = face_area + (int64_t)b * F;
    int nvalid = 0;
    for (int f0 = 0; f0 < F; f0 += RED_THREADS) {
        const int f = f0 + t;
        const float a = f < F ? fa[f] : -1.f, u = f < F ? fu[f] : 0.f, g = f < F ? fg[f] : 0.f;
        const bool ok = a >= 0.f;
        int total;
        const int r = score::block_rank(ok, cnt, total);
        if (ok && a > 0.f) {                                         // measurable: l2 finite and > 0
            const int slot = (nvalid + r) & (RED_THREADS - 1);       // total <= 256: the slots of one pass are distinct
            acc[0][slot] += (double)a * (double)u;
            acc[1][slot] += g < 0.f ? (double)a : 0.0;
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
    float* o = nscores + 4 * (int64_t)b;
    o[0] = area > 0.0 ? (float)(acc[0][0] / area) : 0.f;
    o[1] = area > 0.0 ? (float)(acc[1][0] / area) : 0.f;
    o[2] = (float)fmin(area, (double)FLT_MAX);
    o[3] = (float)nvalid;
}

// workspace: face_abs (B, F) fp32 | face_area (B, F) fp32, -1 = invalid, 0 = not measurable | nn_idx (B, F, 7) int32, each part 256-byte aligned
struct NormalsWs { float* face_abs; float* face_area; int* nn_idx; };

inline size_t normals_ws_bytes(int B, int F, NormalsWs* ws = nullptr, void* base = nullptr) {
    const size_t b_face = wt::align256((size_t)B * F * sizeof(float)), b_idx = wt::align256((size_t)B * F * 7 * sizeof(int));
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->face_abs = reinterpret_cast<float*>(p);
        ws->face_area = reinterpret_cast<float*>(p + b_face);
        ws->nn_idx = reinterpret_cast<int*>(p + 2 * b_face);
    }
    return 2 * b_face + b_idx;
}

inline hipError_t launch_mesh_normals(const float* coords, int B, int F, const float* cloud, int cloud_ld, int P, int n_per_cloud, float mesh_scale,
                                      float* face_agree, float* nscores, void* workspace, hipStream_t s) {
    NormalsWs ws;
    normals_ws_bytes(B, F, &ws, workspace);
    for (int b0 = 0; b0 < B; b0 += MAX_GRID_Y) {
        const unsigned nb = (unsigned)std::min(MAX_GRID_Y, B - b0);
        hipLaunchKernelGGL(face_normals_kernel, dim3((unsigned)((F + FACE_THREADS - 1) / FACE_THREADS), nb), dim3(FACE_THREADS), 0, s, coords, b0, F, cloud,
                           cloud_ld, P, n_per_cloud, mesh_scale, face_agree, ws.face_abs, ws.face_area, ws.nn_idx);
        hipLaunchKernelGGL(reduce_normals_kernel, dim3(nb), dim3(RED_THREADS), 0, s, face_agree, ws.face_abs, ws.face_area, b0, F, nscores);
        const hipError_t r = hipGetLastError();
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

}  // namespace mnorm
}  // namespace ma
