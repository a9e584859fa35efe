// Fit of a generated mesh to the cloud it was generated from (--fit_iters): the pairing of every cloud point with
// its nearest admissible face and the per-face sums of the point-to-plane normal equations.  The host (meshanything_amd/mesh_fit.py)
// assembles and solves the small vertex system in float64.  Has no reference counterpart: the reference never moves a vertex.
//
// Inputs: verts (V, 3) fp32 in CLOUD units (the caller has multiplied by mesh_scale), faces (M, 3) int32 into them, cloud (P, 6) fp32,
// xyz then the normal m.  Everything below is fp32 without FMA contraction (`#pragma clang fp contract(off)` in every function), with
// IEEE division and square root, every operation rounding on its own in the order written, so that tests/mesh_fit_ref.py restates it
// in numpy float32 bit for bit.  dot(u, v) = fl(fl(u.x*v.x + u.y*v.y) + u.z*v.z), cross(u, v) = (u.y*v.z - u.z*v.y, ...).
//
// Per face, once per workgroup while staging (prep_face):
//   e0 = B - A, e1 = C - B, e2 = A - C, l_i = dot(e_i, e_i); n = the cross product of the two shorter edges (wt::tri_dist's choice),
//   n2 = dot(n, n), fp = flat * ((sqrtf(l0) + sqrtf(l1)) + sqrtf(l2)).  The face is ADMISSIBLE when its three indices are in range and
//   differ, its nine coordinates are finite and n2 > fp * fp (inradius above `flat`: tri_dist's rule); then nh = n / sqrtf(n2).
// Per point p with normal m, dot(m, m) > 0, over the admissible faces in ascending index (pair_face):
//   min_cos > 0 and |dot(nh, m)| < min_cos: the face is skipped.
//   a = A - p, b = B - p, c = C - p.  Edge i from vertex v: t = l_i > 0 ? -dot(v, e_i) / l_i : 0, clamped to [0, 1], q = v + t * e_i,
//   d = dot(q, q); the edge with the least d wins, the lowest on ties.
//   s0 = dot(cross(a, e0), nh), s1 = dot(cross(b, e1), nh), s2 = dot(cross(c, e2), nh), S = (s0 + s1) + s2.  INSIDE when s0, s1, s2 >= 0
//   and S > 0: w = (s1 / S, s2 / S, s0 / S), r = -((w0 * a + w1 * b) + w2 * c), d2 = dot(r, r).  Otherwise the winning edge: w = (1 - t, t,
//   0) on AB, (0, 1 - t, t) on BC, (t, 0, 1 - t) on CA, r = -q, d2 = d.
//   The face replaces the best so far when d2 < best (strict: the lowest face index wins ties; a NaN never wins).
//   The point is PAIRED when a face was found and d2 <= dist * dist; then s = dot(m, r).
// Outputs per point: pt_face (-1 = unpaired), pt_w (3 weights), and in the workspace pt_s and pt_r2 (= d2); 0 for an unpaired point.
//
// Per face f, over its paired points (sum pass), NSUM = 48 int64 values: [0] the count; then in 2^-32 fixed point, every fp32 term
// converted to double, multiplied by 2^32 and rounded half to even: [1] sum fl(s*s), [2] sum d2, [3 + 3k + a] g[k][a] = sum
// fl(fl(w_k*s)*m_a), [12 + 6*kl + ac] H[kl][ac] = sum fl(fl(w_k*w_l)*fl(m_a*m_c)), kl in (00, 01, 02, 11, 12, 22), ac in (xx, xy, xz,
// yy, yz, zz).  Integer sums do not depend on their order: the same bits on every run and for every launch shape.
//
// Two launches.  Pair: one point per thread, 256 per workgroup, the faces pass through LDS in tiles of FACE_TILE, inadmissible ones
// dropped while staging (score::cloud_to_mesh_kernel's scheme), every lane then reads the same face (a broadcast).  Sum: grid (faces,
// chunks of SUM_CHUNK points): a workgroup scans its chunk of pt_face, a thread that meets its face adds the point's 48 terms to
// int64 registers; then a wave reduction by shuffles, the four waves through LDS, and 48 integer atomics per workgroup into face_sums
// (zeroed first).  No floating-point atomics anywhere.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "mesh_score.hpp"

namespace ma {
namespace fit {

using wt::F3;

constexpr int PT_THREADS = 256;      // pair pass: points per workgroup, one per thread
constexpr int FACE_TILE = 256;       // ... and faces staged per pass: 13 dwords each, 13 KB of LDS
constexpr int FACE_DW = 13;          // A, B, C, nh, the face index (as bits)
constexpr int SUM_THREADS = 256;     // sum pass
constexpr int SUM_CHUNK = 1 << 18;   // points per workgroup of the sum pass
constexpr int NSUM = 48;
constexpr int ST_FACE_INDEX = 1, ST_VERT_NONFINITE = 2, ST_CLOUD_NONFINITE = 4;   // bits of the status word
static_assert(FACE_TILE == PT_THREADS && PT_THREADS == 256, "score::block_rank and the staging assume 256 threads");

__device__ inline float dot3(F3 u, F3 v) {
#pragma clang fp contract(off)
    return (u.x * v.x + u.y * v.y) + u.z * v.z;
}
__device__ inline F3 cross3(F3 u, F3 v) {
#pragma clang fp contract(off)
    return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ inline F3 sub3(F3 u, F3 v) {
#pragma clang fp contract(off)
    return {u.x - v.x, u.y - v.y, u.z - v.z};
}

// the point-independent part of a face: admissible or not, and its unit normal
__device__ inline bool prep_face(F3 A, F3 B, F3 C, float flat, F3& nh) {
#pragma clang fp contract(off)
    const F3 e0 = sub3(B, A), e1 = sub3(C, B), e2 = sub3(A, C);
    const float l0 = dot3(e0, e0), l1 = dot3(e1, e1), l2 = dot3(e2, e2);
    const F3 n = (l0 >= l1 && l0 >= l2) ? cross3(e1, e2) : (l1 >= l2 ? cross3(e2, e0) : cross3(e0, e1));
    const float n2 = dot3(n, n);
    const float fp = flat * ((sqrtf(l0) + sqrtf(l1)) + sqrtf(l2));
    if (!(n2 > fp * fp) || !(n2 < INFINITY)) return false;
    const float len = sqrtf(n2);
    nh = {n.x / len, n.y / len, n.z / len};
    return true;
}

// edge from vertex v (relative to the point) along e: the squared distance d of its nearest point q = v + t * e, and t
__device__ inline float edge_near(F3 v, F3 e, float& t, F3& q) {
#pragma clang fp contract(off)
    const float l = dot3(e, e);
    float u = l > 0.f ? -dot3(v, e) / l : 0.f;
    u = fminf(fmaxf(u, 0.f), 1.f);
    t = u;
    q = {v.x + u * e.x, v.y + u * e.y, v.z + u * e.z};
    return dot3(q, q);
}

// the point of face A, B, C nearest to p: its weights w, r = p - that point, and the squared distance
__device__ inline float pair_face(F3 A, F3 B, F3 C, F3 nh, F3 p, F3& w, F3& r) {
#pragma clang fp contract(off)
    const F3 e0 = sub3(B, A), e1 = sub3(C, B), e2 = sub3(A, C);
    const F3 a = sub3(A, p), b = sub3(B, p), c = sub3(C, p);
    const float s0 = dot3(cross3(a, e0), nh), s1 = dot3(cross3(b, e1), nh), s2 = dot3(cross3(c, e2), nh);
    const float S = (s0 + s1) + s2;
    if (s0 >= 0.f && s1 >= 0.f && s2 >= 0.f && S > 0.f) {
        w = {s1 / S, s2 / S, s0 / S};
        r = {-((w.x * a.x + w.y * b.x) + w.z * c.x), -((w.x * a.y + w.y * b.y) + w.z * c.y), -((w.x * a.z + w.y * b.z) + w.z * c.z)};
        return dot3(r, r);
    }
    float t0, t1, t2;
    F3 q0, q1, q2;
    const float d0 = edge_near(a, e0, t0, q0), d1 = edge_near(b, e1, t1, q1), d2 = edge_near(c, e2, t2, q2);
    float d = d0;
    F3 q = q0;
    w = {1.0f - t0, t0, 0.f};
    if (d1 < d) { d = d1; q = q1; w = {0.f, 1.0f - t1, t1}; }
    if (d2 < d) { d = d2; q = q2; w = {t2, 0.f, 1.0f - t2}; }
    r = {-q.x, -q.y, -q.z};
    return d;
}

// grid: tiles of PT_THREADS points.  status: bits ST_* are set (an integer atomic) where the input breaks the caller's promises; such a
// face is inadmissible and such a point unpaired, so the kernel stays in bounds and NaN-free whatever it is given.
__global__ __launch_bounds__(PT_THREADS) void pair_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int M,
                                                          const float* __restrict__ cloud, int cloud_ld, int P, float dist2, float min_cos, float flat,
                                                          int* __restrict__ pt_face, float* __restrict__ pt_w, float* __restrict__ pt_s,
                                                          float* __restrict__ pt_r2, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ float tri[FACE_TILE * FACE_DW];
    __shared__ int cnt[4];
    const int p = blockIdx.x * PT_THREADS + threadIdx.x;
    bool live = p < P;
    F3 q = {0.f, 0.f, 0.f}, m = {0.f, 0.f, 0.f};
    int bad = 0;
    if (live) {
        const float* c = cloud + (int64_t)p * cloud_ld;
        q = {c[0], c[1], c[2]};
        m = {c[3], c[4], c[5]};
        if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(m.x) && isfinite(m.y) && isfinite(m.z))) { bad |= ST_CLOUD_NONFINITE; live = false; }
        else if (!(dot3(m, m) > 0.f)) live = false;                  // a zero normal pairs with nothing
    }
    float best = INFINITY, bs = 0.f;
    int bf = -1;
    F3 bw = {0.f, 0.f, 0.f};
    for (int f0 = 0; f0 < M; f0 += FACE_TILE) {
        const int f = f0 + threadIdx.x;
        F3 A = {0.f, 0.f, 0.f}, B = A, C = A, nh = A;
        bool ok = false;
        if (f < M) {
            const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
            if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) bad |= ST_FACE_INDEX;
            else {
                const float* va = verts + 3 * (int64_t)i0;
                const float* vb = verts + 3 * (int64_t)i1;
                const float* vc = verts + 3 * (int64_t)i2;
                A = {va[0], va[1], va[2]}; B = {vb[0], vb[1], vb[2]}; C = {vc[0], vc[1], vc[2]};
                const bool fin = isfinite(A.x) && isfinite(A.y) && isfinite(A.z) && isfinite(B.x) && isfinite(B.y) && isfinite(B.z) && isfinite(C.x) &&
                                 isfinite(C.y) && isfinite(C.z);
                if (!fin) bad |= ST_VERT_NONFINITE;
                else ok = i0 != i1 && i1 != i2 && i0 != i2 && prep_face(A, B, C, flat, nh);
            }
        }
        int total;
        const int rk = score::block_rank(ok, cnt, total);
        if (ok) {
            float* t = tri + rk * FACE_DW;                           // stride 13 dwords: no bank conflict
            t[0] = A.x; t[1] = A.y; t[2] = A.z; t[3] = B.x; t[4] = B.y; t[5] = B.z; t[6] = C.x; t[7] = C.y; t[8] = C.z;
            t[9] = nh.x; t[10] = nh.y; t[11] = nh.z; t[12] = __int_as_float(f);
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < total; ++i) {
                const float* t = tri + i * FACE_DW;
                const F3 nh2 = {t[9], t[10], t[11]};
                if (min_cos > 0.f && fabsf(dot3(nh2, m)) < min_cos) continue;
                F3 w, r;
                const float d2 = pair_face(F3{t[0], t[1], t[2]}, F3{t[3], t[4], t[5]}, F3{t[6], t[7], t[8]}, nh2, q, w, r);
                if (d2 < best) { best = d2; bf = __float_as_int(t[12]); bw = w; bs = dot3(m, r); }
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(status, bad);
    if (p >= P) return;
    const bool paired = live && bf >= 0 && best <= dist2;
    pt_face[p] = paired ? bf : -1;
    pt_w[3 * (int64_t)p] = paired ? bw.x : 0.f;
    pt_w[3 * (int64_t)p + 1] = paired ? bw.y : 0.f;
    pt_w[3 * (int64_t)p + 2] = paired ? bw.z : 0.f;
    pt_s[p] = paired ? bs : 0.f;
    pt_r2[p] = paired ? best : 0.f;
}

__device__ inline long long fixed32(float x) { return __double2ll_rn((double)x * 4294967296.0); }

// grid (M faces, chunks of SUM_CHUNK points); face_sums (M, NSUM) int64, zeroed before the launch
__global__ __launch_bounds__(SUM_THREADS) void sum_kernel(const int* __restrict__ pt_face, const float* __restrict__ pt_w, const float* __restrict__ pt_s,
                                                          const float* __restrict__ pt_r2, const float* __restrict__ cloud, int cloud_ld, int P,
                                                          unsigned long long* __restrict__ face_sums) {
#pragma clang fp contract(off)
    __shared__ unsigned long long part[NSUM];
    const int f = blockIdx.x;
    const int p0 = blockIdx.y * SUM_CHUNK, p1 = min(P, p0 + SUM_CHUNK);
    long long acc[NSUM];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0;
    if (threadIdx.x < NSUM) part[threadIdx.x] = 0ull;
    for (int p = p0 + threadIdx.x; p < p1; p += SUM_THREADS) {
        if (pt_face[p] != f) continue;
        const float w[3] = {pt_w[3 * (int64_t)p], pt_w[3 * (int64_t)p + 1], pt_w[3 * (int64_t)p + 2]};
        const float* c = cloud + (int64_t)p * cloud_ld;
        const float m[3] = {c[3], c[4], c[5]};
        const float s = pt_s[p];
        acc[0] += 1;
        acc[1] += fixed32(s * s);
        acc[2] += fixed32(pt_r2[p]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ws = w[k] * s;
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[3 + 3 * k + a] += fixed32(ws * m[a]);
        }
        const float mm[6] = {m[0] * m[0], m[0] * m[1], m[0] * m[2], m[1] * m[1], m[1] * m[2], m[2] * m[2]};
        const float ww[6] = {w[0] * w[0], w[0] * w[1], w[0] * w[2], w[1] * w[1], w[1] * w[2], w[2] * w[2]};
#pragma unroll
        for (int kl = 0; kl < 6; ++kl) {
#pragma unroll
            for (int ac = 0; ac < 6; ++ac) acc[12 + 6 * kl + ac] += fixed32(ww[kl] * mm[ac]);
        }
    }
    if (!__syncthreads_or(acc[0] != 0)) return;                      // (also the barrier after part[] = 0)
#pragma unroll
    for (int j = 0; j < NSUM; ++j) {
        long long v = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(&part[j], (unsigned long long)v);   // LDS, integer
    }
    __syncthreads();
    if (threadIdx.x < NSUM && part[threadIdx.x] != 0ull) atomicAdd(&face_sums[(int64_t)f * NSUM + threadIdx.x], part[threadIdx.x]);
}

// workspace: pt_s (P) fp32 | pt_r2 (P) fp32 | the status word (int32, 256 bytes reserved), each part 256-byte aligned
struct FitWs { float* pt_s; float* pt_r2; int* status; };

inline size_t fit_ws_bytes(int P, FitWs* ws = nullptr, void* base = nullptr) {
    const size_t b_pt = wt::align256((size_t)P * sizeof(float));
    if (ws) {
        char* p = static_cast<char*>(base);
        ws->pt_s = reinterpret_cast<float*>(p);
        ws->pt_r2 = reinterpret_cast<float*>(p + b_pt);
        ws->status = reinterpret_cast<int*>(p + 2 * b_pt);
    }
    return 2 * b_pt + 256;
}

inline hipError_t launch_mesh_fit_pairs(const float* verts, int V, const int* faces, int M, const float* cloud, int cloud_ld, int P, float dist, float min_cos,
                                        float flat, int* pt_face, float* pt_w, int64_t* face_sums, void* workspace, hipStream_t s) {
    FitWs ws;
    fit_ws_bytes(P, &ws, workspace);
    hipError_t r = hipMemsetAsync(ws.status, 0, sizeof(int), s);
    if (r != hipSuccess) return r;
    r = hipMemsetAsync(face_sums, 0, (size_t)M * NSUM * sizeof(int64_t), s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(pair_kernel, dim3((unsigned)((P + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, s, verts, V, faces, M, cloud, cloud_ld, P,
                       dist * dist, min_cos, flat, pt_face, pt_w, ws.pt_s, ws.pt_r2, ws.status);
    hipLaunchKernelGGL(sum_kernel, dim3((unsigned)M, (unsigned)((P + SUM_CHUNK - 1) / SUM_CHUNK)), dim3(SUM_THREADS), 0, s, pt_face, pt_w, ws.pt_s, ws.pt_r2,
                       cloud, cloud_ld, P, reinterpret_cast<unsigned long long*>(face_sums));
    return hipGetLastError();
}

}  // namespace fit
}  // namespace ma
