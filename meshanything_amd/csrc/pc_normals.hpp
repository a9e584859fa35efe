// Normals for a raw point cloud (`--input_type pc_xyz`).  Has no reference counterpart: the reference takes only
// clouds that already carry unit normals, or meshes.
//
// knn: for Q query points (rows query_idx[q] of ref, or every row when query_idx is NULL) the k nearest of the N rows of ref (N, ref_ld)
// fp32, xyz in the first three columns.  The key of reference row r for query x is
//     d = fl32(fl32(dx*dx + dy*dy) + dz*dz),  dx = fl32(qx - rx), ...      (no FMA contraction; a NaN key, which only non-finite coordinates produce, counts as +inf)
// and neighbours are ordered by the pair (d, r) ascending -- a total order, so the result is one fixed list whatever the launch shape:
// a query is its own neighbour at distance 0, duplicates are ordinary points.
//
// Search: grid (tiles of 256 queries, splits).  One query per thread, its k-best list in registers (knn_list.hpp, shared with the cell-grid
// search of pc_grid.hpp: K = 8, 16 or 32 slots, the smallest
// that holds k; every index is a compile-time constant, so nothing goes to scratch); the split's range of ref passes through LDS in
// tiles of 1024 points, x / y / z apart, read four points at a time as broadcasts.  With one split the lists go straight to the output;
// otherwise every split leaves its K-list in the workspace, [split][slot][query] so that stores and loads coalesce, and the merge
// kernel (again one query per thread) inserts them into one list.  Because the order is total the merged list is the one a single
// split finds, bit for bit.
//
// normals: one query per thread, float64, no FMA contraction.  Centroid c = (sum x) / k and covariance (sum (x - c)(x - c)^T) / k, both
// summed in neighbour-list order; cyclic Jacobi on the 3x3; eigenvalues ascending, the unit eigenvector of the smallest, signed so that
// its component of largest magnitude is positive (lowest axis on ties).  k coincident neighbours: (0, 0, 1) and zero eigenvalues.
// No atomics anywhere: the same inputs give the same bits.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "knn_list.hpp"
#include "watertight.hpp"

namespace ma {
namespace pcn {

constexpr int Q_THREADS = 256;       // queries per workgroup, one per thread
constexpr int REF_TILE = 1024;       // reference points staged per pass: 12 KB of LDS
constexpr int MIN_CHUNK = 256;       // the automatic choice gives a split at least this many reference points ...
constexpr int TARGET_GROUPS = 1024;  // ... and stops splitting at 4 workgroups per CU of a 256-CU part
constexpr int MAX_SPLITS = 64;
static_assert(REF_TILE % Q_THREADS == 0 && REF_TILE % 4 == 0, "the staging loop and the float4 reads");

// splits == 0: enough splits to fill the chip, none shorter than MIN_CHUNK points.  A function of (N, Q) alone, so that the workspace
// size can be asked for without a device.
inline int resolve_splits(int N, int Q, int splits) {
    if (splits > 0) return std::min(splits, N);
    const int tiles = (Q + Q_THREADS - 1) / Q_THREADS;
    const int want = (TARGET_GROUPS + tiles - 1) / tiles;
    const int fit = std::max(1, N / MIN_CHUNK);
    return std::max(1, std::min({want, fit, MAX_SPLITS}));
}

inline size_t knn_ws_bytes(int N, int Q, int k, int splits) {
    const int s = resolve_splits(N, Q, splits);
    return s == 1 ? 256 : 2 * wt::align256((size_t)s * slots_for(k) * Q * sizeof(float));
}

template <int K>
__global__ __launch_bounds__(Q_THREADS) void knn_search_kernel(const float* __restrict__ ref, int N, int ref_ld, const int* __restrict__ query_idx, int Q,
                                                               int k, int chunk, int direct, float* __restrict__ out_d, int* __restrict__ out_i) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float xs[REF_TILE];
    __shared__ __attribute__((aligned(16))) float ys[REF_TILE];
    __shared__ __attribute__((aligned(16))) float zs[REF_TILE];
    const int q = blockIdx.x * Q_THREADS + threadIdx.x;
    const bool live = q < Q;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        int qi = query_idx ? query_idx[q] : q;
        qi = min(max(qi, 0), N - 1);                               // a bad index reads inside ref
        const float* c = ref + (int64_t)qi * ref_ld;
        qx = c[0]; qy = c[1]; qz = c[2];
    }
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
    const int r0 = blockIdx.y * chunk, r1 = min(N, r0 + chunk);
    for (int t0 = r0; t0 < r1; t0 += REF_TILE) {
        const int n = min(REF_TILE, r1 - t0);
        for (int i = threadIdx.x; i < REF_TILE; i += Q_THREADS) {
            float x = INFINITY, y = INFINITY, z = INFINITY;         // past the range: a key of +inf, and the index check below
            if (i < n) {
                const float* c = ref + (int64_t)(t0 + i) * ref_ld;
                x = c[0]; y = c[1]; z = c[2];
            }
            xs[i] = x; ys[i] = y; zs[i] = z;
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < n; i += 4) {
                const float4 X = *reinterpret_cast<const float4*>(xs + i);
                const float4 Y = *reinterpret_cast<const float4*>(ys + i);
                const float4 Z = *reinterpret_cast<const float4*>(zs + i);
                const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = qx - px[j], dy = qy - py[j], dz = qz - pz[j];
                    d[j] = fminf((dx * dx + dy * dy) + dz * dz, INFINITY);   // minNum: a NaN key (non-finite coordinates) becomes +inf
                }
                // one branch per four points: almost always none of them reaches the list
                const float worst = bd[K - 1];
                if (d[0] <= worst || d[1] <= worst || d[2] <= worst || d[3] <= worst) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = t0 + i + j;
                        if (i + j < n && before(d[j], r, bd[K - 1], bi[K - 1])) insert<K>(bd, bi, d[j], r);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (direct) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s < k) { out_d[(int64_t)q * k + s] = bd[s]; out_i[(int64_t)q * k + s] = bi[s]; }
        }
    } else {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const int64_t o = ((int64_t)blockIdx.y * K + s) * Q + q;
            out_d[o] = bd[s]; out_i[o] = bi[s];
        }
    }
}

// one query per thread: the lists of all splits into one.  A split's list is ascending and ends in (inf, INT_MAX) fillers when its
// range had fewer than K points.
template <int K>
__global__ __launch_bounds__(Q_THREADS) void knn_merge_kernel(const float* __restrict__ ws_d, const int* __restrict__ ws_i, int splits, int Q, int k,
                                                              float* __restrict__ nbr_d2, int* __restrict__ nbr_idx) {
    const int q = blockIdx.x * Q_THREADS + threadIdx.x;
    if (q >= Q) return;
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
    for (int sp = 0; sp < splits; ++sp) {
        for (int s = 0; s < K; ++s) {
            const int64_t o = ((int64_t)sp * K + s) * Q + q;
            const float d = ws_d[o];
            const int i = ws_i[o];
            if (!before(d, i, bd[K - 1], bi[K - 1])) break;          // ascending: nothing after it fits either
            insert<K>(bd, bi, d, i);
        }
    }
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s < k) { nbr_d2[(int64_t)q * k + s] = bd[s]; nbr_idx[(int64_t)q * k + s] = bi[s]; }
    }
}

// one Jacobi rotation of the symmetric 3x3 in the plane (p, q); r is the third axis, vp / vq the eigenvector columns p and q
__device__ inline void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&vp)[3], double (&vq)[3]) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // the smaller root: |angle| <= pi / 4
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double p = arp, q = arq;
    arp = c * p - s * q;
    arq = s * p + c * q;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double a = vp[j], b = vq[j];
        vp[j] = c * a - s * b;
        vq[j] = s * a + c * b;
    }
}

constexpr int JACOBI_SWEEPS = 12;    // a 3x3 converges quadratically: 4 to 6 sweeps in practice

// The symmetric 3x3 (a00 a01 a02; a01 a11 a12; a02 a12 a22) by cyclic Jacobi, float64, no FMA contraction: its eigenvalues ascending (the
// lower axis first among equals) and the unit eigenvector of the smallest, signed so that its component of largest magnitude is positive
// (lowest axis on ties).  Shared by normals_kernel and the smoothing kernel of pc_smooth.hpp; non-finite input gives non-finite output.
__device__ inline void smallest_eigenvector(double a00, double a11, double a22, double a01, double a02, double a12, double& l0, double& l1, double& l2,
                                            double& nx, double& ny, double& nz) {
#pragma clang fp contract(off)
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        rotate(a00, a11, a01, a02, a12, v0, v1);                    // (0, 1), third axis 2
        rotate(a00, a22, a02, a01, a12, v0, v2);                    // (0, 2), third axis 1
        rotate(a11, a22, a12, a01, a02, v1, v2);                    // (1, 2), third axis 0
    }
    // ascending, the lower axis first among equals; n = the column of the smallest
    l0 = a00; l1 = a11; l2 = a22;
    nx = v0[0]; ny = v0[1]; nz = v0[2];
    if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; nx = v1[0]; ny = v1[1]; nz = v1[2]; }
    if (l2 < l0) { const double t = l0; l0 = l2; l2 = t; nx = v2[0]; ny = v2[1]; nz = v2[2]; }
    if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx /= len; ny /= len; nz /= len;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const double lead = ax >= ay && ax >= az ? nx : (ay >= az ? ny : nz);
    if (lead < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
}

__global__ __launch_bounds__(Q_THREADS) void normals_kernel(const float* __restrict__ ref, int N, int ref_ld, const int* __restrict__ nbr_idx, int Q,
                                                            int k, double* __restrict__ normals, double* __restrict__ eigvals) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * Q_THREADS + threadIdx.x;
    if (q >= Q) return;
    const int* nb = nbr_idx + (int64_t)q * k;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    bool same = true;
    for (int s = 0; s < k; ++s) {
        const float* c = ref + (int64_t)min(max(nb[s], 0), N - 1) * ref_ld;   // a bad index reads inside ref
        const float x = c[0], y = c[1], z = c[2];
        if (s == 0) { fx = x; fy = y; fz = z; }
        same = same && x == fx && y == fy && z == fz;
        sx += (double)x; sy += (double)y; sz += (double)z;
    }
    const double cx = sx / (double)k, cy = sy / (double)k, cz = sz / (double)k;
    double a00 = 0.0, a11 = 0.0, a22 = 0.0, a01 = 0.0, a02 = 0.0, a12 = 0.0;
    for (int s = 0; s < k; ++s) {
        const float* c = ref + (int64_t)min(max(nb[s], 0), N - 1) * ref_ld;
        const double dx = (double)c[0] - cx, dy = (double)c[1] - cy, dz = (double)c[2] - cz;
        a00 += dx * dx; a11 += dy * dy; a22 += dz * dz;
        a01 += dx * dy; a02 += dx * dz; a12 += dy * dz;
    }
    a00 /= (double)k; a11 /= (double)k; a22 /= (double)k; a01 /= (double)k; a02 /= (double)k; a12 /= (double)k;
    double l0, l1, l2, nx, ny, nz;
    smallest_eigenvector(a00, a11, a22, a01, a02, a12, l0, l1, l2, nx, ny, nz);
    const bool finite = isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(l0) && isfinite(l1) && isfinite(l2);
    if (same || !finite) {                                          // coincident neighbours (or coordinates that overflow): no plane to fit
        nx = 0.0; ny = 0.0; nz = 1.0;
        if (same) { l0 = 0.0; l1 = 0.0; l2 = 0.0; }
    }
    double* on = normals + 3 * (int64_t)q;
    double* oe = eigvals + 3 * (int64_t)q;
    on[0] = nx; on[1] = ny; on[2] = nz;
    oe[0] = l0; oe[1] = l1; oe[2] = l2;
}

template <int K>
inline void launch_knn_k(const float* ref, int N, int ref_ld, const int* query_idx, int Q, int k, int splits, int* nbr_idx, float* nbr_d2, void* workspace,
                         hipStream_t s) {
    const unsigned tiles = (unsigned)((Q + Q_THREADS - 1) / Q_THREADS);
    const int chunk = (N + splits - 1) / splits;
    if (splits == 1) {
        hipLaunchKernelGGL(knn_search_kernel<K>, dim3(tiles, 1), dim3(Q_THREADS), 0, s, ref, N, ref_ld, query_idx, Q, k, chunk, 1, nbr_d2, nbr_idx);
        return;
    }
    float* ws_d = static_cast<float*>(workspace);
    int* ws_i = reinterpret_cast<int*>(static_cast<char*>(workspace) + wt::align256((size_t)splits * K * Q * sizeof(float)));
    hipLaunchKernelGGL(knn_search_kernel<K>, dim3(tiles, (unsigned)splits), dim3(Q_THREADS), 0, s, ref, N, ref_ld, query_idx, Q, k, chunk, 0, ws_d, ws_i);
    hipLaunchKernelGGL(knn_merge_kernel<K>, dim3(tiles), dim3(Q_THREADS), 0, s, ws_d, ws_i, splits, Q, k, nbr_d2, nbr_idx);
}

// splits: already resolved (resolve_splits)
inline hipError_t launch_knn(const float* ref, int N, int ref_ld, const int* query_idx, int Q, int k, int splits, int* nbr_idx, float* nbr_d2,
                             void* workspace, hipStream_t s) {
    switch (slots_for(k)) {
        case 8: launch_knn_k<8>(ref, N, ref_ld, query_idx, Q, k, splits, nbr_idx, nbr_d2, workspace, s); break;
        case 16: launch_knn_k<16>(ref, N, ref_ld, query_idx, Q, k, splits, nbr_idx, nbr_d2, workspace, s); break;
        default: launch_knn_k<32>(ref, N, ref_ld, query_idx, Q, k, splits, nbr_idx, nbr_d2, workspace, s); break;
    }
    return hipGetLastError();
}

inline hipError_t launch_normals(const float* ref, int N, int ref_ld, const int* nbr_idx, int Q, int k, double* normals, double* eigvals, hipStream_t s) {
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((Q + Q_THREADS - 1) / Q_THREADS)), dim3(Q_THREADS), 0, s, ref, N, ref_ld, nbr_idx, Q, k, normals,
                       eigvals);
    return hipGetLastError();
}

}  // namespace pcn
}  // namespace ma
