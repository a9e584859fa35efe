// One iteration of rigid registration (ICP) of a source cloud onto a target cloud over the cell grid of pc_grid.hpp, for `--register_dist`
// (DESIGN.md section 21); PCL's registration module and Open3D's registration_icp do the same job.  Has no reference counterpart.
//
// Build (launch_build): pcg::launch_build bins the target, and the same build bins the source ONCE, in its own untransformed frame, into
// a second pcg::layout region.  The search takes the source's records in that cell order (thread t owns record t), so that a wave's lanes
// are neighbours in space; a rigid motion keeps neighbours neighbours, so the source is never sorted again, whatever the pose.
//
// Step, for a pose (R row-major, t), with r2 = fl32(D * D) computed once on the host and no FMA contraction anywhere:
//   transform:  p'_a = fl32(fl32(fl32(fl32(R_a0 * x) + fl32(R_a1 * y)) + fl32(R_a2 * z)) + t_a)
//   key:        d = fl32(fl32(dx*dx + dy*dy) + dz*dz), dx = fl32(p'_x - q_x), ...: ma_op_pc_knn's, between p' and a target row q
//   pair:       the target row least in (d, index) among the rows with d <= r2 (equality included; a NaN key pairs nothing); none:
//               nn_idx = -1, nn_d2 = +inf.  A total order, so the pair is a function of the clouds, the pose and D alone.
// Guard (count_kernel, bound_kernel): the transformed source is counted into the TARGET's cells, m_c per cell, and sum_c m_c * (target
// rows in the block of R rings around c, clipped to the grid), R = pcr::rings, goes to a 64-bit total that the host reads back and compares
// with max_pairs before the search is launched.  The argument of pc_radius.hpp carries over word for word with "query" = a transformed
// source row: it uses the query's cell and the faces only, not that the query is a record of the grid.  Rows whose p' is not finite
// evaluate no key and are not counted.  pcc::bound_kernel is not touched: its n_c is the gridded cloud's own count.
// Search (search_kernel): the ring and segment walk of pc_grid.hpp (`ring_walk` below: the block grows by one ring per round and only the
// gained cells are visited), started at the cell of p' in the target's grid.  It ends when the block is the whole grid, when there is a
// pair and its key is STRICTLY below fl32(b * b) for every side of the block that is not a grid border (rule (b) of pcg::search_kernel with
// k = 1: every unsearched row has a key >= that bound), or when every such side has fl32(b * b) > r2 (the radius rule of pcc::hook_kernel:
// no unsearched row can have a key <= r2).  Either way the least (d, index) with d <= r2 over ALL target rows has been seen: the result
// does not depend on the grid.  Output per ORIGINAL source row.
// Moments (moments_kernel, reduce_kernel): the order of the records inside a cell comes from the build's atomics, so nothing is summed
// in record order.  One thread takes ROWS_PER_THREAD original rows, recomputes p', the key and the row's terms from nn_idx, and adds them
// in float64 in this FIXED order: workgroup g, thread t adds rows g * GROUP_ROWS + j * 256 + t for j = 0, 1, ..: increasing row; then a
// tree over the 256 lanes in LDS, lane t += lane t + w for w = 128, 64, .., 1; then ONE workgroup adds the workgroups' partials in index
// order, slot s in thread s.  No floating-point atomics: the same inputs give the same 32 doubles for every grid, every workspace
// content and every run.  The longest chain of additions behind a slot is ROWS_PER_THREAD + 8 + the number of workgroups.
//   sums[0] pairs used, [1] sum of (double)d over them, [30] pairs skipped (plane metric: the target's normal is zero or not finite), [31] 0
//   point metric:  [2..4] sum (p' - c), [5..7] sum (q - c), [8..16] sum (p' - c)(q - c)^T row-major; differences in float64 of the float32 values
//   plane metric:  n = normal / sqrt((nx*nx + ny*ny) + nz*nz) in float64, e = (double)p' - (double)q, r = (n_x*e_x + n_y*e_y) + n_z*e_z,
//                  u = (double)p' - (double)c, a = u x n (a_x = u_y*n_z - u_z*n_y and cyclically), J = (a, n);
//                  [2] sum r*r, [3..8] sum J_k * r, [9..29] sum J_k * J_l for k <= l, row-major
//
// Non-finite coordinates through the raw ABI: every read stays inside the records and the cell starts (pc_grid.hpp), row indices read
// from records or nn_idx are range-checked, a source row with a non-finite p' walks nothing and pairs nothing, and its terms are not formed.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"
#include "pc_radius.hpp"

namespace ma {
namespace pcreg {

constexpr int THREADS = pcg::THREADS;
constexpr int ROWS_PER_THREAD = 16;                    // MA_PC_REGISTER_ROWS_PER_THREAD
constexpr int GROUP_ROWS = THREADS * ROWS_PER_THREAD;  // the source rows of one moments workgroup
constexpr int SLOTS = 32;                              // MA_PC_REGISTER_SUMS
constexpr int TREE_SLOTS = 8;                          // slots per pass of the LDS tree: 8 x 256 doubles = 16 KB
static_assert(SLOTS % TREE_SLOTS == 0 && THREADS >= SLOTS, "whole passes; one thread per slot in the last stage");

struct Pose {
    float r[9], t[3];
};

struct Layout {
    size_t source, total, src_count, nn_idx, partials, bytes;
};

inline int moment_groups(int M) { return (M + GROUP_ROWS - 1) / GROUP_ROWS; }

// pcg::layout(N, cells): the target | pcg::layout(M, cells): the source | the 64-bit pair total | the transformed source's count per
// target cell | nn_idx (M), used when the caller passes none | the workgroups' partial sums
inline Layout layout(int N, int M, int cells) {
    Layout l;
    size_t o = pcg::layout(N, cells).bytes;
    l.source = o;    o += pcg::layout(M, cells).bytes;
    l.total = o;     o += wt::align256(sizeof(unsigned long long));
    l.src_count = o; o += wt::align256((size_t)cells * sizeof(int));
    l.nn_idx = o;    o += wt::align256((size_t)M * sizeof(int));
    l.partials = o;  o += wt::align256((size_t)moment_groups(M) * SLOTS * sizeof(double));
    l.bytes = o;
    return l;
}

__device__ inline void transform(const Pose& P, float x, float y, float z, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    px = ((P.r[0] * x + P.r[1] * y) + P.r[2] * z) + P.t[0];
    py = ((P.r[3] * x + P.r[4] * y) + P.r[5] * z) + P.t[1];
    pz = ((P.r[6] * x + P.r[7] * y) + P.r[8] * z) + P.t[2];
}

__device__ inline int cell_id_of(float x, float y, float z, const pcg::Grid& g) {
    const int cx = pcg::cell_of(x, g.ox, g.cell, g.nx), cy = pcg::cell_of(y, g.oy, g.cell, g.ny), cz = pcg::cell_of(z, g.oz, g.cell, g.nz);
    return (cz * g.ny + cy) * g.nx + cx;
}

// The ring and segment walk of pc_grid.hpp for a query that need not be a record of the grid: from cell (cx, cy, cz) the block grows by
// one ring per round, clipped to the grid; visit(p0, p1) gets every range of records the block gained (an x-row that is new as a whole is
// one range, of a row the block had already only the new cell at either end); after a round stop(lx, hx, ly, hy, lz, hz) may end the walk,
// which ends in any case when the block is the whole grid.  N: the number of records, the clamp of every range.
template <class Visit, class Stop>
__device__ inline void ring_walk(const pcg::Grid& g, const int* __restrict__ start, int N, int cx, int cy, int cz, Visit visit, Stop stop) {
    int olx = 0, ohx = -1, oly = 0, ohy = -1, olz = 0, ohz = -1;    // the block of the round before: empty
    for (int r = 0;; ++r) {
        const int lx = max(cx - r, 0), hx = min(cx + r, g.nx - 1);
        const int ly = max(cy - r, 0), hy = min(cy + r, g.ny - 1);
        const int lz = max(cz - r, 0), hz = min(cz + r, g.nz - 1);
        for (int z = lz; z <= hz; ++z) {
            for (int y = ly; y <= hy; ++y) {
                const int row = (z * g.ny + y) * g.nx;
                const bool had = z >= olz && z <= ohz && y >= oly && y <= ohy;   // the block had this row: only its ends are new
                const int a0 = lx, b0 = had ? olx - 1 : hx;
                const int a1 = had ? ohx + 1 : 0, b1 = had ? hx : -1;
                for (int seg = 0; seg < 2; ++seg) {
                    const int a = seg ? a1 : a0, b = seg ? b1 : b0;
                    if (a > b) continue;
                    visit(max(start[row + a], 0), min(start[row + b + 1], N));
                }
            }
        }
        if (lx == 0 && hx == g.nx - 1 && ly == 0 && hy == g.ny - 1 && lz == 0 && hz == g.nz - 1) break;
        if (stop(lx, hx, ly, hy, lz, hz)) break;
        olx = lx; ohx = hx; oly = ly; ohy = hy; olz = lz; ohz = hz;
    }
}

// the transformed source counted into the target's cells
__global__ __launch_bounds__(THREADS) void count_kernel(const float* __restrict__ src, int M, int src_ld, Pose P, pcg::Grid g, int* __restrict__ src_count) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= M) return;
    const float* c = src + (int64_t)i * src_ld;
    float px, py, pz;
    transform(P, c[0], c[1], c[2], px, py, pz);
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return;    // evaluates no key
    atomicAdd(&src_count[cell_id_of(px, py, pz, g)], 1);
}

// sum over the target's cells c of src_count[c] * (target rows in the block of R rings around c): integer atomics, any order, one value
__global__ __launch_bounds__(THREADS) void bound_kernel(const int* __restrict__ start, int N, const int* __restrict__ src_count, int M, pcg::Grid g, int R,
                                                        unsigned long long* __restrict__ total) {
    __shared__ unsigned long long sh[THREADS];
    const int cells = g.nx * g.ny * g.nz;
    const int c = blockIdx.x * THREADS + threadIdx.x;
    unsigned long long mine = 0;
    if (c < cells) {
        const int m = min(max(src_count[c], 0), M);
        if (m > 0) {
            const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
            const int lx = max(cx - R, 0), hx = min(cx + R, g.nx - 1);
            const int ly = max(cy - R, 0), hy = min(cy + R, g.ny - 1);
            const int lz = max(cz - R, 0), hz = min(cz + R, g.nz - 1);
            unsigned long long around = 0;
            for (int z = lz; z <= hz; ++z) {
                for (int y = ly; y <= hy; ++y) {
                    const int row = (z * g.ny + y) * g.nx;
                    around += (unsigned long long)min(max(start[row + hx + 1] - start[row + lx], 0), N);
                }
            }
            mine = (unsigned long long)m * around;
        }
    }
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] != 0) atomicAdd(total, sh[0]);
}

__global__ __launch_bounds__(THREADS) void search_kernel(const float4* __restrict__ tgt_sorted, const int* __restrict__ tgt_start, int N,
                                                         const float4* __restrict__ src_sorted, int M, Pose P, float r2, pcg::Grid g,
                                                         int* __restrict__ nn_idx, float* __restrict__ nn_d2) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= M) return;
    const float4 me = src_sorted[t];
    const int qi = __float_as_int(me.w);
    if (qi < 0 || qi >= M) return;                                  // a record the build did not write: no row to answer for
    float qx, qy, qz;
    transform(P, me.x, me.y, me.z, qx, qy, qz);
    float bd = INFINITY;
    int bi = INT_MAX;
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {             // otherwise every key of this row is NaN or +inf: no pair
        const int cx = pcg::cell_of(qx, g.ox, g.cell, g.nx), cy = pcg::cell_of(qy, g.oy, g.cell, g.ny), cz = pcg::cell_of(qz, g.oz, g.cell, g.nz);
        ring_walk(
            g, tgt_start, N, cx, cy, cz,
            [&](int p0, int p1) {
                for (int p = p0; p < p1; ++p) {
                    const float4 c = tgt_sorted[p];
                    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    const int i = __float_as_int(c.w);
                    if (!(d <= r2) || i < 0 || i >= N) continue;    // a NaN key pairs nothing
                    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
                }
            },
            [&](int lx, int hx, int ly, int hy, int lz, int hz) {
                bool below = bi != INT_MAX, out = true;             // (b): the pair precedes every unsearched row; radius rule: none within r2
                const auto side = [&](float b) { const float bb = b * b; below = below && bd < bb; out = out && bb > r2; };
                if (lx > 0) side(qx - pcg::face(g.ox, g.cell, lx));
                if (hx < g.nx - 1) side(qx - pcg::face(g.ox, g.cell, hx + 1));
                if (ly > 0) side(qy - pcg::face(g.oy, g.cell, ly));
                if (hy < g.ny - 1) side(qy - pcg::face(g.oy, g.cell, hy + 1));
                if (lz > 0) side(qz - pcg::face(g.oz, g.cell, lz));
                if (hz < g.nz - 1) side(qz - pcg::face(g.oz, g.cell, hz + 1));
                return below || out;
            });
    }
    nn_idx[qi] = bi == INT_MAX ? -1 : bi;
    if (nn_d2) nn_d2[qi] = bd;
}

// the terms of one source row added to acc; PLANE: the point-to-plane metric, else point-to-point
template <bool PLANE>
__device__ inline void add_row(double (&acc)[SLOTS], const float* __restrict__ s, const Pose& P, const float* __restrict__ tgt, int N, int tgt_ld,
                               const float* __restrict__ normals, int normals_ld, int j, double cx, double cy, double cz) {
#pragma clang fp contract(off)
    if (j < 0 || j >= N) return;
    float px, py, pz;
    transform(P, s[0], s[1], s[2], px, py, pz);
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return;
    const float* q = tgt + (int64_t)j * tgt_ld;
    const float qx = q[0], qy = q[1], qz = q[2];
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    const double ux = (double)px - cx, uy = (double)py - cy, uz = (double)pz - cz;
    if (PLANE) {
        const float* nf = normals + (int64_t)j * normals_ld;
        const double rx = (double)nf[0], ry = (double)nf[1], rz = (double)nf[2];
        const double len = sqrt((rx * rx + ry * ry) + rz * rz);
        if (!(len > 0.0) || !isfinite(len)) { acc[30] += 1.0; return; }
        const double nx = rx / len, ny = ry / len, nz = rz / len;
        const double ex = (double)px - (double)qx, ey = (double)py - (double)qy, ez = (double)pz - (double)qz;
        const double r = (nx * ex + ny * ey) + nz * ez;
        const double ax = uy * nz - uz * ny, ay = uz * nx - ux * nz, az = ux * ny - uy * nx;
        acc[0] += 1.0;
        acc[1] += (double)d;
        acc[2] += r * r;
        acc[3] += ax * r; acc[4] += ay * r; acc[5] += az * r; acc[6] += nx * r; acc[7] += ny * r; acc[8] += nz * r;
        acc[9] += ax * ax; acc[10] += ax * ay; acc[11] += ax * az; acc[12] += ax * nx; acc[13] += ax * ny; acc[14] += ax * nz;
        acc[15] += ay * ay; acc[16] += ay * az; acc[17] += ay * nx; acc[18] += ay * ny; acc[19] += ay * nz;
        acc[20] += az * az; acc[21] += az * nx; acc[22] += az * ny; acc[23] += az * nz;
        acc[24] += nx * nx; acc[25] += nx * ny; acc[26] += nx * nz;
        acc[27] += ny * ny; acc[28] += ny * nz;
        acc[29] += nz * nz;
    } else {
        const double v[3] = {(double)qx - cx, (double)qy - cy, (double)qz - cz}, u[3] = {ux, uy, uz};
        acc[0] += 1.0;
        acc[1] += (double)d;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[2 + k] += u[k];
            acc[5 + k] += v[k];
#pragma unroll
            for (int l = 0; l < 3; ++l) acc[8 + 3 * k + l] += u[k] * v[l];
        }
    }
}

template <bool PLANE>
__global__ __launch_bounds__(THREADS) void moments_kernel(const float* __restrict__ src, int M, int src_ld, Pose P, const float* __restrict__ tgt, int N,
                                                          int tgt_ld, const float* __restrict__ normals, int normals_ld, const int* __restrict__ nn_idx,
                                                          float c0, float c1, float c2, double* __restrict__ partials) {
    __shared__ double sh[TREE_SLOTS][THREADS];
    double acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) acc[s] = 0.0;
    const double cx = (double)c0, cy = (double)c1, cz = (double)c2;
    const int base = blockIdx.x * GROUP_ROWS + threadIdx.x;
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {                     // increasing row
        const int i = base + j * THREADS;
        if (i < M) add_row<PLANE>(acc, src + (int64_t)i * src_ld, P, tgt, N, tgt_ld, normals, normals_ld, nn_idx[i], cx, cy, cz);
    }
#pragma unroll
    for (int pass = 0; pass < SLOTS / TREE_SLOTS; ++pass) {
#pragma unroll
        for (int k = 0; k < TREE_SLOTS; ++k) sh[k][threadIdx.x] = acc[pass * TREE_SLOTS + k];
        __syncthreads();
        for (int w = THREADS / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
#pragma unroll
                for (int k = 0; k < TREE_SLOTS; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
            }
            __syncthreads();
        }
        if ((int)threadIdx.x < TREE_SLOTS) partials[(int64_t)blockIdx.x * SLOTS + pass * TREE_SLOTS + threadIdx.x] = sh[threadIdx.x][0];
        __syncthreads();
    }
}

// the workgroups' partials in index order, slot s in thread s of the one workgroup
__global__ __launch_bounds__(THREADS) void reduce_kernel(const double* __restrict__ partials, int groups, double* __restrict__ sums) {
    const int s = threadIdx.x;
    if (s >= SLOTS) return;
    double sum = 0.0;
    for (int gi = 0; gi < groups; ++gi) sum += partials[(int64_t)gi * SLOTS + s];
    sums[s] = sum;
}

inline unsigned long long* total_of(int N, int M, const pcg::Grid& g, void* workspace) {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + layout(N, M, pcg::cells_of(g)).total);
}

inline hipError_t launch_build(const float* tgt, int N, int tgt_ld, const float* src, int M, int src_ld, const pcg::Grid& g, void* workspace, hipStream_t s) {
    const hipError_t e = pcg::launch_build(tgt, N, tgt_ld, g, workspace, s);
    if (e != hipSuccess) return e;
    return pcg::launch_build(src, M, src_ld, g, static_cast<char*>(workspace) + layout(N, M, pcg::cells_of(g)).source, s);
}

// the pair bound of this pose into the workspace's total
inline hipError_t launch_bound(const float* src, int M, int src_ld, const Pose& P, int N, const pcg::Grid& g, int R, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const Layout l = layout(N, M, cells);
    char* ws = static_cast<char*>(workspace);
    int* src_count = reinterpret_cast<int*>(ws + l.src_count);
    unsigned long long* total = reinterpret_cast<unsigned long long*>(ws + l.total);
    hipError_t e = hipMemsetAsync(src_count, 0, (size_t)cells * sizeof(int), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(total, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)((M + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, src, M, src_ld, P, g, src_count);
    hipLaunchKernelGGL(bound_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       reinterpret_cast<const int*>(ws + pcg::layout(N, cells).start), N, src_count, M, g, R, total);
    return hipGetLastError();
}

// search, moments and the last sum; nn_idx NULL: the workspace's own array
inline hipError_t launch_step(const float* tgt, int N, int tgt_ld, const float* src, int M, int src_ld, const Pose& P, const float* centre, float r2,
                              const pcg::Grid& g, const float* normals, int normals_ld, int* nn_idx, float* nn_d2, double* sums, void* workspace,
                              hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const Layout l = layout(N, M, cells);
    const pcg::Layout tl = pcg::layout(N, cells), sl = pcg::layout(M, cells);
    char* ws = static_cast<char*>(workspace);
    int* idx = nn_idx ? nn_idx : reinterpret_cast<int*>(ws + l.nn_idx);
    double* partials = reinterpret_cast<double*>(ws + l.partials);
    // a row the search does not answer for (only a workspace that was never built has one) pairs nothing
    hipError_t e = hipMemsetAsync(idx, 0xFF, (size_t)M * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(search_kernel, dim3((unsigned)((M + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, reinterpret_cast<const float4*>(ws + tl.sorted),
                       reinterpret_cast<const int*>(ws + tl.start), N, reinterpret_cast<const float4*>(ws + l.source + sl.sorted), M, P, r2, g, idx, nn_d2);
    if (sums) {
        const int groups = moment_groups(M);
        if (normals)
            hipLaunchKernelGGL(moments_kernel<true>, dim3((unsigned)groups), dim3(THREADS), 0, s, src, M, src_ld, P, tgt, N, tgt_ld, normals, normals_ld, idx,
                               centre[0], centre[1], centre[2], partials);
        else
            hipLaunchKernelGGL(moments_kernel<false>, dim3((unsigned)groups), dim3(THREADS), 0, s, src, M, src_ld, P, tgt, N, tgt_ld, normals, normals_ld, idx,
                               centre[0], centre[1], centre[2], partials);
        hipLaunchKernelGGL(reduce_kernel, dim3(1), dim3(THREADS), 0, s, partials, groups, sums);
    }
    return hipGetLastError();
}

}  // namespace pcreg
}  // namespace ma
