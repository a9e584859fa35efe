// The k nearest neighbours of EVERY point of a cloud over a uniform cell grid, for statistical outlier removal (`--outlier_k`; DESIGN.md
// section 14).  Has no reference counterpart.  The lists are ma_op_pc_knn's (pc_normals.hpp), bit for bit: the same key
//     d = fl32(fl32(dx*dx + dy*dy) + dz*dz),  dx = fl32(qx - rx), ...      (no FMA contraction; a NaN key counts as +inf)
// and the same total order (d, index).  The k best under a total order are unique, so they do not depend on the order in which the
// points are visited, and therefore not on the grid.
//
// The grid: origin[3], cell > 0, dims[3] (each 1 .. 128, product <= 2^21).  Per axis face[i] = fl32(origin + fl32(i * cell)), i = 0 .. dim,
// non-decreasing because both roundings are monotone.  The cell of a coordinate x is the largest i in [0, dim - 1] with i = 0 or
// face[i] <= x: a binary search over the faces, comparisons alone (no division whose rounding could disagree with the faces the stop
// rule below uses).  So the border cells are unbounded outward, a point outside the box belongs to the nearest border cell, and a NaN
// goes to cell 0.  Cell id = (cz * ny + cy) * nx + cx: the cells of one x-row are neighbours in memory.
//
// Build: (memset of the counts) -> count_kernel: cell id per point, atomicAdd on its cell's count -> tile_sum_kernel + scan_kernel: the
// exclusive scan of the counts, tiles of 2048 cells, each workgroup adding the sums of the tiles before its own (two launches, no
// workgroup waits for another) -> scatter_kernel: (x, y, z, original index) as one 16-byte record per point into cell order, the place
// inside the cell from an atomicAdd on the cell's cursor.  The order inside a cell is whatever the atomics give; no output depends on it.
//
// Search: one query per thread, 256 per workgroup, queries taken in cell order (thread t owns record t), so that a wave's lanes walk
// the same cells.  The query's block of cells starts at its own cell and grows by one ring per round, clipped to the grid; a round
// visits only the cells the block gained.  Of an x-row that is new as a whole the points are one contiguous range of records; of a row
// the block had already, the one new cell at either end.  After a round the search of that query ends when
//   (a) the block is the whole grid, or
//   (b) the list is full and its k-th key is STRICTLY below the bound of the block: the minimum, over the block's sides that are not
//       grid borders, of fl32(b * b), b = fl32(q_axis - face_of_that_side).
// Why (b) is exact, with no slack.  Take a point r outside the block; on some axis its cell lies beyond a side of the block that is not
// a grid border, say above the high side hi < dim - 1, whose face is f = face[hi + 1].  By the cell rule f <= face[cell(r)] <= r, and
// q < f because q's own cell is <= hi (the rule again: face[cell(q) + 1] > q).  So r - q >= f - q > 0 in exact arithmetic, rounding is
// monotone, hence |fl32(q - r)| >= |fl32(q - f)| = |b| and fl32(dx * dx) >= fl32(b * b).  Every later step of the key adds a
// non-negative term and rounds monotonically, so the key of r is >= fl32(b * b) >= the bound.  (The low side is the mirror image: r <
// face[lo] <= q.)  A k-th key strictly below the bound therefore precedes every unsearched point in the order (d, index).  The strict
// inequality keeps out the one case the bound does not cover: an unsearched point of EQUAL key and lower index.
// Non-finite coordinates: b or the k-th key is NaN or inf, (b) may never hold, and the search ends by (a) after at most 127 rounds; every
// read stays inside the records and the cell starts, which the scan makes consistent with the counts whatever the coordinates are.
//
// Outputs, each optional: nbr_idx / nbr_d2 (N, k) in the ORIGINAL row order, and mean_dist (N) float64 = (sum_j sqrt((double) d_j)) / k
// in list order, no contraction, the point itself included at distance 0.  With mean_dist alone the lists never leave the registers.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "knn_list.hpp"
#include "watertight.hpp"

namespace ma {
namespace pcg {

constexpr int THREADS = 256;         // points (build) or queries (search) per workgroup, one per thread
constexpr int MAX_DIM = 128;
constexpr int MAX_CELLS = 1 << 21;
constexpr int MAX_POINTS = 1 << 22;
constexpr int SCAN_TILE = 2048;      // cells per workgroup of the scan: 8 per thread
constexpr int SCAN_PER_THREAD = SCAN_TILE / THREADS;
constexpr int MAX_TILES = MAX_CELLS / SCAN_TILE;
static_assert(SCAN_TILE % THREADS == 0 && MAX_CELLS % SCAN_TILE == 0, "whole tiles, eight cells per thread");

struct Grid {
    float ox, oy, oz, cell;
    int nx, ny, nz;
};

inline int cells_of(const Grid& g) { return g.nx * g.ny * g.nz; }

struct Layout {
    size_t cell_id, cursor, start, tile_sum, sorted, bytes;
};

// cell_id (N) int32 | cursor (cells) int32: the counts, then each cell's next free record | start (cells + 1) int32 | tile_sum | records
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = 0;
    l.cell_id = o;  o += wt::align256((size_t)N * sizeof(int));
    l.cursor = o;   o += wt::align256((size_t)cells * sizeof(int));
    l.start = o;    o += wt::align256(((size_t)cells + 1) * sizeof(int));
    l.tile_sum = o; o += wt::align256((size_t)MAX_TILES * sizeof(int));
    l.sorted = o;   o += wt::align256((size_t)N * sizeof(float4));
    l.bytes = o;
    return l;
}

__device__ inline float face(float origin, float cell, int i) {
#pragma clang fp contract(off)
    const float step = (float)i * cell;
    return origin + step;
}

// the largest i in [0, dim - 1] with i = 0 or face[i] <= x; a NaN fails every comparison and ends at 0
__device__ inline int cell_of(float x, float origin, float cell, int dim) {
    int lo = 0, hi = dim - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (face(origin, cell, mid) <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(THREADS) void count_kernel(const float* __restrict__ ref, int N, int ref_ld, Grid g, int* __restrict__ cell_id,
                                                        int* __restrict__ counts) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= N) return;
    const float* c = ref + (int64_t)p * ref_ld;
    const int cx = cell_of(c[0], g.ox, g.cell, g.nx), cy = cell_of(c[1], g.oy, g.cell, g.ny), cz = cell_of(c[2], g.oz, g.cell, g.nz);
    const int id = (cz * g.ny + cy) * g.nx + cx;
    cell_id[p] = id;
    atomicAdd(&counts[id], 1);
}

// the sum of the 256 values v, one per thread, in every thread
__device__ inline int block_sum(int v, int* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const int total = sh[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(THREADS) void tile_sum_kernel(const int* __restrict__ counts, int cells, int* __restrict__ tile_sum) {
    __shared__ int sh[THREADS];
    const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
    int v = 0;
    for (int j = 0; j < SCAN_PER_THREAD; ++j) v += base + j < cells ? counts[base + j] : 0;
    const int total = block_sum(v, sh);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// counts (cells) -> start (cells + 1), the exclusive scan with start[cells] = N, and in place the cursors, a copy of start[0 .. cells)
__global__ __launch_bounds__(THREADS) void scan_kernel(int* __restrict__ counts, int cells, const int* __restrict__ tile_sum, int N, int* __restrict__ start) {
    __shared__ int sh[THREADS];
    int before = 0;
    for (int t = threadIdx.x; t < (int)blockIdx.x; t += THREADS) before += tile_sum[t];
    const int tile_base = block_sum(before, sh);
    const int base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
    int c[SCAN_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        c[j] = base + j < cells ? counts[base + j] : 0;
        mine += c[j];
    }
    // inclusive scan of the 256 thread sums
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int w = 1; w < THREADS; w <<= 1) {
        const int add = (int)threadIdx.x >= w ? sh[threadIdx.x - w] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    int run = tile_base + sh[threadIdx.x] - mine;
#pragma unroll
    for (int j = 0; j < SCAN_PER_THREAD; ++j) {
        if (base + j < cells) { start[base + j] = run; counts[base + j] = run; }
        run += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) start[cells] = N;
}

__global__ __launch_bounds__(THREADS) void scatter_kernel(const float* __restrict__ ref, int N, int ref_ld, const int* __restrict__ cell_id,
                                                          int* __restrict__ cursor, float4* __restrict__ sorted) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= N) return;
    const float* c = ref + (int64_t)p * ref_ld;
    const int pos = atomicAdd(&cursor[cell_id[p]], 1);               // in [start[id], start[id + 1]): the counts came from the same cell_id
    if (pos >= 0 && pos < N) sorted[pos] = make_float4(c[0], c[1], c[2], __int_as_float(p));
}

template <int K>
__global__ __launch_bounds__(THREADS) void search_kernel(const float4* __restrict__ sorted, const int* __restrict__ start, const int* __restrict__ cell_id,
                                                         int N, int k, Grid g, int* __restrict__ nbr_idx, float* __restrict__ nbr_d2,
                                                         double* __restrict__ mean_dist) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= N) return;
    const float4 me = sorted[t];
    const float qx = me.x, qy = me.y, qz = me.z;
    const int qi = min(max(__float_as_int(me.w), 0), N - 1);
    const int id = cell_id[qi];
    const int cx = id % g.nx, cy = (id / g.nx) % g.ny, cz = id / (g.nx * g.ny);
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
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
                    const int s0 = start[row + a], s1 = min(start[row + b + 1], N);
                    for (int p = max(s0, 0); p < s1; ++p) {
                        const float4 c = sorted[p];
                        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                        const float d = fminf((dx * dx + dy * dy) + dz * dz, INFINITY);   // minNum: a NaN key (non-finite coordinates) becomes +inf
                        const int i = __float_as_int(c.w);
                        if (pcn::before(d, i, bd[K - 1], bi[K - 1])) pcn::insert<K>(bd, bi, d, i);
                    }
                }
            }
        }
        if (lx == 0 && hx == g.nx - 1 && ly == 0 && hy == g.ny - 1 && lz == 0 && hz == g.nz - 1) break;   // (a)
        float kth = INFINITY;
        int kth_i = INT_MAX;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s == k - 1) { kth = bd[s]; kth_i = bi[s]; }
        }
        bool stop = kth_i != INT_MAX;                               // the list is full
        if (lx > 0) { const float b = qx - face(g.ox, g.cell, lx); stop = stop && kth < b * b; }
        if (hx < g.nx - 1) { const float b = qx - face(g.ox, g.cell, hx + 1); stop = stop && kth < b * b; }
        if (ly > 0) { const float b = qy - face(g.oy, g.cell, ly); stop = stop && kth < b * b; }
        if (hy < g.ny - 1) { const float b = qy - face(g.oy, g.cell, hy + 1); stop = stop && kth < b * b; }
        if (lz > 0) { const float b = qz - face(g.oz, g.cell, lz); stop = stop && kth < b * b; }
        if (hz < g.nz - 1) { const float b = qz - face(g.oz, g.cell, hz + 1); stop = stop && kth < b * b; }
        if (stop) break;                                            // (b)
        olx = lx; ohx = hx; oly = ly; ohy = hy; olz = lz; ohz = hz;
    }
    if (nbr_idx) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s < k) nbr_idx[(int64_t)qi * k + s] = bi[s];
        }
    }
    if (nbr_d2) {
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s < k) nbr_d2[(int64_t)qi * k + s] = bd[s];
        }
    }
    if (mean_dist) {
        double sum = 0.0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (s < k) sum += sqrt((double)bd[s]);
        }
        mean_dist[qi] = sum / (double)k;
    }
}

inline hipError_t launch_build(const float* ref, int N, int ref_ld, const Grid& g, void* workspace, hipStream_t s) {
    const int cells = cells_of(g);
    const Layout l = layout(N, cells);
    char* ws = static_cast<char*>(workspace);
    int* cell_id = reinterpret_cast<int*>(ws + l.cell_id);
    int* cursor = reinterpret_cast<int*>(ws + l.cursor);
    int* start = reinterpret_cast<int*>(ws + l.start);
    int* tile_sum = reinterpret_cast<int*>(ws + l.tile_sum);
    float4* sorted = reinterpret_cast<float4*>(ws + l.sorted);
    const unsigned groups = (unsigned)((N + THREADS - 1) / THREADS), tiles = (unsigned)((cells + SCAN_TILE - 1) / SCAN_TILE);
    hipError_t e = hipMemsetAsync(cursor, 0, (size_t)cells * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(count_kernel, dim3(groups), dim3(THREADS), 0, s, ref, N, ref_ld, g, cell_id, cursor);
    hipLaunchKernelGGL(tile_sum_kernel, dim3(tiles), dim3(THREADS), 0, s, cursor, cells, tile_sum);
    hipLaunchKernelGGL(scan_kernel, dim3(tiles), dim3(THREADS), 0, s, cursor, cells, tile_sum, N, start);
    hipLaunchKernelGGL(scatter_kernel, dim3(groups), dim3(THREADS), 0, s, ref, N, ref_ld, cell_id, cursor, sorted);
    return hipGetLastError();
}

inline hipError_t launch_search(int N, int k, const Grid& g, int* nbr_idx, float* nbr_d2, double* mean_dist, void* workspace, hipStream_t s) {
    const Layout l = layout(N, cells_of(g));
    char* ws = static_cast<char*>(workspace);
    const int* cell_id = reinterpret_cast<const int*>(ws + l.cell_id);
    const int* start = reinterpret_cast<const int*>(ws + l.start);
    const float4* sorted = reinterpret_cast<const float4*>(ws + l.sorted);
    const dim3 groups((unsigned)((N + THREADS - 1) / THREADS)), threads(THREADS);
    switch (pcn::slots_for(k)) {
        case 8: hipLaunchKernelGGL(search_kernel<8>, groups, threads, 0, s, sorted, start, cell_id, N, k, g, nbr_idx, nbr_d2, mean_dist); break;
        case 16: hipLaunchKernelGGL(search_kernel<16>, groups, threads, 0, s, sorted, start, cell_id, N, k, g, nbr_idx, nbr_d2, mean_dist); break;
        default: hipLaunchKernelGGL(search_kernel<32>, groups, threads, 0, s, sorted, start, cell_id, N, k, g, nbr_idx, nbr_d2, mean_dist); break;
    }
    return hipGetLastError();
}

}  // namespace pcg
}  // namespace ma
