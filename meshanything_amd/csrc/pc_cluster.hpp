// Euclidean clustering of a point cloud over the cell grid of pc_grid.hpp (`--cluster_radius`): the connected
// components of the graph that links rows i and j when
//     d(i, j) = fl32(fl32(dx*dx + dy*dy) + dz*dz) <= r2,  dx = fl32(x_i - x_j), ...,  r2 = fl32(radius * radius) (computed once, on the host)
// the key of ma_op_pc_knn, no FMA contraction; a NaN key links nothing; fl32(a - b) = -fl32(b - a), so the key is symmetric.
// labels[i] = the smallest row index in the component of i: a function of the cloud and the radius alone, not of the grid, of the order
// the atomics resolve in, or of the run.  Has no reference counterpart.
//
// Build: pcg::launch_build, unchanged (records in cell order, `start` the exclusive scan of the cells' counts).
//
// Pair bound (bound_kernel), before the long kernel: one thread per cell c computes n_c * (the number of points in the block of R rings
// around c, clipped to the grid), R = floor(radius / cell) + 2; the counts come from `start`, an x-row of the block being one contiguous
// range of records.  The values are summed to one 64-bit total (a workgroup sum, then one atomic per workgroup), which the host reads
// back and compares with max_pairs before the hook kernel is launched.
// Why this bounds the key evaluations of the hook kernel from above.  A query evaluates keys only against records of cells in its
// block, each cell once, and its block after round r is its own cell's block of r rings.  So it is enough that every query has stopped
// after round R at the latest.  Take a query q in cell c and a side of its block after round R that is not a grid border, say the high
// x side hx = cx + R < nx - 1, with face f = face[hx + 1].  The cell rule gives q < face[cx + 1] (cx < nx - 1), hence f - q > f -
// face[cx + 1] >= 0 exactly; rounding is monotone, so |b| = |fl32(q - f)| >= g = fl32(f - face[cx + 1]) and fl32(b * b) >= fl32(g * g).
// (The low side mirrors it: face[cx] <= q because cx > 0, and g = fl32(face[cx] - face[cx - R]).)  With exact faces g = R * cell >
// radius + cell, since R > radius / cell + 1; the faces are rounded, fl32(origin + fl32(i * cell)), and with an origin that is huge
// against the cell neighbouring faces can even coincide.  Therefore the host evaluates the test fl32(g * g) > r2 itself, on the same
// float32 faces, for every cell index and side of every axis (`rings_suffice`: at most 6 * 128 comparisons, no device work), and the
// call refuses a grid that fails it.  For a grid that passes, every side test of the stop rule holds after round R for every finite
// query; a query with a non-finite coordinate links nothing (its keys are NaN or +inf) and evaluates no key at all.
//
// Hook (hook_kernel): one query per thread, 256 per workgroup, queries in cell order (thread t owns record t) so that a wave's lanes
// walk the same cells.  The block grows ring by ring and a round visits only the cells gained: the row and segment walk of
// pcg::search_kernel.  The query stops when the block is the whole grid, or when every side that is not a grid border has fl32(b * b) >
// r2, b = fl32(q_axis - face_of_that_side).  Why that is exact: by the bound argument in the header of pc_grid.hpp every unsearched
// point has key >= fl32(b * b) of some such side, > r2, hence is not linked.  For every visited record j with j < i and d <= r2 the
// thread unites i and j in `parent`; the pair (i, j) is seen from the larger row alone, which is enough because the key is symmetric.
//
// Union-find over parent (N) int32, parent[x] = x at the start, lock-free, with the invariant parent[x] <= x.  `find` follows parents;
// path halving stores only an ancestor of x, which is < x.  `unite` takes two roots as last seen; equal: done (in a dense cloud nearly
// every pair); else it CASes the larger from itself to the smaller, and on failure goes on from the value the CAS returned.  A failed
// CAS means another thread's CAS on that word succeeded, and the failing thread's larger root strictly decreases, so the loop ends; no
// thread waits for another's progress.  parent[x] < x for every non-root, so there is no cycle, and a root only ever hooks below a
// smaller row: the root of a finished component is its smallest row.
// Visibility: every read and write of `parent` inside the hook launch is an agent-scope relaxed atomic (__hip_atomic_load / _store /
// _compare_exchange_strong with __HIP_MEMORY_SCOPE_AGENT).  A plain load may be served from an L1 line that another CU's store never
// refreshes.  With the invariant a stale value is still an ancestor, so correctness does not hang on it; the termination of the retry
// loop and the amount of wasted work do.  No ordering between different words is needed: the only payload is the word itself.
//
// Flatten (flatten_kernel): a second launch, the kernel boundary publishes `parent`.  labels[i] = find(i) and, if sizes is given, one
// atomicAdd per row on sizes[root] (zeroed before).
//
// Non-finite coordinates through the raw ABI: every read stays inside the records and the cell starts (pc_grid.hpp); such a query
// returns at once, and as a record its key is NaN or +inf and links nothing; row indices read from the records are clamped into [0, N).
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"

namespace ma {
namespace pcc {

constexpr int THREADS = pcg::THREADS;
constexpr int MAX_RINGS_RATIO = 8;                     // radius / cell <= 8: the bound kernel's block is at most 21 x 21 rows per cell

struct Layout {
    size_t parent, total, bytes;
};

// pcg::layout(N, cells) | parent (N) int32 | the 64-bit total of the pair bound
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = pcg::layout(N, cells).bytes;
    l.parent = o; o += wt::align256((size_t)N * sizeof(int));
    l.total = o;  o += wt::align256(sizeof(unsigned long long));
    l.bytes = o;
    return l;
}

inline int rings(float radius, float cell) { return (int)std::floor((double)radius / (double)cell) + 2; }

// pcg::face on the host: the same two float32 roundings
inline float face_host(float origin, float cell, int i) {
#pragma clang fp contract(off)
    volatile float step = (float)i * cell;
    volatile float f = origin + step;
    return f;
}

// does every side test of the stop rule hold after round R, for every cell index of every axis (header comment)
inline bool rings_suffice(const pcg::Grid& g, float r2, int R) {
#pragma clang fp contract(off)
    const float origin[3] = {g.ox, g.oy, g.oz};
    const int dims[3] = {g.nx, g.ny, g.nz};
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < dims[a]; ++c) {
            if (c + R < dims[a] - 1) {
                volatile float gap = face_host(origin[a], g.cell, c + R + 1) - face_host(origin[a], g.cell, c + 1);
                volatile float sq = gap * gap;
                if (!(sq > r2)) return false;
            }
            if (c - R > 0) {
                volatile float gap = face_host(origin[a], g.cell, c) - face_host(origin[a], g.cell, c - R);
                volatile float sq = gap * gap;
                if (!(sq > r2)) return false;
            }
        }
    }
    return true;
}

// ---- union-find: every access an agent-scope relaxed atomic -------------------------------------------------------------------------
__device__ inline int load_parent(int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int find(int* parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p == x) return x;
        const int gp = load_parent(parent, p);
        if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving: gp is an ancestor of x, gp < p < x
        x = gp;
    }
}

// a and b: roots as last seen (each an ancestor of its row); returns an ancestor of both rows
__device__ inline int unite(int* parent, int a, int b) {
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }               // a the larger
        int seen = a;
        if (__hip_atomic_compare_exchange_strong(parent + a, &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return b;
        a = find(parent, seen);                                     // another thread hooked a: seen = parent[a] < a
        b = find(parent, b);
    }
    return a;
}

__global__ __launch_bounds__(THREADS) void init_kernel(int* __restrict__ parent, int N) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < N) parent[i] = i;
}

// ---- the pair bound -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void bound_kernel(const int* __restrict__ start, int N, pcg::Grid g, int R, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long sh[THREADS];
    const int cells = g.nx * g.ny * g.nz;
    const int c = blockIdx.x * THREADS + threadIdx.x;
    unsigned long long mine = 0;
    if (c < cells) {
        const int n = min(max(start[c + 1] - start[c], 0), N);
        if (n > 0) {
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
            mine = (unsigned long long)n * around;
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

// ---- hook ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void hook_kernel(const float4* __restrict__ sorted, const int* __restrict__ start, const int* __restrict__ cell_id,
                                                       int N, float r2, pcg::Grid g, int* parent) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= N) return;
    const float4 me = sorted[t];
    const float qx = me.x, qy = me.y, qz = me.z;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) return;    // every key of this row is NaN or +inf: it links nothing
    const int qi = min(max(__float_as_int(me.w), 0), N - 1);
    const int id = min(max(cell_id[qi], 0), g.nx * g.ny * g.nz - 1);
    const int cx = id % g.nx, cy = (id / g.nx) % g.ny, cz = id / (g.nx * g.ny);
    int root = qi;                                                  // an ancestor of qi, the root when last seen
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
                        const int j = __float_as_int(c.w);
                        if (j < 0 || j >= qi) continue;             // each pair from its larger row
                        const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                        const float d = (dx * dx + dy * dy) + dz * dz;
                        if (!(d <= r2)) continue;                   // a NaN key links nothing
                        const int other = find(parent, j);
                        if (other != root) root = unite(parent, root, other);
                    }
                }
            }
        }
        if (lx == 0 && hx == g.nx - 1 && ly == 0 && hy == g.ny - 1 && lz == 0 && hz == g.nz - 1) break;
        bool stop = true;
        if (lx > 0) { const float b = qx - pcg::face(g.ox, g.cell, lx); stop = stop && b * b > r2; }
        if (hx < g.nx - 1) { const float b = qx - pcg::face(g.ox, g.cell, hx + 1); stop = stop && b * b > r2; }
        if (ly > 0) { const float b = qy - pcg::face(g.oy, g.cell, ly); stop = stop && b * b > r2; }
        if (hy < g.ny - 1) { const float b = qy - pcg::face(g.oy, g.cell, hy + 1); stop = stop && b * b > r2; }
        if (lz > 0) { const float b = qz - pcg::face(g.oz, g.cell, lz); stop = stop && b * b > r2; }
        if (hz < g.nz - 1) { const float b = qz - pcg::face(g.oz, g.cell, hz + 1); stop = stop && b * b > r2; }
        if (stop) break;
        olx = lx; ohx = hx; oly = ly; ohy = hy; olz = lz; ohz = hz;
    }
}

// ---- flatten ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void flatten_kernel(int* parent, int N, int* __restrict__ labels, int* __restrict__ sizes) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const int root = min(max(find(parent, i), 0), N - 1);
    labels[i] = root;
    if (sizes) atomicAdd(&sizes[root], 1);
}

inline unsigned long long* total_of(int N, const pcg::Grid& g, void* workspace) {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + layout(N, pcg::cells_of(g)).total);
}

// build, parent[i] = i, and the pair bound into the workspace's total
inline hipError_t launch_bound(const float* ref, int N, int ref_ld, const pcg::Grid& g, int R, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const Layout l = layout(N, cells);
    char* ws = static_cast<char*>(workspace);
    hipError_t e = pcg::launch_build(ref, N, ref_ld, g, workspace, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws + l.total, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const int* start = reinterpret_cast<const int*>(ws + pcg::layout(N, cells).start);
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, reinterpret_cast<int*>(ws + l.parent), N);
    hipLaunchKernelGGL(bound_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, start, N, g, R,
                       reinterpret_cast<unsigned long long*>(ws + l.total));
    return hipGetLastError();
}

inline hipError_t launch_hook_flatten(int N, float r2, const pcg::Grid& g, int* labels, int* sizes, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const pcg::Layout gl = pcg::layout(N, cells);
    const Layout l = layout(N, cells);
    char* ws = static_cast<char*>(workspace);
    int* parent = reinterpret_cast<int*>(ws + l.parent);
    const dim3 groups((unsigned)((N + THREADS - 1) / THREADS)), threads(THREADS);
    if (sizes) {
        const hipError_t e = hipMemsetAsync(sizes, 0, (size_t)N * sizeof(int), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hook_kernel, groups, threads, 0, s, reinterpret_cast<const float4*>(ws + gl.sorted), reinterpret_cast<const int*>(ws + gl.start),
                       reinterpret_cast<const int*>(ws + gl.cell_id), N, r2, g, parent);
    hipLaunchKernelGGL(flatten_kernel, groups, threads, 0, s, parent, N, labels, sizes);
    return hipGetLastError();
}

}  // namespace pcc
}  // namespace ma
