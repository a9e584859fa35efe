// Euclidean clustering of a point cloud over the cell grid of pc_grid.hpp (`--cluster_radius`): the connected
// components of the graph that links rows i and j when
//     d(i, j) = fl32(fl32(dx*dx + dy*dy) + dz*dz) <= r2,  dx = fl32(x_i - x_j), ...,  r2 = fl32(radius * radius) (computed once, on the host)
// the key of ma_op_pc_knn, no FMA contraction; a NaN key links nothing; fl32(a - b) = -fl32(b - a), so the key is symmetric.
// labels[i] = the smallest row index in the component of i: a function of the cloud and the radius alone, not of the grid, of the order
// the atomics resolve in, or of the run.  Has no reference counterpart.
//
// Build: pcg::launch_build, unchanged (records in cell order, `start` the exclusive scan of the cells' counts).
//
// Pair bound, before the long kernel: pcr::launch_bound and the host's pcr::rings_suffice (pc_radius.hpp, which proves that the bound
// holds for a walk with limit r2); the host reads it back and compares it with max_pairs before the hook kernel is launched.
//
// Hook (hook_kernel): one query per thread, 256 per workgroup, queries in cell order (thread t owns record t) so that a wave's lanes
// walk the same cells.  The block grows ring by ring and a round visits only the cells gained: the row and segment walk of
// pcg::search_kernel.  The query stops when the block is the whole grid, or when every side that is not a grid border has fl32(b * b) >
// r2, b = fl32(q_axis - face_of_that_side).  Why that is exact: by the bound argument in the header of pc_grid.hpp every unsearched point has key >=
// fl32(b * b) of some such side, > r2, hence is not linked.  For every visited record j with j < i and d <= r2 the thread unites i
// and j in `parent`; the pair (i, j) is seen from the larger row alone, which is enough because the key is symmetric.
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
#include "pc_radius.hpp"

namespace ma {
namespace pcc {

constexpr int THREADS = pcg::THREADS;

struct Layout {
    size_t parent, bytes;
};

// pcr::layout(N, cells) | parent (N) int32
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = pcr::layout(N, cells).bytes;
    l.parent = o; o += wt::align256((size_t)N * sizeof(int));
    l.bytes = o;
    return l;
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
    hipLaunchKernelGGL(init_kernel, groups, threads, 0, s, parent, N);
    hipLaunchKernelGGL(hook_kernel, groups, threads, 0, s, reinterpret_cast<const float4*>(ws + gl.sorted), reinterpret_cast<const int*>(ws + gl.start),
                       reinterpret_cast<const int*>(ws + gl.cell_id), N, r2, g, parent);
    hipLaunchKernelGGL(flatten_kernel, groups, threads, 0, s, parent, N, labels, sizes);
    return hipGetLastError();
}

}  // namespace pcc
}  // namespace ma
