// The device side every radius search over the cell grid of pc_grid.hpp shares (ma_op_pc_cluster, ma_op_pc_smooth, ma_op_pc_upsample): the
// pair bound that the host reads back and compares with max_pairs before the op's long kernel is launched, and the host's test that
// makes the bound hold.  The walks of cluster and smooth are the ring walk of pc_grid.hpp with the stop rule "every side has fl32(b * b) >
// r2", r2 = fl32(radius * radius) ("a walk with limit r2" below), which is what the bound counts; to upsample, whose limit is the seed's key, the bound is a guard and no count (pc_upsample.hpp).
//
// Workspace of such an op: pcg::layout(N, cells) | the 64-bit total of the pair bound | the op's own arrays.
//
// Pair bound (bound_kernel): one thread per cell c computes n_c * (the number of points in the block of R rings around c, clipped to
// the grid), R = floor(radius / cell) + 2; the counts come from `start`, an x-row of the block being one contiguous range of records.
// The values are summed to one 64-bit total (a workgroup sum, then one atomic per workgroup).
// Why this bounds the key evaluations of a walk with limit r2 from above.  A query evaluates keys only against records of cells in its
// block, each cell once, and its block after round r is its own cell's block of r rings.  So it is enough that every query has stopped
// after round R at the latest.  Take a query q in cell c and a side of its block after round R that is not a grid border, say the high
// x side hx = cx + R < nx - 1, with face f = face[hx + 1].  The cell rule gives q < face[cx + 1] (cx < nx - 1), hence f - q > f -
// face[cx + 1] >= 0 exactly; rounding is monotone, so |b| = |fl32(q - f)| >= g = fl32(f - face[cx + 1]) and fl32(b * b) >= fl32(g * g).
// (The low side mirrors it: face[cx] <= q because cx > 0, and g = fl32(face[cx] - face[cx - R]).)  With exact faces g = R * cell >
// radius + cell, since R > radius / cell + 1; the faces are rounded, fl32(origin + fl32(i * cell)), and with an origin that is huge
// against the cell neighbouring faces can even coincide.  Therefore the host evaluates the test fl32(g * g) > r2 itself, on the same
// float32 faces, for every cell index and side of every axis (`rings_suffice`: at most 6 * 128 comparisons, no device work), and the
// call refuses a grid that fails it.  For a grid that passes, every side test of the stop rule holds after round R for every finite
// query; a query with a non-finite coordinate has no key <= r2 (its keys are NaN or +inf) and evaluates no key at all.
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"

namespace ma {
namespace pcr {

constexpr int THREADS = pcg::THREADS;
constexpr int MAX_RINGS_RATIO = 8;                     // radius / cell <= 8: the bound kernel's block is at most 21 x 21 rows per cell

struct Layout {
    size_t total, bytes;
};

// pcg::layout(N, cells) | the 64-bit total of the pair bound; an op's own arrays follow at `bytes`
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = pcg::layout(N, cells).bytes;
    l.total = o; o += wt::align256(sizeof(unsigned long long));
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

}  // namespace pcr

// The kernel keeps the symbol it has had since the bound was the clustering's alone, ma::pcc::bound_kernel: profiles and device-code
// comparisons across this history go by it.
namespace pcc {

__global__ __launch_bounds__(pcr::THREADS) void bound_kernel(const int* __restrict__ start, int N, pcg::Grid g, int R, unsigned long long* __restrict__ total) {
    constexpr int THREADS = pcr::THREADS;
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

}  // namespace pcc

namespace pcr {

inline unsigned long long* total_of(int N, const pcg::Grid& g, void* workspace) {
    return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + layout(N, pcg::cells_of(g)).total);
}

// build, and the pair bound into the workspace's total
inline hipError_t launch_bound(const float* ref, int N, int ref_ld, const pcg::Grid& g, int R, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    char* ws = static_cast<char*>(workspace);
    unsigned long long* total = total_of(N, g, workspace);
    hipError_t e = pcg::launch_build(ref, N, ref_ld, g, workspace, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(total, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pcc::bound_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       reinterpret_cast<const int*>(ws + pcg::layout(N, cells).start), N, g, R, total);
    return hipGetLastError();
}

}  // namespace pcr
}  // namespace ma
