// Moving-least-squares smoothing of a point cloud over the cell grid of pc_grid.hpp (`--smooth_radius`): every row is
// projected onto the plane fitted to its radius neighbourhood, PCL's MovingLeastSquares without the polynomial.  Has no reference counterpart.
//
// The rule, for row i at position q, with r2 = fl32(radius * radius) computed once on the host:
//   neighbours: every row j, i included, with d = fl32(fl32(dx*dx + dy*dy) + dz*dz) <= r2, dx = fl32(q_x - x_j), ... -- the key of
//     ma_op_pc_knn and the link rule of ma_op_pc_cluster, no FMA contraction; a NaN key is not a neighbour.  count[i] = their number.
//   weights, float64, no contraction: s = (double)d / (double)r2, u = 1 - s, w = (u*u)*u.  A polynomial: exact IEEE operations, so a
//     numpy restatement gives every term bit for bit and only the order of the sum differs; 0 at the rim, so a row whose key equals r2
//     changes count and nothing else.
//   moments with e = ((double)dx, (double)dy, (double)dz), the differences of the key: S0 = sum w, S1 = sum w*e, S2_ab = sum (w*e_a)*e_b,
//     summed in the order the walk visits the records.
//   plane: mu = S1 / S0, C = S2 / S0 - mu mu^T, pcn::smallest_eigenvector (the Jacobi of ma_op_pc_normals, its order and sign rule).
//   projection onto the plane through the weighted centroid q - mu: t = (mu_x*n_x + mu_y*n_y) + mu_z*n_z, moved = (double)q - t*n.
//   a row STAYS, moved = (double)q, normal (0, 0, 1), eigenvalues 0, when count < min_count, when all its neighbours coincide, or when
//     anything comes out non-finite.
//
// Build: pcg::launch_build, unchanged.  Pair bound: pcr::launch_bound and the host's pcr::rings_suffice (pc_radius.hpp, whose argument
// is about a walk with limit r2, which this one is).  The workspace is pcr::layout, nothing of this op's own.  The bound is read back by
// the host and compared with max_pairs before the smooth kernel is launched.
//
// Smooth (smooth_kernel): one query per thread, 256 per workgroup, queries in cell order (thread t owns record t) so that a wave's lanes
// walk the same cells; the ring and segment walk and the radius stop rule of pcc::hook_kernel.  The ten float64 accumulators and the
// count live in registers, the Jacobi solve and the projection run in the same thread, and the outputs go to the ORIGINAL row (the
// record's index): no neighbour list ever reaches memory.  No atomics in this kernel; the order of the records inside a cell comes from
// the build's atomics, so the sums may differ between runs in their last bits, count may not.
//
// Non-finite coordinates through the raw ABI: every read stays inside the records and the cell starts (pc_grid.hpp); such a query has
// no neighbour (its keys are NaN or +inf), evaluates no key and stays; row indices read from the records are clamped into [0, N).
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"
#include "pc_normals.hpp"
#include "pc_radius.hpp"

namespace ma {
namespace pcs {

constexpr int THREADS = pcg::THREADS;
constexpr int MIN_COUNT = 3;

__global__ __launch_bounds__(THREADS) void smooth_kernel(const float4* __restrict__ sorted, const int* __restrict__ start, const int* __restrict__ cell_id,
                                                         int N, float r2, pcg::Grid g, int min_count, double* __restrict__ moved,
                                                         double* __restrict__ normals, double* __restrict__ eigvals, int* __restrict__ count) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= N) return;
    const float4 me = sorted[t];
    const float qx = me.x, qy = me.y, qz = me.z;
    const int qi = min(max(__float_as_int(me.w), 0), N - 1);
    int cnt = 0;
    bool same = true;                                               // every neighbour so far lies on q
    double s0 = 0.0, s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {             // otherwise every key of this row is NaN or +inf: no neighbour
        const double dr2 = (double)r2;
        const int id = min(max(cell_id[qi], 0), g.nx * g.ny * g.nz - 1);
        const int cx = id % g.nx, cy = (id / g.nx) % g.ny, cz = id / (g.nx * g.ny);
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
                        const int p0 = start[row + a], p1 = min(start[row + b + 1], N);
                        for (int p = max(p0, 0); p < p1; ++p) {
                            const float4 c = sorted[p];
                            const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                            const float d = (dx * dx + dy * dy) + dz * dz;
                            if (!(d <= r2)) continue;               // a NaN key is not a neighbour
                            ++cnt;
                            same = same && dx == 0.f && dy == 0.f && dz == 0.f;
                            const double s = (double)d / dr2, u = 1.0 - s, w = (u * u) * u;
                            const double ex = (double)dx, ey = (double)dy, ez = (double)dz;
                            const double wx = w * ex, wy = w * ey, wz = w * ez;
                            s0 += w;
                            s1x += wx; s1y += wy; s1z += wz;
                            sxx += wx * ex; sxy += wx * ey; sxz += wx * ez;
                            syy += wy * ey; syz += wy * ez; szz += wz * ez;
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
    double mx = (double)qx, my = (double)qy, mz = (double)qz;       // the row stays ...
    double nx = 0.0, ny = 0.0, nz = 1.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;
    if (cnt >= min_count && !same) {                                // ... unless there is a plane to fit
        const double ux = s1x / s0, uy = s1y / s0, uz = s1z / s0;
        double f0, f1, f2, fx, fy, fz;
        pcn::smallest_eigenvector(sxx / s0 - ux * ux, syy / s0 - uy * uy, szz / s0 - uz * uz, sxy / s0 - ux * uy, sxz / s0 - ux * uz, syz / s0 - uy * uz,
                                  f0, f1, f2, fx, fy, fz);
        const double along = (ux * fx + uy * fy) + uz * fz;
        const double px = mx - along * fx, py = my - along * fy, pz = mz - along * fz;
        if (isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(fx) && isfinite(fy) && isfinite(fz) && isfinite(f0) && isfinite(f1) && isfinite(f2)) {
            mx = px; my = py; mz = pz;
            nx = fx; ny = fy; nz = fz;
            l0 = f0; l1 = f1; l2 = f2;
        }
    }
    if (moved) { double* o = moved + 3 * (int64_t)qi; o[0] = mx; o[1] = my; o[2] = mz; }
    if (normals) { double* o = normals + 3 * (int64_t)qi; o[0] = nx; o[1] = ny; o[2] = nz; }
    if (eigvals) { double* o = eigvals + 3 * (int64_t)qi; o[0] = l0; o[1] = l1; o[2] = l2; }
    if (count) count[qi] = cnt;
}

inline hipError_t launch_smooth(int N, float r2, const pcg::Grid& g, int min_count, double* moved, double* normals, double* eigvals, int* count,
                                void* workspace, hipStream_t s) {
    const pcg::Layout gl = pcg::layout(N, pcg::cells_of(g));
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)((N + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, reinterpret_cast<const float4*>(ws + gl.sorted),
                       reinterpret_cast<const int*>(ws + gl.start), reinterpret_cast<const int*>(ws + gl.cell_id), N, r2, g, min_count, moved, normals,
                       eigvals, count);
    return hipGetLastError();
}

}  // namespace pcs
}  // namespace ma
