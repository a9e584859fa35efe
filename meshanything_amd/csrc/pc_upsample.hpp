// Upsampling of a sparse point cloud over the cell grid of pc_grid.hpp (`--upsample_radius`): every row with a plane
// seeds a disc of lattice points in that plane, and a lattice point is kept iff its seed is the row nearest to it.  PCL's
// MovingLeastSquares with SAMPLE_LOCAL_PLANE upsampling is the same operation, plus the Voronoi restriction.  Has no reference counterpart.
//
// The rule.  Inputs: ref (N, ld >= 3) float32; per row a float64 unit normal n (N, 3), an INPUT of the op (ma_op_pc_smooth fits one);
// per row an optional `active` byte; an integer m in 1..64; step as float64 (the host passes radius / m, computed in float64); a grid as
// in ma_op_pc_smooth with m * step / cell <= 8.  Seed row i at position q is skipped when active is given and 0, when q is not finite or
// when n is not finite.  All arithmetic below is float64 with no FMA contraction, IEEE division and square root:
//   frame: a = the axis with the smallest |n_a|, ties to the lowest axis; u0 = e_a - n_a * n, each component as written;
//     u = u0 / sqrt((u0x^2 + u0y^2) + u0z^2); v = n x u, v_x = n_y*u_z - n_z*u_y and cyclically, not renormalised.
//   candidates: for a in -m..m (outer loop), b in -m..m (inner loop), (a, b) != (0, 0), integer a*a + b*b <= m*m: da = (double)a * step,
//     db = (double)b * step, p_x = (double)q_x + (da*u_x + db*v_x), likewise y and z; c = (float)p, round to nearest; a non-finite c is dropped.
//   keep test, a Voronoi restriction: c is kept iff seed i comes first among ALL rows in the order (d, index), d = fl32(fl32(dx*dx + dy*dy)
//     + dz*dz), dx = fl32(c_x - x_j), ...: the key of ma_op_pc_knn, a NaN key counts as +inf.  A candidate nearer to another row belongs to
//     that row's patch or to nobody; duplicated rows give all their candidates to the lower index; patches of neighbouring seeds do not
//     overlap.
//   output: the kept candidates seed-major (seed 0's, then seed 1's, ...), within a seed in (a, b) loop order: out_xyz (T, 3) float32,
//     out_seed (T) int32, counts (N) int32.  The decision and the bits depend on the inputs alone, not on the grid, on the order of the
//     records inside a cell or on the run: nothing is accumulated, and the first-in-order test has one answer whatever the visiting order.
//
// Search.  The candidate's cell comes from pcg::cell_of; border cells are unbounded outward, so a candidate outside the box is fine.  The
// ring and segment walk is pcg::search_kernel's.  A candidate ends as NOT kept at the first record that precedes the seed in (d, index).
// Otherwise the walk stops, and the candidate is kept, when the block is the whole grid, or when every side of the block that is not a
// grid border has fl32(b * b) > ds STRICTLY, b = fl32(c_axis - face_of_that_side), ds = the seed's key.
// Why that is exact, with no slack (the argument of pc_grid.hpp, the candidate c in the place of the query).  Take a row r outside the
// block; on some axis its cell lies beyond a side of the block that is not a grid border, say above the high side hi < dim - 1 with face
// f = face[hi + 1].  By the cell rule f <= face[cell(r)] <= r, and c < f because c's own cell is <= hi.  So r - c >= f - c > 0 exactly,
// rounding is monotone, |fl32(c - r)| >= |fl32(c - f)| = |b|, fl32(dx * dx) >= fl32(b * b), and every later step of the key adds a
// non-negative term and rounds monotonically: key(r) >= fl32(b * b) > ds.  (The low side mirrors it.)  So no unsearched row precedes the
// seed; the strict inequality keeps out the unsearched row of EQUAL key and lower index.  If the seed itself is still outside the block
// the rule cannot fire (its own key is ds), so a kept candidate has always met its seed.  A non-finite ds (overflow) never satisfies the
// rule and the walk ends at the whole grid after at most 127 rounds.
//
// Kernels: one workgroup of 256 threads per seed.  Thread 0 computes the frame once and shares it through LDS.  The threads stride over
// the (2m+1)^2 lattice slots in loop order, 256 per round; per round the kept flags go through one wave ballot each and a four-entry LDS
// prefix (double-buffered by round parity: one barrier per round), which gives every kept slot its ordered position with no atomics.
// count pass (lattice_kernel<false>): the per-seed counts as 64-bit values -> wt::scan_exclusive, in place, N + 1 entries so the last is
// the total -> the host reads the total back -> emit pass (lattice_kernel<true>) recomputes the keep tests, the same code on the same
// inputs, and writes at offset[seed] + position.  Every write is also guarded by the capacity.  No atomics beyond pcg::launch_build's.
//
// Pair bound: pcr::launch_bound and pcr::rings_suffice (pc_radius.hpp) with radius fl32(m * step), read back and compared with max_pairs
// before the long kernels, as in pc_smooth.hpp.  Here it is the guard against a radius the size of the cloud and not a count of this
// op's keys: a candidate is no row, and its walk ends at the first row that precedes its seed, typically inside its own cell.
//
// Non-finite input through the raw ABI: such a seed is skipped; as a record a non-finite row has key NaN -> +inf or +inf and precedes a
// seed only at an infinite ds.  Every read stays inside the records and the cell starts (pc_grid.hpp), and row indices read from the
// records are clamped into [0, N).
#pragma once
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "pc_grid.hpp"
#include "pc_radius.hpp"
#include "watertight.hpp"

namespace ma {
namespace pcu {

constexpr int THREADS = pcg::THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_M = 64;
constexpr int64_t MAX_SLOTS = int64_t(1) << 31;      // N * (2m+1)^2

struct Layout {
    size_t offs, scan, bytes;
};

// pcr::layout(N, cells) | offs (N + 1) int64: the counts, then their exclusive scan | the scan's tiles
inline Layout layout(int N, int cells) {
    Layout l;
    size_t o = pcr::layout(N, cells).bytes;
    l.offs = o;  o += wt::align256(((size_t)N + 1) * sizeof(int64_t));
    l.scan = o;  o += wt::align256((size_t)wt::scan_ws_elems((int64_t)N + 1) * sizeof(int64_t));
    l.bytes = o;
    return l;
}

// is seed `seed`, whose key to the candidate c is ds, first among all rows in the order (d, index)
__device__ inline bool seed_is_first(const float4* __restrict__ sorted, const int* __restrict__ start, int N, const pcg::Grid& g, float cx_, float cy_,
                                     float cz_, float ds, int seed) {
#pragma clang fp contract(off)
    const int cx = pcg::cell_of(cx_, g.ox, g.cell, g.nx), cy = pcg::cell_of(cy_, g.oy, g.cell, g.ny), cz = pcg::cell_of(cz_, g.oz, g.cell, g.nz);
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
                        const float dx = cx_ - c.x, dy = cy_ - c.y, dz = cz_ - c.z;
                        const float d = fminf((dx * dx + dy * dy) + dz * dz, INFINITY);   // minNum: a NaN key becomes +inf
                        const int j = min(max(__float_as_int(c.w), 0), N - 1);
                        if (d < ds || (d == ds && j < seed)) return false;
                    }
                }
            }
        }
        if (lx == 0 && hx == g.nx - 1 && ly == 0 && hy == g.ny - 1 && lz == 0 && hz == g.nz - 1) return true;
        bool stop = true;
        if (lx > 0) { const float b = cx_ - pcg::face(g.ox, g.cell, lx); stop = stop && b * b > ds; }
        if (hx < g.nx - 1) { const float b = cx_ - pcg::face(g.ox, g.cell, hx + 1); stop = stop && b * b > ds; }
        if (ly > 0) { const float b = cy_ - pcg::face(g.oy, g.cell, ly); stop = stop && b * b > ds; }
        if (hy < g.ny - 1) { const float b = cy_ - pcg::face(g.oy, g.cell, hy + 1); stop = stop && b * b > ds; }
        if (lz > 0) { const float b = cz_ - pcg::face(g.oz, g.cell, lz); stop = stop && b * b > ds; }
        if (hz < g.nz - 1) { const float b = cz_ - pcg::face(g.oz, g.cell, hz + 1); stop = stop && b * b > ds; }
        if (stop) return true;
        olx = lx; ohx = hx; oly = ly; ohy = hy; olz = lz; ohz = hz;
    }
}

// EMIT = false: offs[seed] = counts[seed] = the kept candidates of the seed.  EMIT = true: offs is the scan; writes out_xyz / out_seed.
template <bool EMIT>
__global__ __launch_bounds__(THREADS) void lattice_kernel(const float* __restrict__ ref, int N, int ref_ld, const double* __restrict__ normals,
                                                          const uint8_t* __restrict__ active, int m, double step, const float4* __restrict__ sorted,
                                                          const int* __restrict__ start, pcg::Grid g, int64_t* __restrict__ offs,
                                                          int* __restrict__ counts, float* __restrict__ out_xyz, int* __restrict__ out_seed,
                                                          int64_t capacity) {
#pragma clang fp contract(off)
    __shared__ double frame[6];                                     // u, v
    __shared__ int seeded;
    __shared__ int wave_kept[2][WAVES];
    const int seed = blockIdx.x;                                    // < N: the launch has N workgroups
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* qp = ref + (int64_t)seed * ref_ld;
    const float qx = qp[0], qy = qp[1], qz = qp[2];
    if (tid == 0) {
        const double nx = normals[3 * (int64_t)seed], ny = normals[3 * (int64_t)seed + 1], nz = normals[3 * (int64_t)seed + 2];
        const bool on = (!active || active[seed] != 0) && isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(nx) && isfinite(ny) && isfinite(nz);
        seeded = on ? 1 : 0;
        if (on) {
            const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
            const int a = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);   // the smallest |n_a|, ties to the lowest axis
            const double na = a == 0 ? nx : (a == 1 ? ny : nz);
            const double u0x = (a == 0 ? 1.0 : 0.0) - na * nx, u0y = (a == 1 ? 1.0 : 0.0) - na * ny, u0z = (a == 2 ? 1.0 : 0.0) - na * nz;
            const double len = sqrt((u0x * u0x + u0y * u0y) + u0z * u0z);
            const double ux = u0x / len, uy = u0y / len, uz = u0z / len;
            frame[0] = ux; frame[1] = uy; frame[2] = uz;
            frame[3] = ny * uz - nz * uy; frame[4] = nz * ux - nx * uz; frame[5] = nx * uy - ny * ux;
        }
    }
    __syncthreads();
    if (!seeded) {                                                  // the whole workgroup alike
        if (!EMIT && tid == 0) { offs[seed] = 0; if (counts) counts[seed] = 0; }
        if (EMIT && tid == 0 && counts) counts[seed] = 0;
        return;
    }
    const double ux = frame[0], uy = frame[1], uz = frame[2], vx = frame[3], vy = frame[4], vz = frame[5];
    const int side = 2 * m + 1, slots = side * side;
    const int64_t first = EMIT ? offs[seed] : 0;
    int base = 0;                                                   // kept in the rounds before
    for (int s0 = 0, round = 0; s0 < slots; s0 += THREADS, ++round) {
        const int slot = s0 + tid;
        bool keep = false;
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (slot < slots) {
            const int a = slot / side - m, b = slot % side - m;
            if ((a != 0 || b != 0) && a * a + b * b <= m * m) {
                const double da = (double)a * step, db = (double)b * step;
                const double px = (double)qx + (da * ux + db * vx), py = (double)qy + (da * uy + db * vy), pz = (double)qz + (da * uz + db * vz);
                cx = (float)px; cy = (float)py; cz = (float)pz;
                if (isfinite(cx) && isfinite(cy) && isfinite(cz)) {
                    const float dx = cx - qx, dy = cy - qy, dz = cz - qz;
                    const float ds = fminf((dx * dx + dy * dy) + dz * dz, INFINITY);
                    keep = seed_is_first(sorted, start, N, g, cx, cy, cz, ds, seed);
                }
            }
        }
        const unsigned long long ballot = __ballot(keep);
        if (lane == 0) wave_kept[round & 1][wave] = __popcll(ballot);
        __syncthreads();                                            // the next round writes the other buffer: one barrier per round
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int k = wave_kept[round & 1][w];
            if (w < wave) before += k;
            all += k;
        }
        if (EMIT && keep) {
            const int64_t at = first + base + before + __popcll(ballot & ((1ull << lane) - 1ull));
            if (at >= 0 && at < capacity) {
                if (out_xyz) { float* o = out_xyz + 3 * at; o[0] = cx; o[1] = cy; o[2] = cz; }
                if (out_seed) out_seed[at] = seed;
            }
        }
        base += all;
    }
    if (tid == 0) {
        if (!EMIT) offs[seed] = base;
        if (counts) counts[seed] = base;
    }
}

inline int64_t* offs_of(int N, const pcg::Grid& g, void* workspace) {
    return reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + layout(N, pcg::cells_of(g)).offs);
}

// the count pass and the scan; afterwards offs[N] (device) is the total.  counts: written here only by a count-only call
inline hipError_t launch_count(const float* ref, int N, int ref_ld, const double* normals, const uint8_t* active, int m, double step, const pcg::Grid& g,
                               int* counts, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const pcg::Layout gl = pcg::layout(N, cells);
    const Layout l = layout(N, cells);
    char* ws = static_cast<char*>(workspace);
    int64_t* offs = reinterpret_cast<int64_t*>(ws + l.offs);
    hipError_t e = hipMemsetAsync(offs + N, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lattice_kernel<false>, dim3((unsigned)N), dim3(THREADS), 0, s, ref, N, ref_ld, normals, active, m, step,
                       reinterpret_cast<const float4*>(ws + gl.sorted), reinterpret_cast<const int*>(ws + gl.start), g, offs, counts, (float*)nullptr,
                       (int*)nullptr, (int64_t)0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return wt::scan_exclusive(offs, (int64_t)N + 1, reinterpret_cast<int64_t*>(ws + l.scan), s);
}

inline hipError_t launch_emit(const float* ref, int N, int ref_ld, const double* normals, const uint8_t* active, int m, double step, const pcg::Grid& g,
                              int* counts, float* out_xyz, int* out_seed, int64_t capacity, void* workspace, hipStream_t s) {
    const int cells = pcg::cells_of(g);
    const pcg::Layout gl = pcg::layout(N, cells);
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(lattice_kernel<true>, dim3((unsigned)N), dim3(THREADS), 0, s, ref, N, ref_ld, normals, active, m, step,
                       reinterpret_cast<const float4*>(ws + gl.sorted), reinterpret_cast<const int*>(ws + gl.start), g,
                       reinterpret_cast<int64_t*>(ws + layout(N, cells).offs), counts, out_xyz, out_seed, capacity);
    return hipGetLastError();
}

}  // namespace pcu
}  // namespace ma
