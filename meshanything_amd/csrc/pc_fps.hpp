// Farthest-point sampling of a point cloud (`--point_sampling fps`).  Has no reference counterpart: the reference
// keeps `np.random.choice(N, n, replace=False)` rows.
//
// ref (N, ref_ld) fp32, xyz in the first three columns.  key(a, b) = fl32(fl32(dx*dx + dy*dy) + dz*dz), dx = fl32(a.x - b.x), ... -- the
// key of knn_search_kernel, no FMA contraction.  m_i = +inf; for t = 0 .. n-1: idx[t] = s_t, d2[t] = m_{s_t}; m_i = min(m_i, key(p_i,
// p_{s_t})); m_{s_t} = -1; s_{t+1} = the i of greatest m_i, the lowest index among equals.  s_0 is the caller's, or (start = -1) the
// point farthest from the bounding box's centre c = fl32(fl32(lo + hi) * 0.5), the lowest index among equals.  "(greater m, then lower
// index)" is a total order, so the pick does not depend on how the points are spread over threads and workgroups: both forms below, and a
// numpy float32 restatement, give the same indices and the same bits.  No atomics, nothing waits for another workgroup inside a launch.
//
// One-workgroup form (N <= ONE_MAX_POINTS): one launch of 1024 threads for all n picks.  A thread keeps P = 1, 2, 4, 8 or 16 points
// (x, y, z, m), point j + 1024 * p in slot p of thread j; every slot index is a compile-time constant, so nothing goes to scratch.
// Per pick: the update and the thread's best slot; the wave's best by four DPP steps and three v_readlane pairs; the lane that
// owns it leaves (m, index, x, y, z) in the wave's LDS entry; ONE barrier; every wave reduces the 16 entries again (each lane reads
// entry lane & 15, four DPP steps) and reads the winner's coordinates from its entry.  The entries are double-buffered by pick parity:
// a wave that writes pick t + 2 has passed the barrier of pick t + 1, which every wave reaches only after it has read pick t.
//
// Many-workgroup form (any N): one launch per pick, m in the workspace.  Workgroup b owns the points [b * slice, (b + 1) * slice).
// Launch t: every workgroup reduces the G (<= 1024) partials (m, index) that launch t - 1 left -- redundantly, each for itself, which
// is what lets a pick be ONE launch with no exchange inside it: a kernel boundary is the only hand-off -- and so knows s_t; workgroup 0
// writes idx[t] and d2[t]; then it updates its slice against p_{s_t} and leaves its own partial in the other of two partial arrays
// (launch t + 1 reads what launch t wrote while it writes its own).  Launch 0 takes m as +inf, so the workspace needs no clearing.
// The host enqueues n launches and reads nothing back.
//
// start = -1: two small launches over the same slices.  Per-slice bounding boxes; then every workgroup reduces the G boxes (min and
// max are exact, so the order does not matter), forms c and leaves (key(p_i, c), i) of its slice's farthest point as a partial, which
// the first pick -- of either form -- reduces like any other.
//
// Non-finite coordinates (the Python side refuses them): a NaN key never lowers m and never wins a comparison; every index that is
// read or written is clamped into [0, N).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "watertight.hpp"

namespace ma {
namespace fps {

constexpr int MAX_POINTS = 1 << 22;
constexpr int ONE_THREADS = 1024;                       // the one-workgroup form: 16 waves, 4 per SIMD, at most 128 VGPRs each
constexpr int ONE_MAX_SLOTS = 16;                       // points per thread: 64 VGPRs of x, y, z, m
constexpr int ONE_MAX_POINTS = ONE_THREADS * ONE_MAX_SLOTS;   // 16 384
// form = 0 takes the one-workgroup form up to here: measured faster at every N it holds (4 096 picks: 5.5 against 19.1 ms at N = 4 096,
// 11.6 against 19.0 ms at N = 16 384; the many-workgroup form is bound by its 4 096 launches until N ~ 2^19)
constexpr int AUTO_ONE_MAX_POINTS = ONE_MAX_POINTS;
constexpr int MANY_THREADS = 256;
constexpr int MIN_SLICE = 512;                          // points per workgroup of the many-workgroup form, at least
constexpr int MAX_GROUPS = 1024;
static_assert(MAX_POINTS / MAX_GROUPS % MANY_THREADS == 0, "the largest slice is whole rounds of a workgroup");

// points per workgroup: MIN_SLICE until that needs more than MAX_GROUPS workgroups, then N / MAX_GROUPS rounded up to whole rounds
inline int slice_for(int N) {
    const int per = (N + MAX_GROUPS - 1) / MAX_GROUPS;
    return std::max(MIN_SLICE, (per + MANY_THREADS - 1) / MANY_THREADS * MANY_THREADS);
}
inline int groups_for(int N) { const int s = slice_for(N); return (N + s - 1) / s; }

// form: 0 = by N, 1 = one workgroup, 2 = many workgroups
inline int resolve_form(int N, int form) { return form != 0 ? form : (N <= AUTO_ONE_MAX_POINTS ? 1 : 2); }

// workspace: m (N) fp32 | partials (2, G) {fp32 m, int32 index} | boxes (G, 6) fp32; the same for every form
struct Layout {
    size_t m, part, box, bytes;
    int G;
};
inline Layout layout(int N) {
    Layout L;
    L.G = groups_for(N);
    L.m = 0;
    L.part = wt::align256((size_t)N * sizeof(float));
    L.box = L.part + 2 * wt::align256((size_t)L.G * 8);
    L.bytes = L.box + wt::align256((size_t)L.G * 6 * sizeof(float));
    return L;
}

struct Partial {
    float m;
    int i;
};

__device__ inline float key(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// (m, i) before (bm, bi): greater m, then lower index
__device__ inline bool better(float m, int i, float bm, int bi) { return (m > bm) | ((m == bm) & (i < bi)); }   // no branches

template <int CTRL>
__device__ inline void dpp_best(float& m, int& i) {
    const float om = dpp_mov<CTRL>(m);
    const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xf, 0xf, false);
    const bool b = better(om, oi, m, i);
    m = b ? om : m;
    i = b ? oi : i;
}
// the best of each aligned group of 16 lanes, in every lane of the group
__device__ inline void row_best(float& m, int& i) {
    dpp_best<DPP_XOR1>(m, i);
    dpp_best<DPP_XOR2>(m, i);
    dpp_best<DPP_HALF_MIRROR>(m, i);
    dpp_best<DPP_ROW_MIRROR>(m, i);
}
// the best of the wave, in every lane
__device__ inline void wave_best(float& m, int& i) {
    row_best(m, i);
    float bm = readlane_f(m, 0);
    int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float om = readlane_f(m, r);
        const int oi = __builtin_amdgcn_readlane(i, r);
        const bool b = better(om, oi, bm, bi);
        bm = b ? om : bm;
        bi = b ? oi : bi;
    }
    m = bm;
    i = bi;
}

// the best of a workgroup of up to 16 waves, in every thread; sm / si: 16 entries of LDS that nobody else touches until the next barrier
__device__ inline void block_best(float& m, int& i, float* sm, int* si) {
    wave_best(m, i);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    if (lane == 0) { sm[wave] = m; si[wave] = i; }
    __syncthreads();
    const int e = lane & 15;
    m = e < waves ? sm[e] : -INFINITY;
    i = e < waves ? si[e] : INT_MAX;
    row_best(m, i);
}

__device__ inline int clamp_index(int i, int N) { return min(max(i, 0), N - 1); }

// the best of the G partials a previous launch left, in every thread
__device__ inline void combine_partials(const Partial* __restrict__ part, int G, float& m, int& i, float* sm, int* si) {
    m = -INFINITY;
    i = INT_MAX;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {                // ascending g, ascending index: strictly greater keeps the lowest
        const Partial p = part[g];
        if (better(p.m, p.i, m, i)) { m = p.m; i = p.i; }
    }
    block_best(m, i, sm, si);
}

// ---- start = -1 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MANY_THREADS) void fps_box_kernel(const float* __restrict__ ref, int N, int ref_ld, int slice, float* __restrict__ boxes) {
    __shared__ float red[6][MANY_THREADS / 64];
    const int r0 = blockIdx.x * slice, r1 = min(N, r0 + slice);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = r0 + threadIdx.x; i < r1; i += MANY_THREADS) {
        const float* c = ref + (int64_t)i * ref_ld;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = -wave_max(-lo[a]), h = wave_max(hi[a]);
        if (lane == 0) { red[a][wave] = l; red[3 + a][wave] = h; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[threadIdx.x][0];
        for (int w = 1; w < MANY_THREADS / 64; ++w) v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        boxes[blockIdx.x * 6 + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(MANY_THREADS) void fps_start_kernel(const float* __restrict__ ref, int N, int ref_ld, int slice, int G,
                                                                 const float* __restrict__ boxes, Partial* __restrict__ part_out) {
#pragma clang fp contract(off)
    __shared__ float sm[16];
    __shared__ int si[16];
    __shared__ float red[6][MANY_THREADS / 64];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int g = threadIdx.x; g < G; g += MANY_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], boxes[g * 6 + a]); hi[a] = fmaxf(hi[a], boxes[g * 6 + 3 + a]); }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = -wave_max(-lo[a]), h = wave_max(hi[a]);
        if (lane == 0) { red[a][wave] = l; red[3 + a][wave] = h; }
    }
    __syncthreads();
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float l = red[a][0], h = red[3 + a][0];
        for (int w = 1; w < MANY_THREADS / 64; ++w) { l = fminf(l, red[a][w]); h = fmaxf(h, red[3 + a][w]); }
        c[a] = (l + h) * 0.5f;
    }
    const int r0 = blockIdx.x * slice, r1 = min(N, r0 + slice);
    float bm = -INFINITY;
    int bi = INT_MAX;
    for (int i = r0 + threadIdx.x; i < r1; i += MANY_THREADS) {
        const float* p = ref + (int64_t)i * ref_ld;
        const float d = key(p[0], p[1], p[2], c[0], c[1], c[2]);
        if (d > bm || bi == INT_MAX) { bm = d; bi = i; }              // a NaN key still leaves an index of the slice
    }
    block_best(bm, bi, sm, si);
    if (threadIdx.x == 0) part_out[blockIdx.x] = Partial{bm, bi};
}

// ---- the many-workgroup form: launch t ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MANY_THREADS) void fps_pick_kernel(const float* __restrict__ ref, int N, int ref_ld, int slice, int G, int t, int last, int start,
                                                                float* __restrict__ m, const Partial* __restrict__ part_in,
                                                                Partial* __restrict__ part_out, int* __restrict__ idx, float* __restrict__ d2) {
    __shared__ float sm[2][16];
    __shared__ int si[2][16];
    float cm = INFINITY;
    int s = start;
    if (t > 0 || start < 0) combine_partials(part_in, G, cm, s, sm[0], si[0]);
    if (t == 0) cm = INFINITY;
    s = clamp_index(s, N);
    if (blockIdx.x == 0 && threadIdx.x == 0) { idx[t] = s; d2[t] = cm; }
    if (last) return;
    const float* ps = ref + (int64_t)s * ref_ld;
    const float sx = ps[0], sy = ps[1], sz = ps[2];
    const int r0 = blockIdx.x * slice, r1 = min(N, r0 + slice);
    float bm = -INFINITY;
    int bi = INT_MAX;
    for (int i = r0 + threadIdx.x; i < r1; i += MANY_THREADS) {
        const float* p = ref + (int64_t)i * ref_ld;
        const float old = t == 0 ? INFINITY : m[i];
        float v = fminf(old, key(p[0], p[1], p[2], sx, sy, sz));       // minNum: a NaN key leaves m as it is
        v = i == s ? -1.f : v;
        m[i] = v;
        if (v > bm || bi == INT_MAX) { bm = v; bi = i; }
    }
    block_best(bm, bi, sm[1], si[1]);
    if (threadIdx.x == 0) part_out[blockIdx.x] = Partial{bm, bi};
}

// ---- the one-workgroup form: all n picks ------------------------------------------------------------------------------------------------
struct Entry {                                                         // what a wave leaves per pick: 32 bytes
    float m;
    int i;
    float x, y, z;
    int pad[3];
};

template <int P>
__global__ __launch_bounds__(ONE_THREADS) void fps_one_kernel(const float* __restrict__ ref, int N, int ref_ld, int n, int start,
                                                              const Partial* __restrict__ start_part, int G, int* __restrict__ idx,
                                                              float* __restrict__ d2) {
    __shared__ float sm[16];
    __shared__ int si[16];
    __shared__ __attribute__((aligned(16))) Entry entry[2][ONE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float x[P], y[P], z[P], m[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int i = tid + ONE_THREADS * p;
        const float* c = ref + (int64_t)min(i, N - 1) * ref_ld;        // a slot without a point reads inside ref and is never chosen:
        x[p] = c[0]; y[p] = c[1]; z[p] = c[2];
        m[p] = i < N ? INFINITY : -INFINITY;                           // its m is never lowered
    }
    float cm = INFINITY;
    int s = start;
    if (start < 0) combine_partials(start_part, G, cm, s, sm, si);
    cm = INFINITY;
    s = clamp_index(s, N);
    float sx, sy, sz;
    {
        const float* ps = ref + (int64_t)s * ref_ld;
        sx = ps[0]; sy = ps[1]; sz = ps[2];
    }
    for (int t = 0;; ++t) {
        if (tid == 0) { idx[t] = s; d2[t] = cm; }
        if (t == n - 1) break;
        float bm = -INFINITY;
        int bp = -1;
        const int ds = s - tid;                                        // slot p holds s where ONE_THREADS * p == ds
#pragma unroll
        for (int p = 0; p < P; ++p) {
            float v = fminf(m[p], key(x[p], y[p], z[p], sx, sy, sz));
            v = ds == ONE_THREADS * p ? -1.f : v;
            m[p] = v;
            const bool b = v > bm;                                     // ascending index: strictly greater keeps the lowest
            bm = b ? v : bm;
            bp = b ? p : bp;
        }
        int bi = bp < 0 ? INT_MAX : tid + ONE_THREADS * bp;
        wave_best(bm, bi);
        // the wave's best is a point of this wave (or nothing at all: every slot of the wave empty); its owner publishes it
        const bool owner = bi == INT_MAX ? lane == 0 : (bi & (ONE_THREADS - 1)) == tid;
        if (owner) {
            const int slot = bi == INT_MAX ? 0 : bi / ONE_THREADS;
            float ox = x[0], oy = y[0], oz = z[0];
#pragma unroll
            for (int p = 1; p < P; ++p) {
                ox = slot == p ? x[p] : ox;
                oy = slot == p ? y[p] : oy;
                oz = slot == p ? z[p] : oz;
            }
            Entry e;
            e.m = bm; e.i = bi; e.x = ox; e.y = oy; e.z = oz;
            e.pad[0] = 0; e.pad[1] = 0; e.pad[2] = 0;
            entry[t & 1][wave] = e;
        }
        __syncthreads();
        const Entry* es = entry[t & 1];
        cm = es[lane & 15].m;
        s = es[lane & 15].i;
        row_best(cm, s);
        s = clamp_index(s, N);
        const Entry* w = es + ((s & (ONE_THREADS - 1)) >> 6);
        sx = w->x; sy = w->y; sz = w->z;
    }
}

inline void launch_start(const float* ref, int N, int ref_ld, const Layout& L, void* workspace, hipStream_t s) {
    char* ws = static_cast<char*>(workspace);
    float* boxes = reinterpret_cast<float*>(ws + L.box);
    Partial* part0 = reinterpret_cast<Partial*>(ws + L.part);
    const int slice = slice_for(N);
    hipLaunchKernelGGL(fps_box_kernel, dim3((unsigned)L.G), dim3(MANY_THREADS), 0, s, ref, N, ref_ld, slice, boxes);
    hipLaunchKernelGGL(fps_start_kernel, dim3((unsigned)L.G), dim3(MANY_THREADS), 0, s, ref, N, ref_ld, slice, L.G, boxes, part0);
}

template <int P>
inline void launch_one_p(const float* ref, int N, int ref_ld, int n, int start, const Partial* part0, int G, int* idx, float* d2, hipStream_t s) {
    hipLaunchKernelGGL(fps_one_kernel<P>, dim3(1), dim3(ONE_THREADS), 0, s, ref, N, ref_ld, n, start, part0, G, idx, d2);
}

// form: already resolved (resolve_form), 1 only with N <= ONE_MAX_POINTS
inline hipError_t launch_fps(const float* ref, int N, int ref_ld, int n, int start, int form, int* idx, float* d2, void* workspace, hipStream_t s) {
    const Layout L = layout(N);
    char* ws = static_cast<char*>(workspace);
    Partial* part[2] = {reinterpret_cast<Partial*>(ws + L.part), reinterpret_cast<Partial*>(ws + L.part + wt::align256((size_t)L.G * 8))};
    if (start < 0) launch_start(ref, N, ref_ld, L, workspace, s);      // leaves its partials in part[0]
    if (form == 1) {
        const int slots = (N + ONE_THREADS - 1) / ONE_THREADS;
        if (slots <= 1) launch_one_p<1>(ref, N, ref_ld, n, start, part[0], L.G, idx, d2, s);
        else if (slots <= 2) launch_one_p<2>(ref, N, ref_ld, n, start, part[0], L.G, idx, d2, s);
        else if (slots <= 4) launch_one_p<4>(ref, N, ref_ld, n, start, part[0], L.G, idx, d2, s);
        else if (slots <= 8) launch_one_p<8>(ref, N, ref_ld, n, start, part[0], L.G, idx, d2, s);
        else launch_one_p<16>(ref, N, ref_ld, n, start, part[0], L.G, idx, d2, s);
        return hipGetLastError();
    }
    float* m = reinterpret_cast<float*>(ws + L.m);
    const int slice = slice_for(N);
    for (int t = 0; t < n; ++t)                                        // launch t reads part[t & 1], writes part[(t + 1) & 1]
        hipLaunchKernelGGL(fps_pick_kernel, dim3((unsigned)L.G), dim3(MANY_THREADS), 0, s, ref, N, ref_ld, slice, L.G, t, t == n - 1 ? 1 : 0, start, m,
                           part[t & 1], part[(t + 1) & 1], idx, d2);
    return hipGetLastError();
}

}  // namespace fps
}  // namespace ma
