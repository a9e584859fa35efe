// Uniform voxel thinning of a point cloud (`--voxel_size`): one surviving ROW per occupied voxel, found with a hash
// table on the device and no sort.  The rule of pcl::UniformSampling, not VoxelGrid's centroid: rows stay rows, so normals and any further
// columns travel with them.  Has no reference counterpart.
//
// The rule (one device function, `classify`).  ref (N, ld) float32, ld = 3 or 6; leaf L > 0 and origin o float32, o the per-axis minimum of
// the cloud.  Per axis, with no FMA contraction and the IEEE division (no fast-math in the build):
//     t = fl32(fl32(x - o) / L),  i = floor(t)
// A row is SKIPPED (keep = 0), tested in this order: a coordinate is not finite; some t is not >= 0; some i >= 2^21, which also raises the
// out-of-range flag.  key = ix << 42 | iy << 21 | iz, 63 bits, so never the EMPTY value of all ones.  The row's offset from its voxel's
// centre in voxel units: e = fl32(t - ((float)i + 0.5f)), exact for i < 2^21 ((float)i + 0.5f has at most 22 significant bits, and t lies
// within half a unit of it); d = fl32(fl32(ex*ex + ey*ey) + ez*ez) >= 0.  The SURVIVOR of a voxel is its row with the least (d, row index).
// That order is total: the survivor is unique and does not depend on the order of evaluation, the hash, the capacity or the chunking.
//
// The table.  `capacity` slots, a power of two, as two arrays of 64-bit words: keys, EMPTY at first, and best, all ones at first, then the
// state block of four 32-bit words (used, overflow, out_of_range, voxels).  best packs (bits of d) << 32 | row index; d >= 0, so the bits
// of d order as d does and an unsigned minimum of the packed word is the minimum of (d, row).
//
// `insert_kernel`, one row per thread, callable on successive chunks with the chunk's first row `row0`, so the cloud never has to be on the
// device at once.  The slot starts at mix(key) & (capacity - 1) and moves on linearly.  A plain load of the key; only on EMPTY a 64-bit
// atomicCAS(EMPTY -> key), whose return value says whose slot it became; a thread that claims a slot adds one to `used`, and used >
// capacity / 2 sets the overflow flag.  In the slot of its key: a plain load of best, and a 64-bit atomicMin only when the row's word is
// below it.  Both filters are safe because a key, once set, never changes and best only ever decreases: a stale value can cost an atomic,
// never skip a needed one.
//
// Termination is by construction: the probe loop runs at most `capacity` iterations, and from the second on a thread leaves it when it
// sees the overflow flag.  A table that fills up ends in the flag, which the host turns into an error; nothing waits on another thread.
//
// `mark_kernel`, one slot per thread: for an occupied slot keep[best & 0xffffffff] = 1 (a row index outside [0, N) is never written),
// and the waves' counts of occupied slots are added to `voxels`.  The host zeroes keep and `voxels` before it.
//
// Every value is written by a vector store, plain C++ or a HIP atomic.  A wave-level merge of the rows of one voxel ahead of the atomics
// was not built (section 19).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ma {
namespace pcv {

constexpr int THREADS = 256;
constexpr unsigned long long EMPTY = ~0ull;
constexpr int STATE_WORDS = 4;                         // used, overflow, out_of_range, voxels
constexpr size_t STATE_BYTES = 256;
constexpr float INDEX_LIMIT = 2097152.f;               // 2^21

struct State {
    unsigned used, overflow, out_of_range, voxels;
};

inline size_t table_bytes(uint64_t capacity) { return (size_t)capacity * 16 + STATE_BYTES; }
inline unsigned long long* keys_of(void* table) { return static_cast<unsigned long long*>(table); }
inline unsigned long long* best_of(void* table, uint64_t capacity) { return static_cast<unsigned long long*>(table) + capacity; }
inline State* state_of(void* table, uint64_t capacity) { return reinterpret_cast<State*>(static_cast<char*>(table) + (size_t)capacity * 16); }

struct Grid {
    float ox, oy, oz, leaf;
};

// 0 = skipped, 1 = a row of a voxel (key and d set), 2 = skipped and out of range
__device__ inline int classify(float x, float y, float z, const Grid& g, unsigned long long& key, float& d) {
#pragma clang fp contract(off)
    const float big = 3.402823466e+38f;
    if (!(fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big)) return 0;
    const float tx = (x - g.ox) / g.leaf, ty = (y - g.oy) / g.leaf, tz = (z - g.oz) / g.leaf;
    if (!(tx >= 0.f && ty >= 0.f && tz >= 0.f)) return 0;
    const float fx = floorf(tx), fy = floorf(ty), fz = floorf(tz);
    if (fx >= INDEX_LIMIT || fy >= INDEX_LIMIT || fz >= INDEX_LIMIT) return 2;
    const float ex = tx - (fx + 0.5f), ey = ty - (fy + 0.5f), ez = tz - (fz + 0.5f);
    d = (ex * ex + ey * ey) + ez * ez;
    key = ((unsigned long long)(unsigned)fx << 42) | ((unsigned long long)(unsigned)fy << 21) | (unsigned long long)(unsigned)fz;
    return 1;
}

__device__ inline unsigned long long mix(unsigned long long h) {     // the finaliser of splitmix64; the result does not depend on it
    h ^= h >> 30; h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27; h *= 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}

__global__ __launch_bounds__(THREADS) void reset_kernel(ulonglong2* __restrict__ words, unsigned long long pairs, State* __restrict__ st) {
    const unsigned long long stride = (unsigned long long)gridDim.x * THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * THREADS + threadIdx.x; i < pairs; i += stride) words[i] = make_ulonglong2(EMPTY, EMPTY);
    if (blockIdx.x == 0 && threadIdx.x < STATE_WORDS) reinterpret_cast<unsigned*>(st)[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(THREADS) void insert_kernel(const float* __restrict__ ref, int n, int ref_ld, unsigned row0, Grid g,
                                                         unsigned long long* keys, unsigned long long* best, unsigned long long capacity, State* st) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n) return;
    const float* p = ref + (size_t)r * ref_ld;
    unsigned long long key;
    float d;
    const int kind = classify(p[0], p[1], p[2], g, key, d);
    if (kind == 2) __hip_atomic_store(&st->out_of_range, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (kind != 1) return;
    const unsigned long long packed = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(row0 + (unsigned)r);
    const unsigned long long mask = capacity - 1;
    unsigned long long slot = mix(key) & mask;
    for (unsigned long long it = 0; it < capacity; ++it, slot = (slot + 1) & mask) {
        if (it != 0 && __hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
        unsigned long long k = keys[slot];
        if (k == EMPTY) {
            k = atomicCAS(&keys[slot], EMPTY, key);
            if (k == EMPTY) {                                        // claimed
                k = key;
                if ((unsigned long long)atomicAdd(&st->used, 1u) + 1 > capacity / 2)
                    __hip_atomic_store(&st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (k == key) {
            if (packed < best[slot]) atomicMin(&best[slot], packed);
            return;
        }
    }
    __hip_atomic_store(&st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every slot holds another key
}

__global__ __launch_bounds__(THREADS) void mark_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ best,
                                                       unsigned long long capacity, uint8_t* __restrict__ keep, unsigned long long N, State* st) {
    const unsigned long long slot = (unsigned long long)blockIdx.x * THREADS + threadIdx.x;
    const bool occupied = slot < capacity && keys[slot] != EMPTY;
    if (occupied) {
        const unsigned long long row = best[slot] & 0xffffffffull;
        if (row < N) keep[row] = 1;
    }
    const int count = __popcll(__ballot(occupied));
    if ((threadIdx.x & 63) == 0 && count != 0) atomicAdd(&st->voxels, (unsigned)count);
}

inline hipError_t launch_reset(void* table, uint64_t capacity, hipStream_t s) {
    const unsigned long long pairs = capacity;                       // 2 * capacity words of 8 bytes, two to a store
    const unsigned blocks = (unsigned)((pairs + THREADS - 1) / THREADS < 4096 ? (pairs + THREADS - 1) / THREADS : 4096);
    hipLaunchKernelGGL(reset_kernel, dim3(blocks), dim3(THREADS), 0, s, static_cast<ulonglong2*>(table), pairs, state_of(table, capacity));
    return hipGetLastError();
}

inline hipError_t launch_insert(const float* ref, int n, int ref_ld, uint64_t row0, const Grid& g, void* table, uint64_t capacity, hipStream_t s) {
    hipLaunchKernelGGL(insert_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, ref, n, ref_ld, (unsigned)row0, g, keys_of(table),
                       best_of(table, capacity), (unsigned long long)capacity, state_of(table, capacity));
    return hipGetLastError();
}

inline hipError_t launch_mark(void* table, uint64_t capacity, uint8_t* keep, uint64_t N, hipStream_t s) {
    State* st = state_of(table, capacity);
    hipError_t e = hipMemsetAsync(keep, 0, (size_t)N, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(&st->voxels, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mark_kernel, dim3((unsigned)((capacity + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, keys_of(table), best_of(table, capacity),
                       (unsigned long long)capacity, keep, (unsigned long long)N, st);
    return hipGetLastError();
}

}  // namespace pcv
}  // namespace ma
