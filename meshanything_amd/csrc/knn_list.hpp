// The k-best list of the point-cloud neighbour searches (pc_normals.hpp: brute force; pc_grid.hpp: cell grid): K = 8, 16 or 32 slots in
// registers, ascending under the total order (d, index).  Every index is a compile-time constant, so nothing goes to scratch.  Both
// searches insert with this one piece of code: the k best under a total order are unique, so the two give the same list bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace ma {
namespace pcn {

constexpr int MAX_K = 32;

inline int slots_for(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

// (d, i) before (bd, bi) in the order of the lists
__device__ inline bool before(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// put (d, i) into the ascending list; the entry that falls off the end is dropped
template <int K>
__device__ inline void insert(float (&bd)[K], int (&bi)[K], float d, int i) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
        const bool lt = before(d, i, bd[s], bi[s]);
        const float td = bd[s];
        const int ti = bi[s];
        bd[s] = lt ? d : td;
        bi[s] = lt ? i : ti;
        d = lt ? td : d;
        i = lt ? ti : i;
    }
}

}  // namespace pcn
}  // namespace ma
