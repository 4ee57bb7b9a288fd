// What the kernels over a CSR with ascending rows share (graphstats.hip, cores.hip, links.hip, and quality.hip through
// frontier_core.h): the launch shape, the relaxed flag load of a kernel that may have nothing left to do, the two
// bisections, the choice of the shorter of two rows, and the one-thread walk over their common entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#define GS_BLOCK 256
#define GS_MAX_BLOCKS 4096
#define GS_CHECK_EVERY 4   // component rounds / distance levels / peel rounds between two host reads of the flags

__device__ __forceinline__ int32_t gs_flag(const int32_t *f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

#define GS_GRID_LOOP(i, items) \
    for (int64_t i = (int64_t)blockIdx.x * GS_BLOCK + threadIdx.x; i < (items); i += (int64_t)gridDim.x * GS_BLOCK)

// first position in [lo, hi) whose entry is >= x
__device__ __forceinline__ int64_t gs_lower_bound(const int32_t *__restrict__ a, int64_t lo, int64_t hi, int32_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the row of arc e: the last u with ptr[u] <= e
__device__ __forceinline__ int32_t gs_arc_row(const int64_t *__restrict__ ptr, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return (int32_t)lo;
}

// The rows of two vertices, the shorter one first, for a walk over their common entries.
struct GsRows {
    int64_t sb, se, lb, le;
};

__device__ __forceinline__ GsRows gs_rows(const int64_t *__restrict__ ptr, int32_t u, int32_t v) {
    const int64_t ub = ptr[u], ue = ptr[u + 1], vb = ptr[v], ve = ptr[v + 1];
    const bool u_short = ue - ub <= ve - vb;
    return {u_short ? ub : vb, u_short ? ue : ve, u_short ? vb : ub, u_short ? ve : ue};
}

// The common entries of two ascending rows [sb, se) and [lb, le) of adj, the shorter one first: f(k, at) for every entry k
// of the short row that the long row holds, at position `at`.  One thread walks the whole short row and bisects the long
// one with a window that shrinks as both ascend: min(len) log(max len) steps.
template <class F>
__device__ __forceinline__ void gs_common_walk(const int32_t *__restrict__ adj, int64_t sb, int64_t se, int64_t lb, int64_t le, F f) {
    for (int64_t k = sb; k < se && lb < le; ++k) {
        const int32_t x = adj[k];
        lb = gs_lower_bound(adj, lb, le, x);
        if (lb < le && adj[lb] == x) f(k, lb);
    }
}

inline int gs_blocks(int64_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(GS_MAX_BLOCKS, (items + GS_BLOCK - 1) / GS_BLOCK));
}
