// What the kernels over the centrality handle's CSR share (graphstats.hip, cores.hip): the launch shape, the relaxed flag
// load of a kernel that may have nothing left to do, and the two bisections over a symmetric CSR with ascending rows.
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

inline int gs_blocks(int64_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(GS_MAX_BLOCKS, (items + GS_BLOCK - 1) / GS_BLOCK));
}
