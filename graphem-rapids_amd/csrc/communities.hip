// Louvain communities and exact modularity on the GPU (include/graphem_hip.h "communities"; graphem-rapids_amd/
// communities.py), over the centrality handle's deduplicated symmetric CSR.  Every quantity is an integer, every device
// sum an integer atomic or reduction, and no floating-point number is compared: the labels are a pure function of the
// graph, the seed and the two caps.
//
// A level graph is a CSR with uint32 weights (absent on level 0: every weight is 1), int64 self weights and int64 weighted
// degrees k.  One round of a level:
//   cm_best_short_kernel   rows of 1 .. CM_SHORT entries, a group of CM_GROUP lanes per row: the row's (community, weight)
//                          pairs are staged in LDS, every lane combines the pairs of its own entries' communities by a
//                          scan of the staged row, and the group reduces (val, community) with shuffles.
//   cm_best_long_kernel    longer rows, a workgroup per row: an LDS hash table keyed by community (CM_LDS_SLOTS slots,
//                          at most CM_LDS_PROBES probes); a row with a community that finds no slot is appended to the
//                          spill list and left to
//   cm_best_spill_kernel   the same with a table in global memory, one slice per workgroup, as many slices as the
//                          memory budget allows (at least one).
//   cm_move_kernel         the mover test over the adjacency; writes the labels after the round and scatters k into T'.
//   cm_numerator_kernel    sum I' and sum T'^2.
// and one host read of {any target, sum I', sum T'^2}.  Aggregation: arcs -> (c(u), c(v)) keys, hipCUB radix sort and
// reduce-by-key, the diagonal into the self weights and the rest into the next level's CSR.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "cent_handle.h"

#define CM_BLOCK 256
#define CM_MAX_BLOCKS 4096
#define CM_GROUP 8                         // lanes per row in the group-per-row kernels
#define CM_GROUPS (CM_BLOCK / CM_GROUP)    // rows per workgroup and step
#define CM_SHORT 32                        // rows up to this many entries take the short kernel
#define CM_STAGE (CM_SHORT + 1)            // LDS stride of a staged row (odd: the groups of a wave fall on distinct banks)
#define CM_LDS_SLOTS 1024
#define CM_LDS_PROBES 16
#define CM_MAX_SLICES 256
#define CM_GOLDEN 0x9E3779B97F4A7C15ull

namespace {

typedef unsigned long long cm_u64;

// stats words of a round
enum { CM_ANY = 0, CM_SUM_I = 1, CM_SUM_T2 = 2, CM_SPILLED = 3, CM_STATS = 4 };
// words of a level's set-up
enum { CM_N_LONG = 0, CM_MAX_DEG = 1, CM_PREP = 2 };

struct CmGraph {
    int64_t n, M;
    const int64_t *ptr;
    const int32_t *adj;
    const uint32_t *wgt;    // NULL: every weight is 1
    const int64_t *self;    // NULL: every self weight is 0
    const int64_t *k;
};

__host__ __device__ __forceinline__ uint64_t cm_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ cm_u64 cm_word(const cm_u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ cm_u64 cm_max(cm_u64 a, cm_u64 b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t cm_weight(const CmGraph &g, int64_t e) { return g.wgt ? g.wgt[e] : 1u; }

// the better of two candidate moves: the larger val, the smaller community among equals; (INT64_MIN, INT32_MAX) is none
struct CmBest { int64_t val; int32_t d; };
__device__ __forceinline__ CmBest cm_none() { return CmBest{INT64_MIN, INT32_MAX}; }
__device__ __forceinline__ CmBest cm_better(CmBest a, CmBest b) {
    return (b.val > a.val || (b.val == a.val && b.d < a.d)) ? b : a;
}
__device__ __forceinline__ CmBest cm_shfl_xor(CmBest a, int mask) {
    return CmBest{(int64_t)__shfl_xor((long long)a.val, mask), __shfl_xor(a.d, mask)};
}

__device__ __forceinline__ void cm_store_target(int64_t u, int32_t cu, CmBest best, int64_t stay, int32_t *target, cm_u64 *stats) {
    const bool go = best.d != INT32_MAX && best.val > stay;
    target[u] = go ? best.d : cu;
    if (go && cm_word(&stats[CM_ANY]) == 0) stats[CM_ANY] = 1;
}

#define CM_GRID_LOOP(i, items) \
    for (int64_t i = (int64_t)blockIdx.x * CM_BLOCK + threadIdx.x; i < (items); i += (int64_t)gridDim.x * CM_BLOCK)

// ---- level set-up ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_BLOCK) void cm_degree_kernel(int64_t n, const int64_t *__restrict__ ptr, int64_t *k) {
    CM_GRID_LOOP(u, n) k[u] = ptr[u + 1] - ptr[u];
}

// singletons, T = k, the list of long rows and the longest row
__global__ __launch_bounds__(CM_BLOCK) void cm_level_init_kernel(CmGraph g, int32_t *c, cm_u64 *T, int32_t *long_rows, cm_u64 *prep) {
    CM_GRID_LOOP(u, g.n) {
        c[u] = (int32_t)u;
        T[u] = (cm_u64)g.k[u];
        const int64_t deg = g.ptr[u + 1] - g.ptr[u];
        if (deg > CM_SHORT) {
            long_rows[atomicAdd(&prep[CM_N_LONG], 1ull)] = (int32_t)u;
            atomicMax(&prep[CM_MAX_DEG], (cm_u64)deg);
        }
    }
}

// ---- best moves -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_BLOCK) void cm_best_short_kernel(CmGraph g, const int32_t *__restrict__ c, const cm_u64 *__restrict__ T,
                                                                 int32_t *target, cm_u64 *stats) {
    __shared__ int32_t s_comm[CM_GROUPS * CM_STAGE];
    __shared__ uint32_t s_wgt[CM_GROUPS * CM_STAGE];
    const int grp = threadIdx.x / CM_GROUP, lane = threadIdx.x % CM_GROUP;
    int32_t *comm = s_comm + grp * CM_STAGE;
    uint32_t *wt = s_wgt + grp * CM_STAGE;
    for (int64_t base = (int64_t)blockIdx.x * CM_GROUPS; base < g.n; base += (int64_t)gridDim.x * CM_GROUPS) {
        const int64_t u = base + grp;
        int64_t beg = 0;
        int deg = -1;   // -1: no row of this kernel's (past the end, or a long row)
        if (u < g.n) {
            beg = g.ptr[u];
            const int64_t d = g.ptr[u + 1] - beg;
            deg = d <= CM_SHORT ? (int)d : -1;
        }
        for (int j = lane; j < deg; j += CM_GROUP) {
            comm[j] = c[g.adj[beg + j]];
            wt[j] = cm_weight(g, beg + j);
        }
        __syncthreads();
        const int32_t cu = deg >= 0 ? c[u] : 0;
        CmBest best = cm_none();
        cm_u64 w_own = 0;
        int64_t ku = 0;
        if (deg > 0) {
            ku = g.k[u];
            for (int j = lane; j < deg; j += CM_GROUP) {
                const int32_t d = comm[j];
                cm_u64 W = 0;
                bool first = true;
                for (int i = 0; i < deg; ++i) {
                    if (comm[i] != d) continue;
                    W += wt[i];
                    if (i < j) first = false;
                }
                if (d == cu) w_own = W;
                else if (first) best = cm_better(best, CmBest{g.M * (int64_t)W - ku * (int64_t)T[d], d});
            }
        }
#pragma unroll
        for (int m = 1; m < CM_GROUP; m <<= 1) {
            best = cm_better(best, cm_shfl_xor(best, m));
            w_own = cm_max(w_own, (cm_u64)__shfl_xor(w_own, m));
        }
        if (lane == 0 && deg >= 0) {
            const int64_t stay = g.M * (int64_t)w_own - ku * ((int64_t)T[cu] - ku);
            cm_store_target(u, cu, deg > 0 ? best : cm_none(), stay, target, stats);
        }
        __syncthreads();
    }
}

// The reduction of a workgroup's candidates and the store of the row's target; every thread of the workgroup calls it.
__device__ __forceinline__ void cm_block_target(const CmGraph &g, int64_t u, int32_t cu, CmBest best, cm_u64 w_own, const cm_u64 *T,
                                                int32_t *target, cm_u64 *stats, CmBest *s_best, cm_u64 *s_own) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        best = cm_better(best, cm_shfl_xor(best, m));
        w_own = cm_max(w_own, (cm_u64)__shfl_xor(w_own, m));
    }
    if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = best; s_own[threadIdx.x >> 6] = w_own; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CM_BLOCK / 64; ++w) { best = cm_better(best, s_best[w]); w_own = cm_max(w_own, s_own[w]); }
        const int64_t ku = g.k[u];
        const int64_t stay = g.M * (int64_t)w_own - ku * ((int64_t)T[cu] - ku);
        cm_store_target(u, cu, best, stay, target, stats);
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t cm_hash(int32_t d) { return (uint32_t)d * 0x9E3779B1u; }

__global__ __launch_bounds__(CM_BLOCK) void cm_best_long_kernel(CmGraph g, const int32_t *__restrict__ c, const cm_u64 *__restrict__ T,
                                                                const int32_t *__restrict__ long_rows, int64_t n_long, int32_t *target,
                                                                int32_t *spill_rows, cm_u64 *stats) {
    __shared__ int32_t s_key[CM_LDS_SLOTS];
    __shared__ cm_u64 s_val[CM_LDS_SLOTS];
    __shared__ CmBest s_best[CM_BLOCK / 64];
    __shared__ cm_u64 s_own[CM_BLOCK / 64];
    __shared__ int s_overflow;
    for (int64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int64_t u = long_rows[i];
        for (int t = threadIdx.x; t < CM_LDS_SLOTS; t += CM_BLOCK) { s_key[t] = -1; s_val[t] = 0; }
        if (threadIdx.x == 0) s_overflow = 0;
        __syncthreads();
        const int64_t beg = g.ptr[u], end = g.ptr[u + 1];
        for (int64_t e = beg + threadIdx.x; e < end; e += CM_BLOCK) {
            const int32_t d = c[g.adj[e]];
            uint32_t slot = cm_hash(d) >> 22;   // CM_LDS_SLOTS = 2^10
            int p = 0;
            for (; p < CM_LDS_PROBES; ++p, slot = (slot + 1) & (CM_LDS_SLOTS - 1)) {
                const int32_t seen = atomicCAS(&s_key[slot], -1, d);
                if (seen == -1 || seen == d) { atomicAdd(&s_val[slot], (cm_u64)cm_weight(g, e)); break; }
            }
            if (p == CM_LDS_PROBES) s_overflow = 1;
        }
        __syncthreads();
        if (s_overflow) {   // uniform: read after the barrier
            if (threadIdx.x == 0) spill_rows[atomicAdd(&stats[CM_SPILLED], 1ull)] = (int32_t)u;
            __syncthreads();
            continue;
        }
        const int32_t cu = c[u];
        const int64_t ku = g.k[u];
        CmBest best = cm_none();
        cm_u64 w_own = 0;
        for (int t = threadIdx.x; t < CM_LDS_SLOTS; t += CM_BLOCK) {
            const int32_t d = s_key[t];
            if (d < 0) continue;
            if (d == cu) w_own = s_val[t];
            else best = cm_better(best, CmBest{g.M * (int64_t)s_val[t] - ku * (int64_t)T[d], d});
        }
        cm_block_target(g, u, cu, best, w_own, T, target, stats, s_best, s_own);
    }
}

// slots: a power of two >= 2 * the longest row, so a probe sequence always ends
__global__ __launch_bounds__(CM_BLOCK) void cm_best_spill_kernel(CmGraph g, const int32_t *__restrict__ c, const cm_u64 *__restrict__ T,
                                                                 const int32_t *spill_rows, int32_t *target, int32_t *keys, cm_u64 *vals,
                                                                 int64_t slots, int shift, cm_u64 *stats) {
    __shared__ CmBest s_best[CM_BLOCK / 64];
    __shared__ cm_u64 s_own[CM_BLOCK / 64];
    const int64_t n_spilled = (int64_t)cm_word(&stats[CM_SPILLED]);
    int32_t *key = keys + (int64_t)blockIdx.x * slots;
    cm_u64 *val = vals + (int64_t)blockIdx.x * slots;
    for (int64_t i = blockIdx.x; i < n_spilled; i += gridDim.x) {
        const int64_t u = spill_rows[i];
        for (int64_t t = threadIdx.x; t < slots; t += CM_BLOCK) {
            __hip_atomic_store(&key[t], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&val[t], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        __syncthreads();
        const int64_t beg = g.ptr[u], end = g.ptr[u + 1];
        for (int64_t e = beg + threadIdx.x; e < end; e += CM_BLOCK) {
            const int32_t d = c[g.adj[e]];
            int64_t slot = shift < 32 ? (int64_t)(cm_hash(d) >> shift) : 0;
            for (int64_t p = 0; p < slots; ++p, slot = (slot + 1) & (slots - 1)) {
                const int32_t seen = atomicCAS(&key[slot], -1, d);
                if (seen == -1 || seen == d) { atomicAdd(&val[slot], (cm_u64)cm_weight(g, e)); break; }
            }
        }
        __threadfence();
        __syncthreads();
        const int32_t cu = c[u];
        const int64_t ku = g.k[u];
        CmBest best = cm_none();
        cm_u64 w_own = 0;
        for (int64_t t = threadIdx.x; t < slots; t += CM_BLOCK) {
            const int32_t d = __hip_atomic_load(&key[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d < 0) continue;
            const cm_u64 W = cm_word(&val[t]);
            if (d == cu) w_own = W;
            else best = cm_better(best, CmBest{g.M * (int64_t)W - ku * (int64_t)T[d], d});
        }
        cm_block_target(g, u, cu, best, w_own, T, target, stats, s_best, s_own);
    }
}

// ---- movers and the numerator ---------------------------------------------------------------------------------------
// c2 = the labels after the round; T2 (zeroed) += k at the new label
__global__ __launch_bounds__(CM_BLOCK) void cm_move_kernel(CmGraph g, const int32_t *__restrict__ c, const int32_t *__restrict__ target,
                                                           uint64_t prio_base, uint64_t round_bits, int32_t *c2, cm_u64 *T2) {
    const int grp = threadIdx.x / CM_GROUP, lane = threadIdx.x % CM_GROUP;
    // the trip count is the workgroup's, so that every lane of a wave reaches the shuffles
    for (int64_t base = (int64_t)blockIdx.x * CM_GROUPS; base < g.n; base += (int64_t)gridDim.x * CM_GROUPS) {
        const int64_t u = base + grp;
        const bool live = u < g.n;
        int32_t cu = 0, tu = 0;
        int blocked = 0;
        if (live) { cu = c[u]; tu = target[u]; }
        if (live && tu != cu) {
            const uint64_t pu = cm_mix(prio_base ^ (round_bits | (uint64_t)u));
            const int64_t beg = g.ptr[u], end = g.ptr[u + 1];
            for (int64_t e = beg + lane; e < end; e += CM_GROUP) {
                const int32_t v = g.adj[e];
                if (target[v] == c[v]) continue;
                const uint64_t pv = cm_mix(prio_base ^ (round_bits | (uint64_t)v));
                if (pv > pu || (pv == pu && v > u)) blocked = 1;
            }
        }
#pragma unroll
        for (int m = 1; m < CM_GROUP; m <<= 1) blocked |= __shfl_xor(blocked, m);
        if (live && lane == 0) {
            const int32_t nc = blocked ? cu : tu;
            c2[u] = nc;
            atomicAdd(&T2[nc], (cm_u64)g.k[u]);
        }
    }
}

// stats[CM_SUM_I] += the self weights and the weights of the arcs inside a community; stats[CM_SUM_T2] += T^2
__global__ __launch_bounds__(CM_BLOCK) void cm_numerator_kernel(CmGraph g, const int32_t *__restrict__ c, const cm_u64 *__restrict__ T,
                                                                cm_u64 *stats) {
    __shared__ cm_u64 s_sum[2][CM_BLOCK / 64];
    const int lane = threadIdx.x % CM_GROUP;
    cm_u64 inside = 0, squares = 0;
    for (int64_t u = ((int64_t)blockIdx.x * CM_BLOCK + threadIdx.x) / CM_GROUP; u < g.n; u += (int64_t)gridDim.x * CM_GROUPS) {
        const int32_t cu = c[u];
        const int64_t beg = g.ptr[u], end = g.ptr[u + 1];
        for (int64_t e = beg + lane; e < end; e += CM_GROUP)
            if (c[g.adj[e]] == cu) inside += cm_weight(g, e);
        if (lane == 0) {
            if (g.self) inside += (cm_u64)g.self[u];
            const cm_u64 t = T[u];
            squares += t * t;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        inside += (cm_u64)__shfl_xor(inside, m);
        squares += (cm_u64)__shfl_xor(squares, m);
    }
    if ((threadIdx.x & 63) == 0) { s_sum[0][threadIdx.x >> 6] = inside; s_sum[1][threadIdx.x >> 6] = squares; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CM_BLOCK / 64; ++w) { inside += s_sum[0][w]; squares += s_sum[1][w]; }
        if (inside) atomicAdd(&stats[CM_SUM_I], inside);
        if (squares) atomicAdd(&stats[CM_SUM_T2], squares);
    }
}

__global__ __launch_bounds__(CM_BLOCK) void cm_scatter_T_kernel(int64_t n, const int32_t *__restrict__ c, const int64_t *__restrict__ k,
                                                                cm_u64 *T) {
    CM_GRID_LOOP(u, n) if (k[u]) atomicAdd(&T[c[u]], (cm_u64)k[u]);
}

// ---- aggregation ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_BLOCK) void cm_used_kernel(int64_t n, const int32_t *__restrict__ c, int32_t *used) {
    CM_GRID_LOOP(u, n) used[c[u]] = 1;
}

// comp[u] = the coarse vertex of u; the coarse k and the vertices' share of the coarse self weights
__global__ __launch_bounds__(CM_BLOCK) void cm_coarse_vertex_kernel(CmGraph g, const int32_t *__restrict__ c, const int32_t *__restrict__ used,
                                                                    const int32_t *__restrict__ rank, const cm_u64 *__restrict__ T,
                                                                    int32_t *comp, int64_t *k2, cm_u64 *self2) {
    CM_GRID_LOOP(u, g.n) {
        const int32_t a = rank[c[u]];
        comp[u] = a;
        if (used[u]) k2[rank[u]] = (int64_t)T[u];
        if (g.self && g.self[u]) atomicAdd(&self2[a], (cm_u64)g.self[u]);
    }
}

__global__ __launch_bounds__(CM_BLOCK) void cm_arc_key_kernel(CmGraph g, const int32_t *__restrict__ comp, int bits, uint64_t *keys, uint32_t *vals) {
    const int lane = threadIdx.x % CM_GROUP;
    for (int64_t u = ((int64_t)blockIdx.x * CM_BLOCK + threadIdx.x) / CM_GROUP; u < g.n; u += (int64_t)gridDim.x * CM_GROUPS) {
        const uint64_t a = (uint64_t)comp[u] << bits;
        const int64_t beg = g.ptr[u], end = g.ptr[u + 1];
        for (int64_t e = beg + lane; e < end; e += CM_GROUP) {
            keys[e] = a | (uint64_t)comp[g.adj[e]];
            vals[e] = cm_weight(g, e);
        }
    }
}

// a run (a, a) goes to self2[a]; a run (a, b) is one arc of row a
__global__ __launch_bounds__(CM_BLOCK) void cm_run_count_kernel(int64_t runs, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sums,
                                                                int bits, int32_t *is_arc, cm_u64 *row_count, cm_u64 *self2) {
    CM_GRID_LOOP(j, runs) {
        const uint64_t a = keys[j] >> bits, b = keys[j] & ((1ull << bits) - 1);
        is_arc[j] = a != b;
        if (a == b) atomicAdd(&self2[a], (cm_u64)sums[j]);
        else atomicAdd(&row_count[a], 1ull);
    }
}

__global__ __launch_bounds__(CM_BLOCK) void cm_run_place_kernel(int64_t runs, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ sums,
                                                                int bits, const int32_t *__restrict__ is_arc, const int32_t *__restrict__ pos,
                                                                int32_t *adj2, uint32_t *wgt2) {
    CM_GRID_LOOP(j, runs) {
        if (!is_arc[j]) continue;
        adj2[pos[j]] = (int32_t)(keys[j] & ((1ull << bits) - 1));
        wgt2[pos[j]] = sums[j];
    }
}

// of_vertex[v] = the coarse vertex of original vertex v; low[a] = the smallest original id in a
__global__ __launch_bounds__(CM_BLOCK) void cm_project_kernel(int64_t n, const int32_t *__restrict__ comp, int32_t *of_vertex, int32_t *low) {
    CM_GRID_LOOP(v, n) {
        const int32_t a = comp[of_vertex[v]];
        of_vertex[v] = a;
        atomicMin(&low[a], (int32_t)v);
    }
}

__global__ __launch_bounds__(CM_BLOCK) void cm_iota_kernel(int64_t n, int32_t *x) {
    CM_GRID_LOOP(v, n) x[v] = (int32_t)v;
}

__global__ __launch_bounds__(CM_BLOCK) void cm_fill_kernel(int64_t n, int32_t *x, int32_t value) {
    CM_GRID_LOOP(v, n) x[v] = value;
}

__global__ __launch_bounds__(CM_BLOCK) void cm_label_kernel(int64_t n, const int32_t *__restrict__ of_vertex, const int32_t *__restrict__ low,
                                                            int32_t *label) {
    CM_GRID_LOOP(v, n) label[v] = low[of_vertex[v]];
}

// ---- host -----------------------------------------------------------------------------------------------------------
inline int cm_blocks(int64_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(CM_MAX_BLOCKS, (items + CM_BLOCK - 1) / CM_BLOCK));
}
inline int cm_group_blocks(int64_t rows) { return cm_blocks(rows * CM_GROUP); }

#define CM_ALLOC(buf, bytes)                                                                \
    do {                                                                                    \
        if (!(buf).alloc((size_t)(bytes))) {                                                \
            h->err = "hipMalloc failed for " #buf " (" + std::to_string((long long)(bytes)) + " bytes)"; \
            return GH_ERR_NOMEM;                                                            \
        }                                                                                   \
    } while (0)

template <class T> gh_status cm_exclusive_sum(gh_cent *h, const T *in, T *out, int64_t items) {
    size_t temp = 0;
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, in, out, (int)items, h->stream));
    gh_dev<char> tmp;
    CM_ALLOC(tmp, temp);
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, temp, in, out, (int)items, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));   // tmp goes out of scope
    return GH_OK;
}

// {sum I, sum T^2} of labelling c with community sums T, through the stats words
gh_status cm_numerator(gh_cent *h, const CmGraph &g, const int32_t *c, const cm_u64 *T, cm_u64 *d_stats, int64_t out[2]) {
    cm_u64 st[CM_STATS];
    GH_HIP(hipMemsetAsync(d_stats, 0, 8 * CM_STATS, h->stream));
    cm_numerator_kernel<<<dim3(cm_group_blocks(g.n)), dim3(CM_BLOCK), 0, h->stream>>>(g, c, T, d_stats);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(st, d_stats, 8 * CM_STATS, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    out[0] = (int64_t)st[CM_SUM_I];
    out[1] = (int64_t)st[CM_SUM_T2];
    return GH_OK;
}

struct CmWork {   // per-vertex state of the largest level (level 0), reused by the coarser ones
    gh_dev<int32_t> c, c2, target, long_rows, spill_rows, used, rank, comp;
    gh_dev<cm_u64> T, T2, stats, prep;
};

// The rounds of one level on graph g from singletons: w.c / w.T hold the last accepted labels afterwards.
gh_status cm_level_rounds(gh_cent *h, const CmGraph &g, CmWork &w, uint64_t seed, int32_t level, int32_t max_rounds, int64_t *N_out,
                          int32_t *rounds_out) {
    cm_u64 prep[CM_PREP];
    GH_HIP(hipMemsetAsync(w.prep.p, 0, 8 * CM_PREP, h->stream));
    cm_level_init_kernel<<<dim3(cm_blocks(g.n)), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c.p, w.T.p, w.long_rows.p, w.prep.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(prep, w.prep.p, 8 * CM_PREP, hipMemcpyDeviceToHost, h->stream));
    int64_t terms[2];
    GH_TRY_ST(cm_numerator(h, g, w.c.p, w.T.p, w.stats.p, terms));   // synchronises: prep is here as well
    int64_t N = g.M * terms[0] - terms[1];
    const int64_t n_long = (int64_t)prep[CM_N_LONG], max_deg = (int64_t)prep[CM_MAX_DEG];

    // the spill tables: slices of `slots` (key, value) pairs, as many as the budget holds
    gh_dev<int32_t> spill_keys;
    gh_dev<cm_u64> spill_vals;
    int64_t slots = 2, slices = 0;
    int shift = 31;
    if (n_long > 0) {
        while (slots < 2 * max_deg) { slots <<= 1; --shift; }
        slices = std::max<int64_t>(1, std::min<int64_t>({h->budget / (12 * slots), (int64_t)CM_MAX_SLICES, n_long}));
        CM_ALLOC(spill_keys, 4 * slots * slices);
        CM_ALLOC(spill_vals, 8 * slots * slices);
    }
    const uint64_t base = cm_mix(seed + (uint64_t)level * CM_GOLDEN);
    const int group_grid = cm_group_blocks(g.n);
    int32_t rounds = 0, fails = 0;
    for (int32_t r = 0; r < max_rounds; ++r) {
        ++rounds;
        GH_HIP(hipMemsetAsync(w.stats.p, 0, 8 * CM_STATS, h->stream));
        GH_HIP(hipMemsetAsync(w.T2.p, 0, 8 * g.n, h->stream));
        cm_best_short_kernel<<<dim3(group_grid), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c.p, w.T.p, w.target.p, w.stats.p);
        if (n_long > 0) {
            cm_best_long_kernel<<<dim3((unsigned)std::min<int64_t>(n_long, CM_MAX_BLOCKS)), dim3(CM_BLOCK), 0, h->stream>>>(
                g, w.c.p, w.T.p, w.long_rows.p, n_long, w.target.p, w.spill_rows.p, w.stats.p);
            cm_best_spill_kernel<<<dim3((unsigned)slices), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c.p, w.T.p, w.spill_rows.p, w.target.p,
                                                                                          spill_keys.p, spill_vals.p, slots, shift, w.stats.p);
        }
        cm_move_kernel<<<dim3(group_grid), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c.p, w.target.p, base, (uint64_t)r << 32, w.c2.p, w.T2.p);
        cm_numerator_kernel<<<dim3(group_grid), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c2.p, w.T2.p, w.stats.p);
        GH_LAUNCH_CHECK();
        cm_u64 st[CM_STATS];
        GH_HIP(hipMemcpyAsync(st, w.stats.p, 8 * CM_STATS, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (!st[CM_ANY]) break;
        const int64_t N2 = g.M * (int64_t)st[CM_SUM_I] - (int64_t)st[CM_SUM_T2];
        if (N2 > N) {
            N = N2;
            fails = 0;
            std::swap(w.c, w.c2);
            std::swap(w.T, w.T2);
        } else if (++fails == 2) {
            break;
        }
    }
    *N_out = N;
    *rounds_out = rounds;
    return GH_OK;
}

// The coarse graph of labelling w.c on g into `next`; *n2 = its vertices (== g.n: nothing merged, `next` is not built),
// w.comp = the coarse vertex of every vertex of g.
gh_status cm_aggregate(gh_cent *h, const CmGraph &g, int64_t arcs, CmWork &w, cent_level_graph &next, int64_t *n2, int64_t *arcs2) {
    const int64_t n = g.n;
    GH_HIP(hipMemsetAsync(w.used.p, 0, 4 * n, h->stream));
    cm_used_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, w.c.p, w.used.p);
    GH_LAUNCH_CHECK();
    GH_TRY_ST(cm_exclusive_sum(h, w.used.p, w.rank.p, n));
    int32_t tail[2];
    GH_HIP(hipMemcpyAsync(&tail[0], w.used.p + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(&tail[1], w.rank.p + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    const int64_t m = (int64_t)tail[0] + tail[1];
    *n2 = m;
    if (m == n) return GH_OK;

    CM_ALLOC(next.k, 8 * m);
    CM_ALLOC(next.self, 8 * m);
    CM_ALLOC(next.ptr, 8 * (m + 1));
    GH_HIP(hipMemsetAsync(next.self.p, 0, 8 * m, h->stream));
    GH_HIP(hipMemsetAsync(next.ptr.p, 0, 8 * (m + 1), h->stream));
    cm_coarse_vertex_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(g, w.c.p, w.used.p, w.rank.p, w.T.p, w.comp.p, next.k.p,
                                                                                (cm_u64 *)next.self.p);
    GH_LAUNCH_CHECK();
    *arcs2 = 0;
    if (arcs == 0) {
        CM_ALLOC(next.adj, 0);
        CM_ALLOC(next.wgt, 0);
        return GH_OK;
    }
    int bits = 1;
    while ((1ll << bits) < m) ++bits;
    gh_dev<uint64_t> keys, keys_alt, run_keys;
    gh_dev<uint32_t> vals, vals_alt, run_sums;
    gh_dev<int32_t> is_arc, pos, d_runs;
    gh_dev<char> tmp;
    CM_ALLOC(keys, 8 * arcs);
    CM_ALLOC(keys_alt, 8 * arcs);
    CM_ALLOC(vals, 4 * arcs);
    CM_ALLOC(vals_alt, 4 * arcs);
    CM_ALLOC(d_runs, 4);
    cm_arc_key_kernel<<<dim3(cm_group_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(g, w.comp.p, bits, keys.p, vals.p);
    GH_LAUNCH_CHECK();
    hipcub::DoubleBuffer<uint64_t> kb(keys.p, keys_alt.p);
    hipcub::DoubleBuffer<uint32_t> vb(vals.p, vals_alt.p);
    size_t temp = 0;
    GH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp, kb, vb, (int)arcs, 0, 2 * bits, h->stream));
    CM_ALLOC(tmp, temp);
    GH_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, temp, kb, vb, (int)arcs, 0, 2 * bits, h->stream));
    // the runs go into the buffers the sort left free
    uint64_t *rk = kb.Alternate();
    uint32_t *rs = vb.Alternate();
    size_t temp2 = 0;
    GH_HIP(hipcub::DeviceReduce::ReduceByKey(nullptr, temp2, kb.Current(), rk, vb.Current(), rs, d_runs.p, hipcub::Sum(), (int)arcs, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));   // the sort is done with tmp
    CM_ALLOC(tmp, temp2);
    GH_HIP(hipcub::DeviceReduce::ReduceByKey(tmp.p, temp2, kb.Current(), rk, vb.Current(), rs, d_runs.p, hipcub::Sum(), (int)arcs, h->stream));
    int32_t runs = 0;
    GH_HIP(hipMemcpyAsync(&runs, d_runs.p, 4, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));

    CM_ALLOC(is_arc, 4 * (int64_t)runs);
    CM_ALLOC(pos, 4 * (int64_t)runs);
    CM_ALLOC(next.adj, 4 * (int64_t)runs);
    CM_ALLOC(next.wgt, 4 * (int64_t)runs);
    gh_dev<cm_u64> row_count;
    CM_ALLOC(row_count, 8 * (m + 1));
    GH_HIP(hipMemsetAsync(row_count.p, 0, 8 * (m + 1), h->stream));
    cm_run_count_kernel<<<dim3(cm_blocks(runs)), dim3(CM_BLOCK), 0, h->stream>>>(runs, rk, rs, bits, is_arc.p, row_count.p, (cm_u64 *)next.self.p);
    GH_LAUNCH_CHECK();
    GH_TRY_ST(cm_exclusive_sum(h, is_arc.p, pos.p, (int64_t)runs));
    GH_TRY_ST(cm_exclusive_sum(h, (const int64_t *)row_count.p, next.ptr.p, m + 1));
    cm_run_place_kernel<<<dim3(cm_blocks(runs)), dim3(CM_BLOCK), 0, h->stream>>>(runs, rk, rs, bits, is_arc.p, pos.p, next.adj.p, next.wgt.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(arcs2, next.ptr.p + m, 8, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

gh_status cm_louvain(gh_cent *h, uint64_t seed, int32_t max_levels, int32_t max_rounds, int32_t *labels, int32_t *n_levels,
                     int64_t *numerators, int64_t *n_communities, int32_t *rounds) {
    const int64_t n = h->n, M = 2 * h->edges;
    CmWork w;
    gh_dev<int32_t> of_vertex, low, d_label;
    CM_ALLOC(w.c, 4 * n); CM_ALLOC(w.c2, 4 * n); CM_ALLOC(w.target, 4 * n);
    CM_ALLOC(w.long_rows, 4 * n); CM_ALLOC(w.spill_rows, 4 * n);
    CM_ALLOC(w.used, 4 * n); CM_ALLOC(w.rank, 4 * n); CM_ALLOC(w.comp, 4 * n);
    CM_ALLOC(w.T, 8 * n); CM_ALLOC(w.T2, 8 * n); CM_ALLOC(w.stats, 8 * CM_STATS); CM_ALLOC(w.prep, 8 * CM_PREP);
    CM_ALLOC(of_vertex, 4 * n); CM_ALLOC(low, 4 * n); CM_ALLOC(d_label, 4 * n);
    CM_ALLOC(h->lv[0].k, 8 * n);
    cm_degree_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, h->lv[0].k.p);
    cm_iota_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, of_vertex.p);
    GH_LAUNCH_CHECK();
    CmGraph g{n, M, h->d_ptr.p, h->d_adj.p, nullptr, nullptr, h->lv[0].k.p};
    int64_t arcs = M;
    *n_levels = 0;
    for (int32_t level = 0; level < max_levels; ++level) {
        int64_t N = 0, m = 0, arcs2 = 0;
        int32_t rr = 0;
        GH_TRY_ST(cm_level_rounds(h, g, w, seed, level, max_rounds, &N, &rr));
        cent_level_graph &next = h->lv[(level + 1) & 1];
        GH_TRY_ST(cm_aggregate(h, g, arcs, w, next, &m, &arcs2));
        const bool merged = m < g.n;
        if (!merged && level > 0) break;
        int32_t *row = labels + (int64_t)level * n;
        if (merged) {
            cm_fill_kernel<<<dim3(cm_blocks(m)), dim3(CM_BLOCK), 0, h->stream>>>(m, low.p, INT32_MAX);
            cm_project_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, w.comp.p, of_vertex.p, low.p);
            cm_label_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, of_vertex.p, low.p, d_label.p);
        } else {
            cm_iota_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, d_label.p);
        }
        GH_LAUNCH_CHECK();
        GH_HIP(hipMemcpyAsync(row, d_label.p, 4 * n, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        numerators[level] = N;
        n_communities[level] = m;
        rounds[level] = rr;
        *n_levels = level + 1;
        if (!merged) break;
        g = CmGraph{m, M, next.ptr.p, next.adj.p, next.wgt.p, next.self.p, next.k.p};
        arcs = arcs2;
    }
    return GH_OK;
}

gh_status cm_check(gh_cent *h) {
    if (h->edges > (1ll << 30)) { h->err = "communities need a graph of at most 2^30 edges"; return GH_ERR_INVALID; }
    if (2 * h->edges > (int64_t)INT32_MAX) { h->err = "the aggregation sort takes at most 2^31 - 1 arcs"; return GH_ERR_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    return GH_OK;
}

gh_status cm_modularity(gh_cent *h, const int32_t *labels, int64_t out[3]) {
    const int64_t n = h->n;
    gh_dev<int32_t> c;
    gh_dev<cm_u64> T, stats;
    gh_dev<int64_t> k;
    CM_ALLOC(c, 4 * n); CM_ALLOC(T, 8 * n); CM_ALLOC(stats, 8 * CM_STATS); CM_ALLOC(k, 8 * n);
    GH_HIP(hipMemcpyAsync(c.p, labels, 4 * n, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemsetAsync(T.p, 0, 8 * n, h->stream));
    cm_degree_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, k.p);
    cm_scatter_T_kernel<<<dim3(cm_blocks(n)), dim3(CM_BLOCK), 0, h->stream>>>(n, c.p, k.p, T.p);
    GH_LAUNCH_CHECK();
    const CmGraph g{n, 2 * h->edges, h->d_ptr.p, h->d_adj.p, nullptr, nullptr, k.p};
    GH_TRY_ST(cm_numerator(h, g, c.p, T.p, stats.p, out));
    out[2] = g.M;
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_cent_modularity(gh_cent_handle h, const int32_t *labels, int64_t out[3]) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (!out || (!labels && h->n > 0)) { h->err = "labels and out must not be NULL"; return GH_ERR_INVALID; }
    for (int64_t v = 0; v < h->n; ++v)
        if (labels[v] < 0 || labels[v] >= h->n) { h->err = "label of vertex " + std::to_string(v) + " outside [0, n)"; return GH_ERR_INVALID; }
    GH_TRY_ST(cm_check(h));
    out[0] = out[1] = 0;
    out[2] = 2 * h->edges;
    if (h->n == 0) return GH_OK;
    const gh_status st = cm_modularity(h, labels, out);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}

extern "C" gh_status gh_cent_louvain(gh_cent_handle h, uint64_t seed, int32_t max_levels, int32_t max_rounds, int32_t *labels,
                                     int32_t *n_levels, int64_t *numerators, int64_t *n_communities, int32_t *rounds) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (max_levels < 1 || max_rounds < 1) { h->err = "max_levels and max_rounds must be >= 1"; return GH_ERR_INVALID; }
    if (!n_levels || !numerators || !n_communities || !rounds || (!labels && h->n > 0)) {
        h->err = "output arrays must not be NULL";
        return GH_ERR_INVALID;
    }
    GH_TRY_ST(cm_check(h));
    *n_levels = 0;
    if (h->n == 0) return GH_OK;
    const gh_status st = cm_louvain(h, seed, max_levels, max_rounds, labels, n_levels, numerators, n_communities, rounds);
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    h->lv[0].reset();
    h->lv[1].reset();
    return st;
}
