// Monte Carlo Independent Cascade on the GPU (include/graphem_hip.h "influence"; graphem-rapids_amd/influence.py).
//
// Trials are bit-sliced: word w of a (set, vertex) entry holds trials 64w .. 64w+63, and lane t of a wave evaluates the coin
// of trial 64w + t, so one __ballot gives the live mask of an arc for 64 trials.  Coins are never stored: they are
// recomputed from the counter-based hash (header), with mix(seed + t * G) computed once per lane and work item.
//
// A BFS level (round r, from the frontier of round r - 1) is two launches:
//   ic_push_kernel / ic_pull_kernel  next words.  Both are launched; each reads the frontier's entry count on the device
//                                    and only one does work (pull from `pull_min` entries on, Beamer-style), so the host
//                                    never waits for a level.  push: a wave per frontier (entry, word), out-arcs in order,
//                                    ONE 8-byte atomicOr per arc that reaches a new trial (the ballot aggregates the wave;
//                                    lane q does arc q's memory work, 64 arcs at once).
//                                    pull: a wave per unvisited (entry, word) of the whole state, in-arcs in order until
//                                    every unvisited trial is reached, one plain store.  An entry that gains a bit is
//                                    appended to the next frontier list once (per-entry round stamp).
//   ic_advance_kernel                visited |= next over the new list (each entry joins the `touched` list the first time),
//                                    clears the old frontier's words, zeroes the third counter of the ring of three.
// The host reads the frontier count back every IC_CHECK_EVERY levels only.  Counting (ic_count_kernel) and clearing
// (ic_reset_kernel) walk the touched list, never the dense state, so a chunk costs what its cascades reach.
//
// Probabilities: one threshold for the whole graph (gh_ic_spread, gh_ic_rr_sample), or one per arc from two arrays aligned
// with the CSR slots (gh_ic_set_arc_probabilities; gh_ic_spread_arcs, gh_ic_rr_sample_arcs run the ARC instantiations of
// push and pull).  The coin and its key are the same in both.
//
// Linear Threshold (gh_ic_set_lt_weights; gh_ic_spread_lt, gh_ic_rr_sample_lt): the same levels with lt_push_kernel /
// lt_pull_kernel as the next-word launches.  In a trial every vertex selects at most one in-arc: the arc whose fixed-point
// interval [lo, hi) of the target's row holds the 32-bit pick of (trial, target).  Every CSR slot carries the (lo, hi) of
// its arc, in both CSRs, so a launch never looks into another row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "host_util.h"
#include "rr_handle.h"

#define IC_GOLDEN 0x9E3779B97F4A7C15ull
#define IC_BLOCK 256
#define IC_MAX_BLOCKS 2048
#define IC_CHECK_EVERY 4            // levels between two host reads of the frontier count
#define IC_PULL_DIV 16              // pull from (sets in chunk * n) / IC_PULL_DIV frontier entries on
#define IC_DEFAULT_BUDGET (1ll << 30)

namespace {

__host__ __device__ __forceinline__ uint64_t ic_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t ic_key(int32_t u, int32_t v, int directed) {
    const uint32_t a = directed ? (uint32_t)u : (uint32_t)min(u, v);
    const uint32_t b = directed ? (uint32_t)v : (uint32_t)max(u, v);
    return ((uint64_t)a << 32) | b;
}

__device__ __forceinline__ uint64_t ic_valid(int w, int W, int T) {
    const int r = T - 64 * w;
    return (w < W - 1 || r >= 64) ? ~0ull : ((1ull << r) - 1);
}

__device__ __forceinline__ int32_t uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uni64(uint64_t x) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return ((uint64_t)hi << 32) | lo;
}

struct IcLevel {
    const int64_t *out_ptr; const int32_t *out_adj;   // push: arcs u -> v by u
    const int64_t *in_ptr; const int32_t *in_adj;     // pull: arcs u -> v by v
    uint64_t *vis, *cur, *nxt;                        // (sets * n, W) words
    int32_t *mark;                                    // (sets * n) round stamp of the last append
    uint8_t *touched;                                 // (sets * n) entry is in the touched list
    const int32_t *cur_list; int32_t *nxt_list; int32_t *touch_list;
    const int32_t *cur_cnt; int32_t *nxt_cnt; int32_t *zero_cnt; int32_t *touch_cnt;
    int64_t n, pull_min, dense;                       // dense = sets * n * W
    uint64_t seed;
    const uint64_t *trial_tab;                        // REV: the trial of bit b of word w at [64 * w + b]
    uint32_t thr;
    int32_t W, T, directed, round;
    // ARC: the threshold of the arc in each slot of out_adj / in_adj.  Last, so that the scalar instantiations read every
    // other member where they always did.
    const uint32_t *out_thr, *in_thr;
    // LT: the interval (lo, hi) of the arc in each slot of out_adj / in_adj, within the row of the arc's original target
    const uint2 *out_iv, *in_iv;
};

// REV (reverse-reachable sets, gh_ic_rr_sample): the host swaps the two CSRs, so a level walks every arc backwards; the
// coin stays that of the original arc (the pair the other way round), and a lane's trial comes from the per-bit table.
template <bool REV> __device__ __forceinline__ uint64_t ic_lane_word(const IcLevel &a, int32_t w, int lane) {
    if constexpr (REV) return ic_mix(a.seed + a.trial_tab[64 * w + lane] * IC_GOLDEN);
    else return ic_mix(a.seed + (uint64_t)(64 * w + lane) * IC_GOLDEN);
}
template <bool REV> __device__ __forceinline__ uint64_t ic_arc_key(int32_t from, int32_t to, int directed) {
    if constexpr (REV) return ic_key(to, from, directed);
    else return ic_key(from, to, directed);
}

__device__ __forceinline__ void ic_append(const IcLevel &a, int32_t e) {   // one lane
    if (__hip_atomic_load(&a.mark[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.round) return;
    if (atomicExch(&a.mark[e], a.round) != a.round) a.nxt_list[atomicAdd(a.nxt_cnt, 1)] = e;
}

// ARC (per-arc probabilities, gh_ic_set_arc_probabilities): the threshold of an arc comes from the array aligned with the
// CSR slots -- loaded beside the neighbour id, broadcast with it -- instead of the one a.thr.
template <bool REV, bool ARC> __global__ __launch_bounds__(IC_BLOCK) void ic_push_kernel(IcLevel a) {
    const int64_t cnt = *a.cur_cnt;
    if (cnt == 0 || cnt >= a.pull_min) return;
    const int lane = threadIdx.x & 63;
    const int64_t items = cnt * a.W;
    const int64_t nwaves = (int64_t)gridDim.x * (IC_BLOCK / 64);
    for (int64_t i0 = ((int64_t)blockIdx.x * (IC_BLOCK / 64) + (threadIdx.x >> 6)) * 64; i0 < items; i0 += nwaves * 64) {
        const int64_t i = i0 + lane;
        int32_t e = 0, w = 0;
        uint64_t f = 0;
        if (i < items) {
            e = a.cur_list[i / a.W];
            w = (int32_t)(i % a.W);
            f = a.cur[(int64_t)e * a.W + w];
        }
        uint64_t todo = __ballot(f != 0);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int32_t ej = uni(__shfl(e, j)), wj = uni(__shfl(w, j));
            const uint64_t fj = uni64(__shfl(f, j));
            const int64_t s = ej / a.n;
            const int32_t u = (int32_t)(ej - s * a.n);
            const uint64_t h = ic_lane_word<REV>(a, wj, lane);
            const int64_t beg = a.out_ptr[u], end = a.out_ptr[u + 1];
            // 64 arcs at a time: the coins of arc q go to lane q as one live mask, then every lane does its arc's
            // memory work (visited load, atomicOr, append) in parallel instead of one lane arc after arc
            for (int64_t k0 = beg; k0 < end; k0 += 64) {
                const int32_t vk = k0 + lane < end ? a.out_adj[k0 + lane] : 0;
                uint32_t tk = 0;
                if constexpr (ARC) tk = k0 + lane < end ? a.out_thr[k0 + lane] : 0;
                const int m = (int)min((int64_t)64, end - k0);
                uint64_t mine = 0;
                for (int q = 0; q < m; ++q) {
                    const int32_t v = __builtin_amdgcn_readlane(vk, q);
                    const uint32_t thr = ARC ? (uint32_t)__builtin_amdgcn_readlane((int32_t)tk, q) : a.thr;
                    const uint64_t live = __ballot((uint32_t)(ic_mix(h ^ ic_arc_key<REV>(u, v, a.directed)) >> 40) < thr) & fj;
                    if (lane == q) mine = live;
                }
                if (mine) {
                    const int64_t ev = s * a.n + vk;
                    const uint64_t nw = mine & ~a.vis[ev * a.W + wj];
                    if (nw) {
                        atomicOr((unsigned long long *)&a.nxt[ev * a.W + wj], (unsigned long long)nw);
                        ic_append(a, (int32_t)ev);
                    }
                }
            }
        }
    }
}

template <bool REV, bool ARC> __global__ __launch_bounds__(IC_BLOCK) void ic_pull_kernel(IcLevel a) {
    const int64_t cnt = *a.cur_cnt;
    if (cnt == 0 || cnt < a.pull_min) return;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (IC_BLOCK / 64);
    for (int64_t i0 = ((int64_t)blockIdx.x * (IC_BLOCK / 64) + (threadIdx.x >> 6)) * 64; i0 < a.dense; i0 += nwaves * 64) {
        const int64_t i = i0 + lane;   // word index: entry i / W, word i % W
        uint64_t unv = 0;
        if (i < a.dense) unv = ~a.vis[i] & ic_valid((int)(i % a.W), a.W, a.T);
        uint64_t todo = __ballot(unv != 0);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int64_t ij = (int64_t)uni64((uint64_t)(i0 + j));
            const uint64_t uj = uni64(__shfl(unv, j));
            const int32_t e = uni((int32_t)(ij / a.W)), wj = uni((int32_t)(ij % a.W));
            const int64_t s = e / a.n;
            const int32_t v = (int32_t)(e - s * a.n);
            const uint64_t *cw = a.cur + s * a.n * a.W + wj;
            uint64_t acc = 0, h = 0;
            bool have_h = false;
            const int64_t beg = a.in_ptr[v], end = a.in_ptr[v + 1];
            // 64 in-arcs at a time: lane q loads the frontier word of arc q's source, coins only for the nonzero ones
            for (int64_t k0 = beg; k0 < end && acc != uj; k0 += 64) {
                int32_t uk = 0;
                uint32_t tk = 0;
                uint64_t fk = 0;
                if (k0 + lane < end) {
                    uk = a.in_adj[k0 + lane];
                    if constexpr (ARC) tk = a.in_thr[k0 + lane];
                    fk = cw[(int64_t)uk * a.W] & uj;
                }
                uint64_t arcs = __ballot(fk != 0);
                while (arcs && acc != uj) {
                    const int q = __ffsll((unsigned long long)arcs) - 1;
                    arcs &= arcs - 1;
                    const int32_t u = __builtin_amdgcn_readlane(uk, q);
                    const uint64_t f = uni64(__shfl(fk, q)) & ~acc;
                    if (f == 0) continue;
                    if (!have_h) { h = ic_lane_word<REV>(a, wj, lane); have_h = true; }
                    const uint32_t thr = ARC ? (uint32_t)__builtin_amdgcn_readlane((int32_t)tk, q) : a.thr;
                    acc |= __ballot((uint32_t)(ic_mix(h ^ ic_arc_key<REV>(u, v, a.directed)) >> 40) < thr) & f;
                }
            }
            if (acc && lane == 0) {
                a.nxt[ij] = acc;
                ic_append(a, e);
            }
        }
    }
}

// ---- Linear Threshold ----------------------------------------------------------------------------------------------------
// pick(seed, t, v): the trial's word mixed with the self-loop key (v, v), which no arc coin has; the top 32 bits.
__device__ __forceinline__ uint32_t lt_pick(uint64_t h, int32_t v) {
    return (uint32_t)(ic_mix(h ^ (((uint64_t)(uint32_t)v << 32) | (uint32_t)v)) >> 32);
}

// The pick belongs to the arc's ORIGINAL target.  Forward push walks u's out-arcs, so the target is the neighbour: one mix
// per arc and lane, as the IC coin costs (a slot with an empty interval costs nothing).  Reverse push walks the arcs INTO u
// backwards, so the target is u itself: one pick per (entry, word), and a slot costs two compares against its (lo, hi),
// broadcast beside the neighbour id.
template <bool REV> __global__ __launch_bounds__(IC_BLOCK) void lt_push_kernel(IcLevel a) {
    const int64_t cnt = *a.cur_cnt;
    if (cnt == 0 || cnt >= a.pull_min) return;
    const int lane = threadIdx.x & 63;
    const int64_t items = cnt * a.W;
    const int64_t nwaves = (int64_t)gridDim.x * (IC_BLOCK / 64);
    for (int64_t i0 = ((int64_t)blockIdx.x * (IC_BLOCK / 64) + (threadIdx.x >> 6)) * 64; i0 < items; i0 += nwaves * 64) {
        const int64_t i = i0 + lane;
        int32_t e = 0, w = 0;
        uint64_t f = 0;
        if (i < items) {
            e = a.cur_list[i / a.W];
            w = (int32_t)(i % a.W);
            f = a.cur[(int64_t)e * a.W + w];
        }
        uint64_t todo = __ballot(f != 0);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int32_t ej = uni(__shfl(e, j)), wj = uni(__shfl(w, j));
            const uint64_t fj = uni64(__shfl(f, j));
            const int64_t s = ej / a.n;
            const int32_t u = (int32_t)(ej - s * a.n);
            const uint64_t h = ic_lane_word<REV>(a, wj, lane);
            uint32_t pk = 0;
            if constexpr (REV) pk = lt_pick(h, u);
            const int64_t beg = a.out_ptr[u], end = a.out_ptr[u + 1];
            for (int64_t k0 = beg; k0 < end; k0 += 64) {
                int32_t vk = 0;
                uint2 ck = make_uint2(0, 0);
                if (k0 + lane < end) {
                    vk = a.out_adj[k0 + lane];
                    ck = a.out_iv[k0 + lane];
                }
                const int m = (int)min((int64_t)64, end - k0);
                uint64_t mine = 0;
                for (int q = 0; q < m; ++q) {
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)ck.x, q);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)ck.y, q);
                    if (lo == hi) continue;   // a zero-weight arc: nobody selects it
                    if constexpr (!REV) pk = lt_pick(h, __builtin_amdgcn_readlane(vk, q));
                    const uint64_t live = __ballot(pk >= lo && pk < hi) & fj;
                    if (lane == q) mine = live;
                }
                if (mine) {
                    const int64_t ev = s * a.n + vk;
                    const uint64_t nw = mine & ~a.vis[ev * a.W + wj];
                    if (nw) {
                        atomicOr((unsigned long long *)&a.nxt[ev * a.W + wj], (unsigned long long)nw);
                        ic_append(a, (int32_t)ev);
                    }
                }
            }
        }
    }
}

// Forward pull walks the arcs into v, so v is the target: one pick per (entry, word), two compares per slot whose source is
// in the frontier.  The slots of v's row ascend in cumulative weight (the row IS the target's row), so after a batch whose
// last bound is c every trial with pick < c has had its one selected source looked at, and the row stops once no unvisited
// trial is left beyond that.  Reverse pull walks v's out-arcs backwards: the target is the neighbour, one mix per arc whose
// target is in the frontier.
template <bool REV> __global__ __launch_bounds__(IC_BLOCK) void lt_pull_kernel(IcLevel a) {
    const int64_t cnt = *a.cur_cnt;
    if (cnt == 0 || cnt < a.pull_min) return;
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (IC_BLOCK / 64);
    for (int64_t i0 = ((int64_t)blockIdx.x * (IC_BLOCK / 64) + (threadIdx.x >> 6)) * 64; i0 < a.dense; i0 += nwaves * 64) {
        const int64_t i = i0 + lane;   // word index: entry i / W, word i % W
        uint64_t unv = 0;
        if (i < a.dense) unv = ~a.vis[i] & ic_valid((int)(i % a.W), a.W, a.T);
        uint64_t todo = __ballot(unv != 0);
        while (todo) {
            const int j = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const int64_t ij = (int64_t)uni64((uint64_t)(i0 + j));
            const uint64_t uj = uni64(__shfl(unv, j));
            const int32_t e = uni((int32_t)(ij / a.W)), wj = uni((int32_t)(ij % a.W));
            const int64_t s = e / a.n;
            const int32_t v = (int32_t)(e - s * a.n);
            const uint64_t *cw = a.cur + s * a.n * a.W + wj;
            uint64_t acc = 0, h = 0;
            uint32_t pk = 0;
            bool have_h = false;
            const int64_t beg = a.in_ptr[v], end = a.in_ptr[v + 1];
            for (int64_t k0 = beg; k0 < end && acc != uj; k0 += 64) {
                int32_t uk = 0;
                uint2 ck = make_uint2(0, 0);
                uint64_t fk = 0;
                if (k0 + lane < end) {
                    uk = a.in_adj[k0 + lane];
                    ck = a.in_iv[k0 + lane];
                    if (ck.x != ck.y) fk = cw[(int64_t)uk * a.W] & uj;
                }
                uint64_t arcs = __ballot(fk != 0);
                while (arcs && acc != uj) {
                    const int q = __ffsll((unsigned long long)arcs) - 1;
                    arcs &= arcs - 1;
                    const uint64_t f = uni64(__shfl(fk, q)) & ~acc;
                    if (f == 0) continue;
                    if (!have_h) {
                        h = ic_lane_word<REV>(a, wj, lane);
                        if constexpr (!REV) pk = lt_pick(h, v);
                        have_h = true;
                    }
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)ck.x, q);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)ck.y, q);
                    if constexpr (REV) pk = lt_pick(h, __builtin_amdgcn_readlane(uk, q));
                    acc |= __ballot(pk >= lo && pk < hi) & f;
                }
                if constexpr (!REV) {
                    if (have_h) {
                        const int last = uni((int32_t)min((int64_t)64, end - k0)) - 1;
                        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int32_t)ck.y, last);
                        if ((uj & ~acc & ~__ballot(pk < c)) == 0) break;
                    }
                }
            }
            if (acc && lane == 0) {
                a.nxt[ij] = acc;
                ic_append(a, e);
            }
        }
    }
}

__global__ __launch_bounds__(IC_BLOCK) void ic_advance_kernel(IcLevel a) {
    const int64_t ncur = (int64_t)*a.cur_cnt * a.W, nnew = (int64_t)*a.nxt_cnt * a.W;
    const int64_t stride = (int64_t)gridDim.x * IC_BLOCK;
    const int64_t t0 = (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x;
    if (t0 == 0) *a.zero_cnt = 0;
    for (int64_t i = t0; i < ncur; i += stride) a.cur[(int64_t)a.cur_list[i / a.W] * a.W + i % a.W] = 0;
    for (int64_t i = t0; i < nnew; i += stride) {
        const int32_t e = a.nxt_list[i / a.W];
        const int64_t x = (int64_t)e * a.W + i % a.W;
        a.vis[x] |= a.nxt[x];
        if (i % a.W == 0 && !a.touched[e]) {
            a.touched[e] = 1;
            a.touch_list[atomicAdd(a.touch_cnt, 1)] = e;
        }
    }
}

// Round 0: the seed entries (unique, uploaded to list 0 and to the touched list) get every valid trial.
__global__ __launch_bounds__(IC_BLOCK) void ic_seed_kernel(const int32_t *__restrict__ seeds, int64_t count, int32_t W, int32_t T,
                                                          uint64_t *vis, uint64_t *cur, uint8_t *touched) {
    const int64_t i = (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x;
    if (i >= count * W) return;
    const int32_t e = seeds[i / W];
    const int w = (int)(i % W);
    const uint64_t m = ic_valid(w, W, T);
    vis[(int64_t)e * W + w] = m;
    cur[(int64_t)e * W + w] = m;
    if (w == 0) touched[e] = 1;
}

// counts[s][t] = reached vertices of set s in trial t.  A wave takes 64 touched entries and one word; lane t adds bit t of
// each and flushes its sum with one atomicAdd when the set changes (entries of one set are mostly contiguous).
__global__ __launch_bounds__(IC_BLOCK) void ic_count_kernel(const int32_t *__restrict__ touch_list, const int32_t *touch_cnt,
                                                           const uint64_t *__restrict__ vis, int64_t n, int32_t W, int32_t T,
                                                           int32_t *counts) {
    const int64_t cnt = *touch_cnt;
    const int lane = threadIdx.x & 63;
    const int64_t batches = (cnt + 63) / 64 * W;
    const int64_t nwaves = (int64_t)gridDim.x * (IC_BLOCK / 64);
    for (int64_t q = (int64_t)blockIdx.x * (IC_BLOCK / 64) + (threadIdx.x >> 6); q < batches; q += nwaves) {
        const int64_t b = q / W;
        const int w = (int)(q % W);
        const int64_t i = b * 64 + lane;
        int32_t s = -1;
        uint64_t x = 0;
        if (i < cnt) {
            const int32_t e = touch_list[i];
            s = (int32_t)(e / n);
            x = vis[(int64_t)e * W + w];
        }
        const int t = 64 * w + lane;
        int32_t cur_s = -1, acc = 0;
        for (int j = 0; j < 64; ++j) {
            const int32_t sj = __shfl(s, j);
            if (sj < 0) break;
            if (sj != cur_s) {
                if (acc && t < T) atomicAdd(&counts[(int64_t)cur_s * T + t], acc);
                cur_s = sj;
                acc = 0;
            }
            acc += (int32_t)((__shfl(x, j) >> lane) & 1);
        }
        if (acc && t < T) atomicAdd(&counts[(int64_t)cur_s * T + t], acc);
    }
}

__global__ __launch_bounds__(IC_BLOCK) void ic_reset_kernel(const int32_t *__restrict__ touch_list, const int32_t *touch_cnt,
                                                           int32_t W, uint64_t *vis, uint64_t *fa, uint64_t *fb, int32_t *mark,
                                                           uint8_t *touched) {
    const int64_t items = (int64_t)*touch_cnt * W;
    for (int64_t i = (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x; i < items; i += (int64_t)gridDim.x * IC_BLOCK) {
        const int32_t e = touch_list[i / W];
        const int64_t x = (int64_t)e * W + i % W;
        vis[x] = 0; fa[x] = 0; fb[x] = 0;
        if (i % W == 0) { mark[e] = 0; touched[e] = 0; }
    }
}

inline int ic_blocks(int64_t threads) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(IC_MAX_BLOCKS, (threads + IC_BLOCK - 1) / IC_BLOCK));
}

}  // namespace

struct gh_ic : gh_host {
    int64_t n = 0, arcs = 0;
    int directed = 0;
    gh_dev<int64_t> d_out_ptr, d_in_own_ptr;   // d_in_own_*: the by-target CSR of a directed graph
    gh_dev<int32_t> d_out_adj, d_in_own_adj;
    const int64_t *d_in_ptr = nullptr;          // not owned: d_in_own_*, or d_out_* for an undirected graph
    const int32_t *d_in_adj = nullptr;
    // per-arc thresholds (gh_ic_set_arc_probabilities): one per slot of d_out_adj / of the in-CSR; graph state, not budgeted
    std::vector<uint64_t> keys;                 // the canonical arc keys, ascending: what the setter resolves pairs against
    bool has_table = false;
    gh_dev<uint32_t> d_out_thr, d_in_thr;
    // Linear Threshold intervals (gh_ic_set_lt_weights): (lo, hi) per slot of d_out_adj / of the in-CSR; graph state of its
    // own beside the per-arc table, not budgeted
    bool has_lt = false;
    gh_dev<uint2> d_out_iv, d_in_iv;
    // chunk state, grown on demand
    int64_t cap_words = 0, cap_ents = 0, cap_counts = 0;
    gh_dev<uint64_t> d_vis, d_fa, d_fb;
    gh_dev<int32_t> d_mark, d_list0, d_list1, d_touch, d_counts, d_cnt;
    gh_dev<uint8_t> d_touched;
    // gh_ic_rr_sample: per-bit trials, counts, offsets and cursors of a chunk, the unsorted members, the scan / sort temp
    int64_t cap_rr_bits = 0, cap_rr_scatter = 0;
    gh_dev<uint64_t> d_rr_trials;
    gh_dev<int32_t> d_rr_count, d_rr_cursor, d_rr_scatter;
    gh_dev<int64_t> d_rr_off;
    gh_dev<char> d_rr_tmp;
};

static thread_local std::string g_ic_error;

namespace {

void ic_free_state(gh_ic *h) {
    h->d_vis.reset(); h->d_fa.reset(); h->d_fb.reset(); h->d_mark.reset(); h->d_list0.reset(); h->d_list1.reset();
    h->d_touch.reset(); h->d_counts.reset(); h->d_cnt.reset(); h->d_touched.reset();
    h->cap_words = h->cap_ents = h->cap_counts = 0;
}

// bytes of chunk state per seed set (the budget counts these)
int64_t ic_bytes_per_set(int64_t n, int W) { return n * (3 * 8 * (int64_t)W + 4 + 1 + 3 * 4); }

gh_status ic_reserve(gh_ic *h, int64_t sets, int32_t W, int32_t T) {
    // every chunk leaves the state all zero, so any layout that fits reuses it
    const int64_t words = sets * h->n * W, ents = sets * h->n;
    if (words <= h->cap_words && ents <= h->cap_ents && sets * T <= h->cap_counts) return GH_OK;
    ic_free_state(h);
    if (!h->d_vis.alloc(8 * words) || !h->d_fa.alloc(8 * words) || !h->d_fb.alloc(8 * words) || !h->d_mark.alloc(4 * ents) ||
        !h->d_touched.alloc(ents) || !h->d_list0.alloc(4 * ents) || !h->d_list1.alloc(4 * ents) || !h->d_touch.alloc(4 * ents) ||
        !h->d_counts.alloc(4 * sets * T) || !h->d_cnt.alloc(4 * 4)) {
        ic_free_state(h);
        h->err = "hipMalloc failed for " + std::to_string(sets) + " seed sets of chunk state";
        return GH_ERR_NOMEM;
    }
    // zero once; afterwards every chunk leaves the state zero behind it (ic_reset_kernel)
    for (auto [p, bytes] : {std::pair<void *, size_t>{h->d_vis.p, 8 * words}, {h->d_fa.p, 8 * words}, {h->d_fb.p, 8 * words},
                            {h->d_mark.p, 4 * ents}, {h->d_touched.p, (size_t)ents}})
        if (hipMemsetAsync(p, 0, bytes, h->stream) != hipSuccess) { h->err = "hipMemsetAsync failed"; return GH_ERR_HIP; }
    h->cap_words = words;
    h->cap_ents = ents;
    h->cap_counts = sets * T;
    return GH_OK;
}

// The levels of one chunk whose round 0 is in place (list 0, the touched list, their counts): push / pull / advance until
// the frontier is empty or max_hops levels have run.  REV: the CSRs swapped and the per-bit trial table (gh_ic_rr_sample).
template <bool REV, bool ARC> void ic_launch_level(const gh_ic *h, const IcLevel &a, int grid) {
    ic_push_kernel<REV, ARC><<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
    ic_pull_kernel<REV, ARC><<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
    ic_advance_kernel<<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
}
template <bool REV> void lt_launch_level(const gh_ic *h, const IcLevel &a, int grid) {
    lt_push_kernel<REV><<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
    lt_pull_kernel<REV><<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
    ic_advance_kernel<<<dim3(grid), dim3(IC_BLOCK), 0, h->stream>>>(a);
}

// The diffusion model of a call: the one threshold of p, the handle's per-arc table, or its Linear Threshold intervals.
struct IcProb {
    bool arc;
    uint32_t thr;   // !arc
    bool lt = false;
};

// What picks the model at an entry point: p for the scalar, and for p = NULL the table named here.
enum IcTable { IC_TABLE_ARCS, IC_TABLE_LT };

inline uint32_t ic_threshold(double p) { return (uint32_t)std::min(16777216.0, std::floor(p * 16777216.0 + 0.5)); }

// What the scalar and the per-arc entry points check of their probability argument.
gh_status ic_prob(gh_ic *h, const double *p, IcTable table, IcProb *out) {
    if (p) {
        if (!(*p >= 0.0 && *p <= 1.0)) { h->err = "p must be in [0, 1]"; return GH_ERR_INVALID; }
        *out = IcProb{false, ic_threshold(*p)};
    } else if (table == IC_TABLE_LT) {
        if (!h->has_lt) { h->err = "no Linear Threshold weights have been set (gh_ic_set_lt_weights)"; return GH_ERR_INVALID; }
        *out = IcProb{false, 0, true};
    } else {
        if (!h->has_table) { h->err = "no arc probabilities have been set (gh_ic_set_arc_probabilities)"; return GH_ERR_INVALID; }
        *out = IcProb{true, 0};
    }
    return GH_OK;
}

template <bool REV>
gh_status ic_run_levels(gh_ic *h, int64_t sets, int32_t W, int32_t T, uint64_t seed, IcProb prob, int32_t max_hops,
                        const uint64_t *trial_tab) {
    IcLevel a{};
    a.out_ptr = REV ? h->d_in_ptr : h->d_out_ptr.p; a.out_adj = REV ? h->d_in_adj : h->d_out_adj.p;
    a.in_ptr = REV ? h->d_out_ptr.p : h->d_in_ptr; a.in_adj = REV ? h->d_out_adj.p : h->d_in_adj;
    if (prob.arc) { a.out_thr = REV ? h->d_in_thr.p : h->d_out_thr.p; a.in_thr = REV ? h->d_out_thr.p : h->d_in_thr.p; }
    if (prob.lt) { a.out_iv = REV ? h->d_in_iv.p : h->d_out_iv.p; a.in_iv = REV ? h->d_out_iv.p : h->d_in_iv.p; }
    a.vis = h->d_vis.p; a.mark = h->d_mark.p; a.touched = h->d_touched.p; a.touch_list = h->d_touch.p; a.touch_cnt = h->d_cnt.p + 3;
    a.n = h->n; a.W = W; a.T = T; a.seed = seed; a.thr = prob.thr; a.directed = h->directed; a.trial_tab = trial_tab;
    a.dense = sets * h->n * W;
    a.pull_min = std::max<int64_t>(1, sets * h->n / IC_PULL_DIV);
    const int grid = ic_blocks(a.dense);   // a wave per 64 items; no level has more than `dense` items
    // a level can only find new vertices while fewer than n rounds have passed
    const int64_t last = max_hops < 0 ? h->n : std::min<int64_t>(max_hops, h->n);
    for (int64_t r = 1; r <= last; ++r) {
        a.round = (int32_t)r;
        a.cur = (r & 1) ? h->d_fa.p : h->d_fb.p;
        a.nxt = (r & 1) ? h->d_fb.p : h->d_fa.p;
        a.cur_list = (r & 1) ? h->d_list0.p : h->d_list1.p;
        a.nxt_list = (r & 1) ? h->d_list1.p : h->d_list0.p;
        a.cur_cnt = h->d_cnt.p + (r - 1) % 3;
        a.nxt_cnt = h->d_cnt.p + r % 3;
        a.zero_cnt = h->d_cnt.p + (r + 1) % 3;
        if (prob.lt) lt_launch_level<REV>(h, a, grid);
        else if (prob.arc) ic_launch_level<REV, true>(h, a, grid);
        else ic_launch_level<REV, false>(h, a, grid);
        GH_HIP(hipGetLastError());
        if (r % IC_CHECK_EVERY == 0 && r < last) {
            int32_t alive = 0;
            GH_HIP(hipMemcpyAsync(&alive, h->d_cnt.p + r % 3, sizeof(alive), hipMemcpyDeviceToHost, h->stream));
            GH_HIP(hipStreamSynchronize(h->stream));
            if (alive == 0) break;
        }
    }
    return GH_OK;
}

// One chunk: `sets` seed sets given as unique entry ids (s * n + v) in `seeds`; counts -> out (sets, T).
gh_status ic_run_chunk(gh_ic *h, int64_t sets, const std::vector<int32_t> &seeds, int32_t W, int32_t T, uint64_t seed,
                       IcProb prob, int32_t max_hops, int32_t *out) {
    GH_HIP(hipMemsetAsync(h->d_counts.p, 0, sizeof(int32_t) * sets * T, h->stream));
    const int32_t c0[4] = {(int32_t)seeds.size(), 0, 0, (int32_t)seeds.size()};   // ring of three + touched count
    if (!seeds.empty()) {
        GH_HIP(hipMemcpyAsync(h->d_cnt.p, c0, sizeof(c0), hipMemcpyHostToDevice, h->stream));
        GH_HIP(hipMemcpyAsync(h->d_list0.p, seeds.data(), 4 * seeds.size(), hipMemcpyHostToDevice, h->stream));
        GH_HIP(hipMemcpyAsync(h->d_touch.p, seeds.data(), 4 * seeds.size(), hipMemcpyHostToDevice, h->stream));
        const int64_t si = (int64_t)seeds.size() * W;
        ic_seed_kernel<<<dim3((unsigned)((si + IC_BLOCK - 1) / IC_BLOCK)), dim3(IC_BLOCK), 0, h->stream>>>(
            h->d_list0.p, (int64_t)seeds.size(), W, T, h->d_vis.p, h->d_fa.p, h->d_touched.p);
        GH_HIP(hipGetLastError());
        GH_TRY_ST(ic_run_levels<false>(h, sets, W, T, seed, prob, max_hops, nullptr));
        const int grid_t = ic_blocks(sets * h->n * W);
        ic_count_kernel<<<dim3(grid_t), dim3(IC_BLOCK), 0, h->stream>>>(h->d_touch.p, h->d_cnt.p + 3, h->d_vis.p, h->n, W, T, h->d_counts.p);
        ic_reset_kernel<<<dim3(grid_t), dim3(IC_BLOCK), 0, h->stream>>>(h->d_touch.p, h->d_cnt.p + 3, W, h->d_vis.p, h->d_fa.p, h->d_fb.p,
                                                                       h->d_mark.p, h->d_touched.p);
        GH_HIP(hipGetLastError());
    }
    GH_HIP(hipMemcpyAsync(out, h->d_counts.p, sizeof(int32_t) * sets * T, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_ic_create(gh_ic_handle *out, int device_id, int64_t n, int64_t n_arcs, const int32_t *arcs, int32_t directed) {
    auto fail = [&](gh_status st, const std::string &msg) { g_ic_error = msg; return st; };
    if (!out) return fail(GH_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "n must be in [1, 2^31)");
    if (n_arcs < 0 || (n_arcs > 0 && !arcs)) return fail(GH_ERR_INVALID, "bad arc list");
    std::vector<uint64_t> key;
    GH_TRY_ST(gh_canonical_edge_keys(n, n_arcs, arcs, directed != 0, "arc", &key, &g_ic_error));
    gh_ic *h = new gh_ic();
    h->budget = IC_DEFAULT_BUDGET;
    h->n = n;
    h->arcs = (int64_t)key.size();
    h->directed = directed ? 1 : 0;
    auto bail = [&](gh_status st, const std::string &msg) { gh_ic_destroy(h); return fail(st, msg); };
    const gh_status st = gh_host_open(h, device_id, &g_ic_error);
    if (st != GH_OK) { gh_ic_destroy(h); return st; }
    // CSR of arcs by source (push) and by target (pull); undirected: both directions, and the two are the same CSR
    for (int pass = 0; pass < (directed ? 2 : 1); ++pass) {
        std::vector<int64_t> ptr;
        std::vector<int32_t> adj;
        gh_csr_from_keys(n, key, !directed ? GH_CSR_SYMMETRIC : pass ? GH_CSR_BY_TARGET : GH_CSR_BY_SOURCE, &ptr, &adj);
        gh_dev<int64_t> &dp = pass ? h->d_in_own_ptr : h->d_out_ptr;
        gh_dev<int32_t> &da = pass ? h->d_in_own_adj : h->d_out_adj;
        if (!dp.alloc(8 * ptr.size()) || !da.alloc(4 * adj.size())) return bail(GH_ERR_NOMEM, "hipMalloc failed");
        if (hipMemcpy(dp.p, ptr.data(), 8 * ptr.size(), hipMemcpyHostToDevice) != hipSuccess ||
            (!adj.empty() && hipMemcpy(da.p, adj.data(), 4 * adj.size(), hipMemcpyHostToDevice) != hipSuccess))
            return bail(GH_ERR_HIP, "upload failed");
    }
    h->d_in_ptr = directed ? h->d_in_own_ptr.p : h->d_out_ptr.p;
    h->d_in_adj = directed ? h->d_in_own_adj.p : h->d_out_adj.p;
    h->keys = std::move(key);
    *out = h;
    return GH_OK;
}

// The threshold arrays are built on the host from the canonical keys, as the CSRs were: the listed pairs become a sorted
// table (u << 32 | v) -> thr, and every slot of a CSR row looks its own arc up in it (an arc that is not listed: 0).
extern "C" gh_status gh_ic_set_arc_probabilities(gh_ic_handle h, int64_t m, const int32_t *arcs, const double *prob) {
    if (!h) { g_ic_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (m < 0 || (m > 0 && (!arcs || !prob))) return fail(GH_ERR_INVALID, "bad arc probability arguments");
    std::vector<std::pair<uint64_t, uint32_t>> tab((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t u = arcs[2 * i], v = arcs[2 * i + 1];
        const std::string pair = "pair " + std::to_string(i) + " (" + std::to_string(u) + ", " + std::to_string(v) + ")";
        bool is_arc = u >= 0 && u < h->n && v >= 0 && v < h->n && u != v;
        if (is_arc) {
            const uint64_t a = h->directed ? u : std::min(u, v), b = h->directed ? v : std::max(u, v);
            is_arc = std::binary_search(h->keys.begin(), h->keys.end(), (a << 32) | b);
        }
        if (!is_arc) return fail(GH_ERR_INVALID, pair + " is not an arc of the graph");
        if (!(prob[i] >= 0.0 && prob[i] <= 1.0)) return fail(GH_ERR_INVALID, "the probability of " + pair + " is not in [0, 1]");
        tab[(size_t)i] = {((uint64_t)u << 32) | (uint64_t)v, ic_threshold(prob[i])};
    }
    std::sort(tab.begin(), tab.end());
    for (int64_t i = 1; i < m; ++i)
        if (tab[(size_t)i].first == tab[(size_t)i - 1].first)
            return fail(GH_ERR_INVALID, "the pair (" + std::to_string(tab[(size_t)i].first >> 32) + ", " +
                                            std::to_string(tab[(size_t)i].first & 0xFFFFFFFFu) + ") is listed twice");
    auto thr_of = [&](int64_t u, int64_t v) -> uint32_t {
        const uint64_t k = ((uint64_t)u << 32) | (uint64_t)v;
        auto it = std::lower_bound(tab.begin(), tab.end(), std::make_pair(k, (uint32_t)0));
        return it != tab.end() && it->first == k ? it->second : 0;
    };
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    // row x, neighbour y: out_thr holds x -> y in the slots of the out-CSR, in_thr holds y -> x in the slots of the in-CSR
    // (for an undirected graph both are over the one symmetric CSR)
    gh_dev<uint32_t> fresh[2];
    std::vector<int64_t> ptr;
    std::vector<int32_t> adj;
    std::vector<uint32_t> thr;
    for (int pass = 0; pass < 2; ++pass) {
        if (h->directed || pass == 0)
            gh_csr_from_keys(h->n, h->keys, !h->directed ? GH_CSR_SYMMETRIC : pass ? GH_CSR_BY_TARGET : GH_CSR_BY_SOURCE, &ptr, &adj);
        thr.resize(adj.size());
        for (int64_t x = 0; x < h->n; ++x)
            for (int64_t k = ptr[(size_t)x]; k < ptr[(size_t)x + 1]; ++k)
                thr[(size_t)k] = pass ? thr_of(adj[(size_t)k], x) : thr_of(x, adj[(size_t)k]);
        if (!fresh[pass].alloc(4 * thr.size())) return fail(GH_ERR_NOMEM, "hipMalloc failed for the arc thresholds");
        if (!thr.empty() && hipMemcpy(fresh[pass].p, thr.data(), 4 * thr.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GH_ERR_HIP, "upload of the arc thresholds failed");
    }
    // nothing failed: the new table replaces the old one (no call of this handle is in flight, every entry point blocks)
    h->d_out_thr = std::move(fresh[0]);
    h->d_in_thr = std::move(fresh[1]);
    h->has_table = true;
    return GH_OK;
}

// The intervals are built on the host in the target's row of the by-target CSR, whose slots ascend in source id: S is the
// sequential double sum of the row's weights and a slot's (lo, hi) = (c_{k-1}, c_k), c_k = min(2^32 - 1, floor(S_k 2^32 + .5)).
// The by-source CSR gets, for its slot (x, y), the interval of arc x -> y out of y's row.
extern "C" gh_status gh_ic_set_lt_weights(gh_ic_handle h, int64_t m, const int32_t *arcs, const double *weight) {
    if (!h) { g_ic_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (m < 0 || (m > 0 && (!arcs || !weight))) return fail(GH_ERR_INVALID, "bad arc weight arguments");
    std::vector<std::pair<uint64_t, double>> tab((size_t)m);   // keyed (target, source): a row's weights lie together
    for (int64_t i = 0; i < m; ++i) {
        const int64_t u = arcs[2 * i], v = arcs[2 * i + 1];
        const std::string pair = "pair " + std::to_string(i) + " (" + std::to_string(u) + ", " + std::to_string(v) + ")";
        bool is_arc = u >= 0 && u < h->n && v >= 0 && v < h->n && u != v;
        if (is_arc) {
            const uint64_t a = h->directed ? u : std::min(u, v), b = h->directed ? v : std::max(u, v);
            is_arc = std::binary_search(h->keys.begin(), h->keys.end(), (a << 32) | b);
        }
        if (!is_arc) return fail(GH_ERR_INVALID, pair + " into vertex " + std::to_string(v) + " is not an arc of the graph");
        if (!(weight[i] >= 0.0 && weight[i] <= 1.0))
            return fail(GH_ERR_INVALID, "the weight of " + pair + " into vertex " + std::to_string(v) + " is not in [0, 1]");
        tab[(size_t)i] = {((uint64_t)v << 32) | (uint64_t)u, weight[i]};
    }
    std::sort(tab.begin(), tab.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    for (int64_t i = 1; i < m; ++i)
        if (tab[(size_t)i].first == tab[(size_t)i - 1].first)
            return fail(GH_ERR_INVALID, "the pair (" + std::to_string(tab[(size_t)i].first & 0xFFFFFFFFu) + ", " +
                                            std::to_string(tab[(size_t)i].first >> 32) + ") into vertex " +
                                            std::to_string(tab[(size_t)i].first >> 32) + " is listed twice");
    // the target's rows: in_ptr / in_adj, slot k of row v = arc in_adj[k] -> v
    std::vector<int64_t> in_ptr, out_ptr;
    std::vector<int32_t> in_adj, out_adj;
    gh_csr_from_keys(h->n, h->keys, h->directed ? GH_CSR_BY_TARGET : GH_CSR_SYMMETRIC, &in_ptr, &in_adj);
    std::vector<uint2> in_iv(in_adj.size()), out_iv;
    size_t t = 0;
    for (int64_t v = 0; v < h->n; ++v) {
        double S = 0.0;
        uint32_t c = 0;
        for (int64_t k = in_ptr[(size_t)v]; k < in_ptr[(size_t)v + 1]; ++k) {
            const uint64_t key = ((uint64_t)v << 32) | (uint64_t)(uint32_t)in_adj[(size_t)k];
            while (t < tab.size() && tab[t].first < key) ++t;   // both ascend by (target, source)
            if (t < tab.size() && tab[t].first == key) S += tab[t].second;
            const uint32_t c1 = (uint32_t)std::min(4294967295.0, std::floor(S * 4294967296.0 + 0.5));
            in_iv[(size_t)k] = make_uint2(c, c1);
            c = c1;
        }
        if (S > 1.0 + 1.0 / 1048576.0)
            return fail(GH_ERR_INVALID, "the weights into vertex " + std::to_string(v) + " sum to " + std::to_string(S) +
                                            ", above 1 + 2^-20");
    }
    const std::vector<int64_t> *optr = &in_ptr;
    const std::vector<int32_t> *oadj = &in_adj;
    if (h->directed) {
        gh_csr_from_keys(h->n, h->keys, GH_CSR_BY_SOURCE, &out_ptr, &out_adj);
        optr = &out_ptr;
        oadj = &out_adj;
    }
    out_iv.resize(oadj->size());
    for (int64_t x = 0; x < h->n; ++x)
        for (int64_t k = (*optr)[(size_t)x]; k < (*optr)[(size_t)x + 1]; ++k) {   // arc x -> y: x's place in y's row, which ascends
            const int64_t y = (*oadj)[(size_t)k];
            const auto rb = in_adj.begin() + in_ptr[(size_t)y], re = in_adj.begin() + in_ptr[(size_t)y + 1];
            out_iv[(size_t)k] = in_iv[(size_t)(std::lower_bound(rb, re, (int32_t)x) - in_adj.begin())];
        }
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    gh_dev<uint2> fresh[2];
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<uint2> &iv = pass ? in_iv : out_iv;
        if (!fresh[pass].alloc(sizeof(uint2) * iv.size())) return fail(GH_ERR_NOMEM, "hipMalloc failed for the arc intervals");
        if (!iv.empty() && hipMemcpy(fresh[pass].p, iv.data(), sizeof(uint2) * iv.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(GH_ERR_HIP, "upload of the arc intervals failed");
    }
    // nothing failed: the new table replaces the old one (no call of this handle is in flight, every entry point blocks)
    h->d_out_iv = std::move(fresh[0]);
    h->d_in_iv = std::move(fresh[1]);
    h->has_lt = true;
    return GH_OK;
}

extern "C" void gh_ic_destroy(gh_ic_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_ic_last_error(gh_ic_handle h) { return h ? h->err.c_str() : g_ic_error.c_str(); }

extern "C" gh_status gh_ic_set_memory_budget(gh_ic_handle h, int64_t bytes) {
    return gh_host_set_budget(h, bytes, IC_DEFAULT_BUDGET, &g_ic_error);
}

extern "C" int64_t gh_ic_arc_count(gh_ic_handle h) { return h ? h->arcs : -1; }

// gh_ic_spread (p: the scalar), gh_ic_spread_arcs and gh_ic_spread_lt (p = NULL: the handle's table of that kind)
static gh_status ic_spread(gh_ic_handle h, const double *p, IcTable table, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                           const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base, int64_t n_base,
                           int64_t *totals, int32_t *per_trial) {
    if (!h) { g_ic_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    IcProb prob;
    GH_TRY_ST(ic_prob(h, p, table, &prob));
    if (n_trials < 1) return fail(GH_ERR_INVALID, "n_trials must be >= 1");
    if (max_hops < -1) return fail(GH_ERR_INVALID, "max_hops must be >= 0, or -1 for no limit");
    if (n_sets < 0 || (n_sets > 0 && (!set_offsets || !totals))) return fail(GH_ERR_INVALID, "bad seed-set arguments");
    if (n_base < 0 || (n_base > 0 && !base)) return fail(GH_ERR_INVALID, "bad base set");
    if (n_sets > 0 && set_offsets[0] != 0) return fail(GH_ERR_INVALID, "set_offsets[0] must be 0");
    for (int64_t s = 0; s < n_sets; ++s)
        if (set_offsets[s + 1] < set_offsets[s]) return fail(GH_ERR_INVALID, "set_offsets must not decrease");
    const int64_t n_vert = n_sets > 0 ? set_offsets[n_sets] : 0;
    if (n_vert > 0 && !set_vertices) return fail(GH_ERR_INVALID, "set_vertices is NULL");
    for (int64_t i = 0; i < n_vert; ++i)
        if (set_vertices[i] < 0 || set_vertices[i] >= h->n) return fail(GH_ERR_INVALID, "seed vertex id outside [0, n)");
    for (int64_t i = 0; i < n_base; ++i)
        if (base[i] < 0 || base[i] >= h->n) return fail(GH_ERR_INVALID, "base vertex id outside [0, n)");
    if (n_sets == 0) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int32_t T = n_trials, W = (n_trials + 63) / 64;
    const int64_t per_set = ic_bytes_per_set(h->n, W);
    int64_t chunk = std::max<int64_t>(1, h->budget / per_set);
    chunk = std::min<int64_t>({chunk, n_sets, (int64_t)INT32_MAX / h->n});
    gh_status st = ic_reserve(h, chunk, W, T);
    if (st != GH_OK) return st;
    std::vector<int32_t> base_u(base, base + n_base);
    std::sort(base_u.begin(), base_u.end());
    base_u.erase(std::unique(base_u.begin(), base_u.end()), base_u.end());
    std::vector<int32_t> base_counts;
    if (!base_u.empty()) {   // |R(base)| per trial, with the same coins
        base_counts.resize(T);
        st = ic_run_chunk(h, 1, base_u, W, T, seed, prob, max_hops, base_counts.data());
        if (st != GH_OK) return st;
    }
    std::vector<int32_t> counts((size_t)chunk * T), one;
    std::vector<int32_t> seeds;
    for (int64_t s0 = 0; s0 < n_sets; s0 += chunk) {
        const int64_t ns = std::min(chunk, n_sets - s0);
        seeds.clear();
        for (int64_t s = 0; s < ns; ++s) {   // unique vertices of base + set s, as entries of the chunk's state
            one.assign(base_u.begin(), base_u.end());
            one.insert(one.end(), set_vertices + set_offsets[s0 + s], set_vertices + set_offsets[s0 + s + 1]);
            std::sort(one.begin(), one.end());
            one.erase(std::unique(one.begin(), one.end()), one.end());
            for (int32_t v : one) seeds.push_back((int32_t)(s * h->n + v));
        }
        st = ic_run_chunk(h, ns, seeds, W, T, seed, prob, max_hops, counts.data());
        if (st != GH_OK) return st;
        for (int64_t s = 0; s < ns; ++s) {
            int64_t tot = 0;
            int32_t *row = counts.data() + s * T;
            for (int32_t t = 0; t < T; ++t) {
                if (!base_counts.empty()) row[t] -= base_counts[t];
                tot += row[t];
            }
            totals[s0 + s] = tot;
            if (per_trial) std::copy(row, row + T, per_trial + (s0 + s) * (int64_t)T);
        }
    }
    return GH_OK;
}

extern "C" gh_status gh_ic_spread(gh_ic_handle h, double p, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                                  const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base, int64_t n_base,
                                  int64_t *totals, int32_t *per_trial) {
    return ic_spread(h, &p, IC_TABLE_ARCS, max_hops, n_trials, seed, n_sets, set_offsets, set_vertices, base, n_base, totals, per_trial);
}

extern "C" gh_status gh_ic_spread_arcs(gh_ic_handle h, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                                       const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base,
                                       int64_t n_base, int64_t *totals, int32_t *per_trial) {
    return ic_spread(h, nullptr, IC_TABLE_ARCS, max_hops, n_trials, seed, n_sets, set_offsets, set_vertices, base, n_base, totals,
                     per_trial);
}

extern "C" gh_status gh_ic_spread_lt(gh_ic_handle h, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                                     const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base,
                                     int64_t n_base, int64_t *totals, int32_t *per_trial) {
    return ic_spread(h, nullptr, IC_TABLE_LT, max_hops, n_trials, seed, n_sets, set_offsets, set_vertices, base, n_base, totals,
                     per_trial);
}

// ---- reverse-reachable sets (header: "reverse influence sampling") ------------------------------------------------------
// A chunk is ONE set of the level machinery with W words: bit b of word w is sample 64w + b of the chunk.  Round 0 sets one
// bit per root; the levels run with the CSRs swapped (ic_run_levels<true>); then the touched list is turned into the CSR of
// the chunk's sets: count per bit (ic_count_kernel), scan, scatter, segmented sort into the collection.
namespace {

// Words per chunk beyond the budget.  A touched entry costs W words in every pass over the lists while a sub-critical
// search sets one or two bits of them, so more words only pay while they save launches: measured on random-regular graphs
// of degree 8 at p = 0.1, 2^18 samples take 333 / 84 / 55 ms at W = 8 / 32 / 64 (n = 100 K) and 324 / 74 / 50 / 38 ms at
// W = 8 / 32 / 64 / 128 (n = 1 M).  And round 0's frontier, up to 64 W roots, has to stay under the pull threshold n / 16
// (half of it here), or every level scans the dense state: 210 ms at W = 128, n = 100 K.  Small graphs keep 16 words.
#define RR_MAX_WORDS 128
#define RR_MIN_WORDS_CAP 16

// Round 0.  Several samples may share a root: its words take one atomicOr per sample, and the first to stamp the entry
// (mark = -1, no round has that stamp) puts it into list 0 and the touched list, so both stay unique.
__global__ __launch_bounds__(IC_BLOCK) void rr_root_kernel(const int32_t *__restrict__ roots, int32_t S, int32_t W, uint64_t *vis,
                                                          uint64_t *cur, int32_t *mark, uint8_t *touched, int32_t *list0,
                                                          int32_t *touch_list, int32_t *cnt) {
    const int32_t j = blockIdx.x * IC_BLOCK + threadIdx.x;
    if (j >= S) return;
    const int32_t r = roots[j];
    const int64_t x = (int64_t)r * W + (j >> 6);
    const unsigned long long bit = 1ull << (j & 63);
    atomicOr((unsigned long long *)&vis[x], bit);
    atomicOr((unsigned long long *)&cur[x], bit);
    if (atomicExch(&mark[r], -1) != -1) {
        touched[r] = 1;
        list0[atomicAdd(cnt, 1)] = r;
        touch_list[atomicAdd(cnt + 3, 1)] = r;
    }
}

// members of sample (w, b) -> scatter[off[64w + b] ..), in the order the atomics fall; the segmented sort orders them
__global__ __launch_bounds__(IC_BLOCK) void rr_scatter_kernel(const int32_t *__restrict__ touch_list, const int32_t *touch_cnt,
                                                             const uint64_t *__restrict__ vis, int32_t W,
                                                             const int64_t *__restrict__ off, int32_t *cursor, int32_t *scatter) {
    const int64_t items = (int64_t)*touch_cnt * W;
    for (int64_t i = (int64_t)blockIdx.x * IC_BLOCK + threadIdx.x; i < items; i += (int64_t)gridDim.x * IC_BLOCK) {
        const int32_t e = touch_list[i / W];
        const int32_t w = (int32_t)(i % W);
        uint64_t x = vis[(int64_t)e * W + w];
        while (x) {
            const int b = __ffsll((unsigned long long)x) - 1;
            x &= x - 1;
            scatter[off[64 * w + b] + atomicAdd(&cursor[64 * w + b], 1)] = e;
        }
    }
}

__global__ __launch_bounds__(IC_BLOCK) void rr_indptr_kernel(const int64_t *__restrict__ off, int32_t S, int64_t base, int64_t *indptr) {
    const int32_t j = blockIdx.x * IC_BLOCK + threadIdx.x;
    if (j < S) indptr[j + 1] = base + off[j + 1];
}

struct RrWiden {
    __host__ __device__ int64_t operator()(int32_t x) const { return x; }
};

gh_status rr_scratch(gh_ic *h, int64_t bits) {
    if (bits <= h->cap_rr_bits) return GH_OK;
    h->cap_rr_bits = 0;
    if (!h->d_rr_trials.alloc(8 * bits) || !h->d_rr_count.alloc(4 * (bits + 1)) || !h->d_rr_cursor.alloc(4 * bits) ||
        !h->d_rr_off.alloc(8 * (bits + 1))) {
        h->err = "hipMalloc failed for the sample tables of a chunk";
        return GH_ERR_NOMEM;
    }
    h->cap_rr_bits = bits;
    return GH_OK;
}

gh_status rr_tmp(gh_ic *h, size_t bytes) {
    if (bytes <= h->d_rr_tmp.bytes) return GH_OK;
    if (!h->d_rr_tmp.alloc(bytes)) { h->err = "hipMalloc failed for scan / sort scratch"; return GH_ERR_NOMEM; }
    return GH_OK;
}

// One chunk of S samples (trials / roots on the host), appended to the collection at (rr->sets, rr->members).
gh_status rr_run_chunk(gh_ic *h, gh_rr *rr, int32_t S, int32_t W, const uint64_t *trials, const int32_t *roots, uint64_t seed,
                       IcProb prob, int32_t max_hops, int64_t asked) {
    const int64_t bits = 64 * (int64_t)W;
    auto refuse = [&](int64_t total) {
        const double mean = (double)(rr->members + total) / (double)(rr->sets + S);
        h->err = "the collection would outgrow its memory budget of " + std::to_string(rr->budget) + " bytes: " +
                 std::to_string(asked) + " samples asked, mean set size " + std::to_string(mean) + " over the first " +
                 std::to_string(rr->sets + S) + " (reverse influence sampling is for sets that are small against n)";
        return GH_ERR_NOMEM;
    };
    {
        const gh_status st0 = rr_reserve(rr, rr->sets + S, rr->members, h->stream);
        if (st0 == GH_ERR_NOMEM) return refuse(0);
        if (st0 != GH_OK) return st0;
    }
    GH_HIP(hipMemsetAsync(h->d_rr_trials.p, 0, 8 * bits, h->stream));
    GH_HIP(hipMemcpyAsync(h->d_rr_trials.p, trials, 8 * (size_t)S, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(rr->d_roots.p + rr->sets, roots, 4 * (size_t)S, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemsetAsync(h->d_cnt.p, 0, 4 * 4, h->stream));
    GH_HIP(hipMemsetAsync(h->d_rr_count.p, 0, 4 * (bits + 1), h->stream));
    GH_HIP(hipMemsetAsync(h->d_rr_cursor.p, 0, 4 * bits, h->stream));
    rr_root_kernel<<<dim3((unsigned)((S + IC_BLOCK - 1) / IC_BLOCK)), dim3(IC_BLOCK), 0, h->stream>>>(
        rr->d_roots.p + rr->sets, S, W, h->d_vis.p, h->d_fa.p, h->d_mark.p, h->d_touched.p, h->d_list0.p, h->d_touch.p, h->d_cnt.p);
    GH_HIP(hipGetLastError());
    GH_TRY_ST(ic_run_levels<true>(h, 1, W, S, seed, prob, max_hops, h->d_rr_trials.p));
    const int grid_t = ic_blocks(h->n * W);
    ic_count_kernel<<<dim3(grid_t), dim3(IC_BLOCK), 0, h->stream>>>(h->d_touch.p, h->d_cnt.p + 3, h->d_vis.p, h->n, W, S, h->d_rr_count.p);
    GH_HIP(hipGetLastError());
    hipcub::TransformInputIterator<int64_t, RrWiden, const int32_t *> wide(h->d_rr_count.p, RrWiden());
    size_t temp = 0;
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, wide, h->d_rr_off.p, (int)(bits + 1), h->stream));
    GH_TRY_ST(rr_tmp(h, temp));
    GH_HIP(hipcub::DeviceScan::ExclusiveSum(h->d_rr_tmp.p, temp, wide, h->d_rr_off.p, (int)(bits + 1), h->stream));
    int64_t total = 0;
    GH_HIP(hipMemcpyAsync(&total, h->d_rr_off.p + bits, 8, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    // from here on a failure must still leave the chunk state zero
    auto reset = [&]() {
        ic_reset_kernel<<<dim3(grid_t), dim3(IC_BLOCK), 0, h->stream>>>(h->d_touch.p, h->d_cnt.p + 3, W, h->d_vis.p, h->d_fa.p, h->d_fb.p,
                                                                       h->d_mark.p, h->d_touched.p);
        return hipStreamSynchronize(h->stream);
    };
    gh_status st = total > INT32_MAX ? GH_ERR_NOMEM : rr_reserve(rr, rr->sets + S, rr->members + total, h->stream);
    if (st == GH_OK && total > h->cap_rr_scatter) {
        h->cap_rr_scatter = 0;
        if (h->d_rr_scatter.alloc(4 * (size_t)total)) h->cap_rr_scatter = total;
        else st = GH_ERR_NOMEM;
    }
    if (st == GH_ERR_NOMEM) (void)refuse(total);
    if (st != GH_OK) { (void)reset(); return st; }
    if (total > 0) {
        rr_scatter_kernel<<<dim3(grid_t), dim3(IC_BLOCK), 0, h->stream>>>(h->d_touch.p, h->d_cnt.p + 3, h->d_vis.p, W, h->d_rr_off.p,
                                                                         h->d_rr_cursor.p, h->d_rr_scatter.p);
        GH_HIP(hipGetLastError());
        int bits_n = 1;
        while (((int64_t)1 << bits_n) < h->n) ++bits_n;
        hipError_t e = hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, temp, h->d_rr_scatter.p, rr->d_members.p + rr->members, (int)total,
                                                                  S, h->d_rr_off.p, h->d_rr_off.p + 1, 0, bits_n, h->stream);
        if (e == hipSuccess && rr_tmp(h, temp) != GH_OK) { (void)reset(); return GH_ERR_NOMEM; }
        if (e == hipSuccess)
            e = hipcub::DeviceSegmentedRadixSort::SortKeys(h->d_rr_tmp.p, temp, h->d_rr_scatter.p, rr->d_members.p + rr->members, (int)total,
                                                           S, h->d_rr_off.p, h->d_rr_off.p + 1, 0, bits_n, h->stream);
        if (e != hipSuccess) {
            h->err = std::string("segmented sort: ") + hipGetErrorString(e);
            (void)reset();
            return GH_ERR_HIP;
        }
    }
    rr_indptr_kernel<<<dim3((unsigned)((S + IC_BLOCK - 1) / IC_BLOCK)), dim3(IC_BLOCK), 0, h->stream>>>(h->d_rr_off.p, S, rr->members,
                                                                                                       rr->d_indptr.p + rr->sets);
    GH_HIP(hipGetLastError());
    GH_HIP(reset());
    rr->sets += S;
    rr->members += total;
    return GH_OK;
}

}  // namespace

// gh_ic_rr_sample (p: the scalar), gh_ic_rr_sample_arcs and gh_ic_rr_sample_lt (p = NULL: the handle's table of that kind)
static gh_status ic_rr_sample(gh_ic_handle h, gh_rr_handle rr, const double *p, IcTable table, int32_t max_hops, uint64_t seed, int64_t n_samples,
                              const uint64_t *trials, const int32_t *roots) {
    if (!h) { g_ic_error = "handle is NULL"; return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (!rr) return fail(GH_ERR_INVALID, "the collection handle is NULL");
    if (rr->n != h->n || rr->device != h->device) return fail(GH_ERR_INVALID, "the collection was created for another n or device");
    IcProb prob;
    GH_TRY_ST(ic_prob(h, p, table, &prob));
    if (max_hops < -1) return fail(GH_ERR_INVALID, "max_hops must be >= 0, or -1 for no limit");
    if (n_samples < 0) return fail(GH_ERR_INVALID, "n_samples must be >= 0");
    if (rr->sets + n_samples > INT32_MAX) return fail(GH_ERR_INVALID, "a collection holds fewer than 2^31 sets");
    if (roots)
        for (int64_t j = 0; j < n_samples; ++j)
            if (roots[j] < 0 || roots[j] >= h->n) return fail(GH_ERR_INVALID, "root vertex id outside [0, n)");
    if (n_samples == 0) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    h->err.clear();
    rr->err.clear();
    // words per chunk: what the budget holds of one set's state, as gh_ic_spread sizes its seed sets
    int64_t W = std::max<int64_t>(1, (h->budget / h->n - 17) / 24);
    W = std::min<int64_t>({W, RR_MAX_WORDS, std::max<int64_t>(RR_MIN_WORDS_CAP, h->n / (2 * 64 * IC_PULL_DIV)), (n_samples + 63) / 64});
    GH_TRY_ST(ic_reserve(h, 1, (int32_t)W, 1));
    GH_TRY_ST(rr_scratch(h, 64 * W));
    const int64_t sets0 = rr->sets, members0 = rr->members;
    std::vector<uint64_t> tr((size_t)(64 * W));
    std::vector<int32_t> ro((size_t)(64 * W));
    for (int64_t j0 = 0; j0 < n_samples; j0 += 64 * W) {
        const int32_t S = (int32_t)std::min<int64_t>(64 * W, n_samples - j0);
        for (int32_t j = 0; j < S; ++j) {
            tr[j] = trials ? trials[j0 + j] : (uint64_t)(sets0 + j0 + j);
            ro[j] = roots ? roots[j0 + j]
                          : (int32_t)(((ic_mix(ic_mix(seed + tr[j] * IC_GOLDEN) ^ ~0ull) >> 32) * (uint64_t)h->n) >> 32);
        }
        const gh_status st = rr_run_chunk(h, rr, S, (S + 63) / 64, tr.data(), ro.data(), seed, prob, max_hops, n_samples);
        if (st != GH_OK) {   // all or nothing: the collection is what it was before the call
            if (h->err.empty()) h->err = rr->err;   // the message of a failed copy while the collection grew
            rr->err = h->err;
            rr->sets = sets0;
            rr->members = members0;
            return st;
        }
    }
    return GH_OK;
}

extern "C" gh_status gh_ic_rr_sample(gh_ic_handle h, gh_rr_handle rr, double p, int32_t max_hops, uint64_t seed, int64_t n_samples,
                                     const uint64_t *trials, const int32_t *roots) {
    return ic_rr_sample(h, rr, &p, IC_TABLE_ARCS, max_hops, seed, n_samples, trials, roots);
}

extern "C" gh_status gh_ic_rr_sample_arcs(gh_ic_handle h, gh_rr_handle rr, int32_t max_hops, uint64_t seed, int64_t n_samples,
                                          const uint64_t *trials, const int32_t *roots) {
    return ic_rr_sample(h, rr, nullptr, IC_TABLE_ARCS, max_hops, seed, n_samples, trials, roots);
}

extern "C" gh_status gh_ic_rr_sample_lt(gh_ic_handle h, gh_rr_handle rr, int32_t max_hops, uint64_t seed, int64_t n_samples,
                                        const uint64_t *trials, const int32_t *roots) {
    return ic_rr_sample(h, rr, nullptr, IC_TABLE_LT, max_hops, seed, n_samples, trials, roots);
}
