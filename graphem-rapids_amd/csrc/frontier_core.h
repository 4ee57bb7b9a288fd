// The bit-parallel multi-source breadth-first search that gh_cent_distances (graphstats.hip) and gh_qual_hop_profile
// (quality.hip) share.  64 sources to a group; bit b of a word belongs to source 64 g + b.  Per (group, vertex) three
// words, [group][vertex]: vis (sources that reached v; the unused bits of a short last group preset), cur and nxt (sources
// whose frontier holds v at the previous / this level).  What a level does with its new bits, the budget, the group count,
// the level kernel's grid and the check interval stay with each caller.
#pragma once
#include "csr_core.h"
#include "host_util.h"

namespace {
// vis = the unused bits of the batch's last group, 0 elsewhere; cur = 0
__global__ __launch_bounds__(GS_BLOCK) void gs_frontier_fill_kernel(int64_t n, int64_t G, uint64_t unused_last, uint64_t *vis, uint64_t *cur) {
    GS_GRID_LOOP(i, G * n) {
        vis[i] = i >= (G - 1) * n ? unused_last : 0;
        cur[i] = 0;
    }
}

// source j of the batch: bit j & 63 of group j >> 6, at its own vertex; a repeated id is a source of its own
__global__ __launch_bounds__(GS_BLOCK) void gs_frontier_seed_kernel(int64_t n, int64_t n_src, const int32_t *__restrict__ src,
                                                                    unsigned long long *vis, unsigned long long *cur) {
    GS_GRID_LOOP(j, n_src) {
        const int64_t w = (j >> 6) * n + src[j];
        atomicOr(&vis[w], 1ull << (j & 63));
        atomicOr(&cur[w], 1ull << (j & 63));
    }
}
}  // namespace

// One vertex of one group at one level: the word of new bits, (OR of cur over the neighbours) & ~vis[v].  nxt[v] is always
// stored, so the ping-pong buffers need no clearing; vis[v] only when something is new.
__device__ __forceinline__ uint64_t gs_frontier_pull(const int64_t *ptr, const int32_t *adj, uint64_t *vis, const uint64_t *cur,
                                                     uint64_t *nxt, int64_t v) {
    uint64_t w = 0;
    const uint64_t need = ~vis[v];
    if (need) {
        uint64_t acc = 0;
        const int64_t beg = ptr[v], end = ptr[v + 1];
        for (int64_t k = beg; k < end; ++k) acc |= cur[adj[k]];
        w = acc & need;
        if (w) vis[v] = ~need | w;
    }
    nxt[v] = w;
    return w;
}

// The state of up to G groups in flight on n vertices: 24 n bytes a group, and flags[L] = 1 when level L reached something
// (what gh_level_loop reads; flags[0] is preset).
struct gs_frontier {
    gh_dev<uint64_t> vis, fa, fb;
    gh_dev<int32_t> flags;
    int64_t n = 0;

    bool alloc(int64_t G, int64_t n_) {
        n = n_;
        return vis.alloc(8 * G * n) && fa.alloc(8 * G * n) && fb.alloc(8 * G * n) && flags.alloc(4 * (n + 2));
    }
    // begins a batch of G groups holding ns <= 64 G sources (d_src, on the device); a launch takes at most max_blocks workgroups
    gh_status begin(gh_host *h, int64_t G, int64_t ns, const int32_t *d_src, int64_t max_blocks) {
        GH_HIP(hipMemsetAsync(flags.p, 0, 4 * (n + 2), h->stream));
        const int32_t one = 1;
        GH_HIP(hipMemcpyAsync(flags.p, &one, 4, hipMemcpyHostToDevice, h->stream));
        const int64_t in_last = ns - 64 * (G - 1);
        const uint64_t unused_last = in_last < 64 ? ~0ull << in_last : 0;
        auto blocks = [&](int64_t items) { return dim3((unsigned)std::max<int64_t>(1, std::min(max_blocks, (items + GS_BLOCK - 1) / GS_BLOCK))); };
        gs_frontier_fill_kernel<<<blocks(G * n), dim3(GS_BLOCK), 0, h->stream>>>(n, G, unused_last, vis.p, fa.p);
        gs_frontier_seed_kernel<<<blocks(ns), dim3(GS_BLOCK), 0, h->stream>>>(n, ns, d_src, vis.as<unsigned long long>(), fa.as<unsigned long long>());
        GH_LAUNCH_CHECK();
        return GH_OK;
    }
    const uint64_t *cur(int32_t L) const { return (L & 1) ? fa.p : fb.p; }   // level L = 1, 2, .. reads cur(L) and writes nxt(L)
    uint64_t *nxt(int32_t L) const { return (L & 1) ? fb.p : fa.p; }
};
