// Graph statistics on the GPU (include/graphem_hip.h "graph statistics"; graphem-rapids_amd/graphstats.py): connected
// components, hop distances from many sources, and triangles per vertex, over the centrality handle's deduplicated
// symmetric CSR (neighbours ascending).  Everything is an integer: no result depends on the order of an atomic.
//
// Components.  label[v] starts as v and only ever drops, to the id of a vertex of v's component.
//   gs_hook_kernel   m = the smallest label among v and its neighbours; when m < label[v], atomicMin m onto
//                    label[label[v]] (the tree's root, once the trees are stars) and onto label[v].
//   gs_jump_kernel   pointer jumping: label[v] = the root of v's tree (follow label[] until it points at itself).  Roots
//                    are not written here, so every tree is a star afterwards.
//   A round that hooks nothing saw label[u] == label[v] on every arc of a forest of stars: one root per component, and
//   since label[x] <= x stays inside the component, that root is the component's smallest id.  Round r runs only when
//   round r - 1 set its flag; the host reads the flags every GS_CHECK_EVERY rounds.
//
// Distances.  The bit-parallel search of frontier_core.h: its state, its fill and seed kernels and the pull step of one
// vertex, shared with quality.hip's hop profile.  Lane = vertex, so the 64 words a wave holds are one group's.
//   gs_level_kernel (L)   gs_frontier_pull gives every lane its word of new bits.  The wave transposes its 64 new words
//                         with 64 ballots: lane b adds the population count of bit b to a register, over a grid-stride
//                         loop; then, per source, integer atomics onto counters that start at zero:
//                         reached += count, dist_sum += L count, eccentricity = max(., L).  Sets flags[L] when anything
//                         was reached; a launch after the last level sees flags[L - 1] == 0 and returns.
//
// Triangles.  One thread per arc (u, v) with u < v: the shorter of the two rows, from its first entry above v, is searched
// in the longer one by bisection (gs_common_walk of csr_core.h: the window shrinks as both ascend), so an arc costs
// min(deg) log(max deg).  Every
// triangle u < v < w is found once, at its arc (u, v), and credited to its three vertices with 64-bit integer atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "cent_handle.h"
#include "csr_core.h"
#include "frontier_core.h"

namespace {

typedef unsigned long long gs_u64;

// ---- components -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_BLOCK) void gs_label_init_kernel(int64_t n, int32_t *label) {
    GS_GRID_LOOP(v, n) label[v] = (int32_t)v;
}

__global__ __launch_bounds__(GS_BLOCK) void gs_hook_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                           int32_t *label, int32_t *flags, int32_t r) {
    if (gs_flag(&flags[r - 1]) == 0) return;
    GS_GRID_LOOP(v, n) {
        const int32_t lv = label[v];
        int32_t m = lv;
        const int64_t beg = ptr[v], end = ptr[v + 1];
        for (int64_t k = beg; k < end; ++k) m = min(m, label[adj[k]]);
        if (m < lv) {
            atomicMin(&label[lv], m);
            atomicMin(&label[v], m);
            if (gs_flag(&flags[r]) == 0) flags[r] = 1;
        }
    }
}

__global__ __launch_bounds__(GS_BLOCK) void gs_jump_kernel(int64_t n, int32_t *label, const int32_t *flags, int32_t r) {
    if (gs_flag(&flags[r]) == 0) return;
    GS_GRID_LOOP(v, n) {
        int32_t l = label[v];
        for (;;) {
            const int32_t p = label[l];
            if (p == l) break;
            l = p;
        }
        label[v] = l;
    }
}

// ---- distances ------------------------------------------------------------------------------------------------------
struct GsLevel {
    const int64_t *ptr; const int32_t *adj;
    uint64_t *vis; const uint64_t *cur; uint64_t *nxt;
    int32_t *flags;              // flags[L] = 1: level L reached something
    gs_u64 *reached, *dist_sum;  // per source of the batch
    int32_t *ecc;
    int64_t n;
    int32_t level;
};

// grid (x, G): the waves of row g stride over the vertices, 64 at a time
__global__ __launch_bounds__(GS_BLOCK) void gs_level_kernel(GsLevel a) {
    if (gs_flag(&a.flags[a.level - 1]) == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t g = blockIdx.y, off = g * a.n;
    uint64_t *vis = a.vis + off, *nxt = a.nxt + off;
    const uint64_t *cur = a.cur + off;
    const int64_t stride = (int64_t)gridDim.x * GS_BLOCK;
    uint32_t cnt = 0;   // lane b: vertices that source 64 g + b reached at this level (< 2^31)
    for (int64_t base = (int64_t)blockIdx.x * GS_BLOCK + (threadIdx.x & ~63); base < a.n; base += stride) {
        const int64_t v = base + lane;
        const uint64_t w = v < a.n ? gs_frontier_pull(a.ptr, a.adj, vis, cur, nxt, v) : 0;
        if (__ballot(w != 0) == 0) continue;
#pragma unroll 8
        for (int b = 0; b < 64; ++b) {
            const uint64_t col = __ballot((w >> b) & 1);
            if (lane == b) cnt += (uint32_t)__popcll(col);
        }
    }
    if (cnt) {
        const int64_t j = g * 64 + lane;
        atomicAdd(&a.reached[j], (gs_u64)cnt);
        atomicAdd(&a.dist_sum[j], (gs_u64)cnt * (gs_u64)a.level);
        atomicMax(&a.ecc[j], a.level);
        if (gs_flag(&a.flags[a.level]) == 0) a.flags[a.level] = 1;
    }
}

// ---- triangles ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_BLOCK) void gs_triangle_kernel(int64_t n, int64_t arcs, const int64_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ adj, gs_u64 *tri) {
    GS_GRID_LOOP(e, arcs) {
        const int32_t v = adj[e];
        const int32_t u = gs_arc_row(ptr, n, e);
        if (v <= u) continue;
        const GsRows r = gs_rows(ptr, u, v);
        // both rows from their first entry above v
        const int64_t sb = gs_lower_bound(adj, r.sb, r.se, v + 1), lb = gs_lower_bound(adj, r.lb, r.le, v + 1);
        gs_u64 c = 0;
        gs_common_walk(adj, sb, r.se, lb, r.le, [&](int64_t k, int64_t) {
            ++c;
            atomicAdd(&tri[adj[k]], 1ull);
        });
        if (c) {
            atomicAdd(&tri[u], c);
            atomicAdd(&tri[v], c);
        }
    }
}

gh_status gs_components(gh_cent *h, int32_t *labels) {
    const int64_t n = h->n;
    gh_dev<int32_t> d_label, d_flags;
    if (!d_label.alloc(4 * n) || !d_flags.alloc(4 * (GS_CHECK_EVERY + 1))) {
        h->err = "hipMalloc failed for the component labels";
        return GH_ERR_NOMEM;
    }
    const int grid = gs_blocks(n);
    const int32_t one = 1;
    GH_HIP(hipMemcpyAsync(d_flags.p, &one, 4, hipMemcpyHostToDevice, h->stream));
    gs_label_init_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(n, d_label.p);
    GH_HIP(hipGetLastError());
    // a round that hooks lowers a label, so n rounds bound the loop from far above
    for (int64_t done = 0;; done += GS_CHECK_EVERY) {
        if (done > n + GS_CHECK_EVERY) { h->err = "component labels did not settle"; return GH_ERR_RUNTIME; }
        GH_HIP(hipMemsetAsync(d_flags.p + 1, 0, 4 * GS_CHECK_EVERY, h->stream));
        for (int32_t r = 1; r <= GS_CHECK_EVERY; ++r) {
            gs_hook_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, h->d_adj.p, d_label.p, d_flags.p, r);
            gs_jump_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(n, d_label.p, d_flags.p, r);
        }
        GH_HIP(hipGetLastError());
        int32_t last = 0;
        GH_HIP(hipMemcpyAsync(&last, d_flags.p + GS_CHECK_EVERY, 4, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (!last) break;
    }
    GH_HIP(hipMemcpyAsync(labels, d_label.p, 4 * n, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

// One batch of G groups holding ns <= 64 G sources; the level kernel adds to reached, dist_sum and eccentricity of the
// batch's sources, which start at zero.
gh_status gs_distance_batch(gh_cent *h, gs_frontier &f, int64_t G, const int32_t *src, int64_t ns, int32_t *d_src, gs_u64 *d_reached,
                            gs_u64 *d_dsum, int32_t *d_ecc) {
    const int64_t n = h->n;
    GH_HIP(hipMemcpyAsync(d_src, src, 4 * ns, hipMemcpyHostToDevice, h->stream));
    GH_TRY_ST(f.begin(h, G, ns, d_src, GS_MAX_BLOCKS));
    GsLevel a{};
    a.ptr = h->d_ptr.p; a.adj = h->d_adj.p;
    a.vis = f.vis.p; a.flags = f.flags.p;
    a.reached = d_reached; a.dist_sum = d_dsum; a.ecc = d_ecc;
    a.n = n;
    const int64_t per_row = std::max<int64_t>(1, GS_MAX_BLOCKS / G);
    const dim3 grid((unsigned)std::min<int64_t>(per_row, (n + GS_BLOCK - 1) / GS_BLOCK), (unsigned)G);
    int32_t last_level = 0;   // the kernel keeps the eccentricities itself
    return gh_level_loop(h, n, f.flags.p, GS_CHECK_EVERY, &last_level, [&](int32_t L) -> gh_status {
        a.level = L;
        a.cur = f.cur(L);
        a.nxt = f.nxt(L);
        gs_level_kernel<<<grid, dim3(GS_BLOCK), 0, h->stream>>>(a);
        GH_HIP(hipGetLastError());
        return GH_OK;
    });
}

}  // namespace

extern "C" gh_status gh_cent_components(gh_cent_handle h, int32_t *labels, int64_t *n_components) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (!labels && h->n > 0) { h->err = "labels must not be NULL"; return GH_ERR_INVALID; }
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    if (h->n > 0) {
        const gh_status st = gs_components(h, labels);
        if (st != GH_OK) { (void)hipStreamSynchronize(h->stream); return st; }
    }
    if (n_components) {
        int64_t c = 0;
        for (int64_t v = 0; v < h->n; ++v) c += labels[v] == v;
        *n_components = c;
    }
    return GH_OK;
}

extern "C" gh_status gh_cent_distances(gh_cent_handle h, int64_t n_sources, const int32_t *sources, int64_t *reached,
                                       int64_t *dist_sum, int32_t *eccentricity) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    auto fail = [&](gh_status st, const std::string &msg) { h->err = msg; return st; };
    if (n_sources < 0 || (n_sources > 0 && !sources)) return fail(GH_ERR_INVALID, "bad source list");
    for (int64_t i = 0; i < n_sources; ++i)
        if (sources[i] < 0 || sources[i] >= h->n) return fail(GH_ERR_INVALID, "source id outside [0, n)");
    if (n_sources == 0 || (!reached && !dist_sum && !eccentricity)) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) return fail(GH_ERR_RUNTIME, "hipSetDevice failed");
    const int64_t n = h->n, groups = (n_sources + 63) / 64;
    int64_t G = std::max<int64_t>(1, h->budget / (24 * n));   // 3 words per (group, vertex)
    G = std::min<int64_t>({G, groups, (int64_t)65535});       // 65535: grid.y
    gs_frontier f;
    gh_dev<int32_t> d_src, d_ecc;
    gh_dev<gs_u64> d_cnt;   // reached beyond the source itself, then dist_sum
    if (!f.alloc(G, n) || !d_src.alloc(4 * 64 * G) || !d_cnt.alloc(16 * 64 * groups) || !d_ecc.alloc(4 * 64 * groups))
        return fail(GH_ERR_NOMEM, "hipMalloc failed for " + std::to_string(G) + " source groups of distance state");
    auto run = [&]() -> gh_status {
        GH_HIP(hipMemsetAsync(d_cnt.p, 0, 16 * 64 * groups, h->stream));
        GH_HIP(hipMemsetAsync(d_ecc.p, 0, 4 * 64 * groups, h->stream));
        for (int64_t g0 = 0; g0 < groups; g0 += G) {
            const int64_t gb = std::min(G, groups - g0);
            const int64_t ns = std::min<int64_t>(64 * gb, n_sources - 64 * g0);
            GH_TRY_ST(gs_distance_batch(h, f, gb, sources + 64 * g0, ns, d_src.p, d_cnt.p + 64 * g0, d_cnt.p + 64 * groups + 64 * g0,
                                        d_ecc.p + 64 * g0));
        }
        if (reached) GH_HIP(hipMemcpyAsync(reached, d_cnt.p, 8 * n_sources, hipMemcpyDeviceToHost, h->stream));
        if (dist_sum) GH_HIP(hipMemcpyAsync(dist_sum, d_cnt.p + 64 * groups, 8 * n_sources, hipMemcpyDeviceToHost, h->stream));
        if (eccentricity) GH_HIP(hipMemcpyAsync(eccentricity, d_ecc.p, 4 * n_sources, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        for (int64_t i = 0; reached && i < n_sources; ++i) reached[i] += 1;   // the source itself
        return GH_OK;
    };
    const gh_status st = run();
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}

extern "C" gh_status gh_cent_triangles(gh_cent_handle h, int64_t *triangles) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (!triangles && h->n > 0) { h->err = "triangles must not be NULL"; return GH_ERR_INVALID; }
    if (h->n == 0) return GH_OK;
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    const int64_t n = h->n, arcs = 2 * h->edges;
    gh_dev<gs_u64> d_tri;
    if (!d_tri.alloc(8 * n)) { h->err = "hipMalloc failed for the triangle counts"; return GH_ERR_NOMEM; }
    auto run = [&]() -> gh_status {
        GH_HIP(hipMemsetAsync(d_tri.p, 0, 8 * n, h->stream));
        if (arcs > 0) {
            gs_triangle_kernel<<<dim3(gs_blocks(arcs)), dim3(GS_BLOCK), 0, h->stream>>>(n, arcs, h->d_ptr.p, h->d_adj.p, d_tri.p);
            GH_HIP(hipGetLastError());
        }
        GH_HIP(hipMemcpyAsync(triangles, d_tri.p, 8 * n, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        return GH_OK;
    };
    const gh_status st = run();
    if (st != GH_OK) (void)hipStreamSynchronize(h->stream);
    return st;
}
