// Core and truss decomposition on the GPU (include/graphem_hip.h "cores and trusses"; graphem-rapids_amd/cores.py): two
// synchronous peels over the centrality handle's deduplicated symmetric CSR (neighbours ascending).  Everything is an
// integer, and within a launch the only words two workgroups share are integer atomics whose final value a LATER launch
// reads: no result depends on the order of an atomic, no workgroup waits for another.
//
// Both peels run the same round over `items` (vertices or edges) with a value val[] (degree or support), a removal stamp
// stamp[] (0: alive, else the round it left in) and seven scalars on the device (CrCtl).  One step is three launches:
//   cr_select_kernel   every alive item with val <= k leaves: stamp = r, and val = k + bonus is its result from here on
//                      (core number: bonus 0; truss number: bonus 2).  Counts the leavers and, over the stayers, takes the
//                      minimum of val -- one add and one min per wave.
//   the push kernel    every leaver takes what it owes from the stayers (below).  Stamps are read only, val of a stayer
//                      only ever drops by atomicSub, val of a leaver is never touched again.
//   cr_step_kernel     one thread.  Leavers: alive -= them, rounds = r, r += 1, done when nobody is alive.  No leaver: the
//                      minimum was taken before anything changed, so k = that minimum, and the next step removes
//                      something; such a step has no round number.
// A finished peel makes every later launch return at once; the host reads the scalars every GS_CHECK_EVERY steps.
//
// Vertex push (cr_vertex_push_kernel): a leaver walks its row and takes 1 from the degree of every neighbour that is
// still alive (stamp 0) -- a neighbour that leaves in the same round has this round's stamp and keeps its value.
//
// Edge set-up: up[u] = the entries of row u above u, scanned to base[]; the upper arc at position a of row u is edge
// base[u] + (a - first upper position of u), the canonical id, and a lower arc (u, v) finds its twin by one bisection of
// row v.  eid[arc] = that id, eu[e] / ea[e] = the lower endpoint and the upper arc's position.  sup[e] = the common
// neighbours of e's endpoints (the shorter row searched in the longer one: gs_common_walk of csr_core.h, as in
// gs_triangle_kernel).
// Edge push (cr_edge_push_kernel): a leaver e = (u, v) intersects the two rows again.  For a common neighbour w the stamps
// of (u, w) and (v, w) say: dead before this round -- the triangle was; leaving now with a smaller id than e -- that edge
// accounts for the triangle; otherwise e takes 1 from the support of each of the two that stays.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "cent_handle.h"
#include "csr_core.h"

namespace {

struct CrCtl {
    int32_t k;          // the threshold: core number, or truss number - 2, of whatever leaves next
    int32_t r;          // the number the next round that removes something gets (from 1)
    int32_t alive;
    int32_t selected;   // leavers of the step in flight
    int32_t mn;         // min val over its stayers
    int32_t done;
    int32_t rounds;     // rounds that removed something
};

__global__ void cr_ctl_init_kernel(CrCtl *c, int32_t items) {
    c->k = 0; c->r = 1; c->alive = items; c->selected = 0; c->mn = INT32_MAX; c->done = 0; c->rounds = 0;
}

__global__ __launch_bounds__(GS_BLOCK) void cr_degree_kernel(int64_t n, const int64_t *__restrict__ ptr, int32_t *deg, int32_t *stamp) {
    GS_GRID_LOOP(v, n) {
        deg[v] = (int32_t)(ptr[v + 1] - ptr[v]);
        stamp[v] = 0;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void cr_select_kernel(int64_t items, int32_t *val, int32_t *stamp, CrCtl *c, int32_t bonus) {
    if (gs_flag(&c->done)) return;
    const int32_t k = c->k, r = c->r;
    int32_t cnt = 0, mn = INT32_MAX;
    GS_GRID_LOOP(i, items) {
        if (stamp[i] != 0) continue;
        const int32_t x = val[i];
        if (x <= k) {
            stamp[i] = r;
            val[i] = k + bonus;
            ++cnt;
        } else {
            mn = min(mn, x);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        mn = min(mn, __shfl_xor(mn, off));
    }
    if ((threadIdx.x & 63) == 0) {
        if (cnt) atomicAdd(&c->selected, cnt);
        if (mn != INT32_MAX) atomicMin(&c->mn, mn);
    }
}

__global__ void cr_step_kernel(CrCtl *c) {
    if (c->done) return;
    const int32_t sel = c->selected;
    if (sel > 0) {
        c->alive -= sel;
        c->rounds = c->r;
        c->r += 1;
        if (c->alive <= 0) c->done = 1;
    } else {
        c->k = c->mn;   // somebody is alive and nobody left: every alive val is above k, and mn is their minimum
    }
    c->selected = 0;
    c->mn = INT32_MAX;
}

__global__ __launch_bounds__(GS_BLOCK) void cr_vertex_push_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                                  int32_t *deg, const int32_t *__restrict__ stamp, const CrCtl *c) {
    if (gs_flag(&c->done) || gs_flag(&c->selected) == 0) return;
    const int32_t r = c->r;
    GS_GRID_LOOP(v, n) {
        if (stamp[v] != r) continue;
        const int64_t beg = ptr[v], end = ptr[v + 1];
        for (int64_t k = beg; k < end; ++k) {
            const int32_t w = adj[k];
            if (stamp[w] == 0) atomicSub(&deg[w], 1);
        }
    }
}

// ---- edges ----------------------------------------------------------------------------------------------------------
// up[u] = entries of row u above u; up[n] = 0 closes the scan
__global__ __launch_bounds__(GS_BLOCK) void cr_upper_count_kernel(int64_t n, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                                  int64_t *up) {
    GS_GRID_LOOP(u, n + 1) up[u] = u < n ? ptr[u + 1] - gs_lower_bound(adj, ptr[u], ptr[u + 1], (int32_t)u + 1) : 0;
}

__global__ __launch_bounds__(GS_BLOCK) void cr_edge_id_kernel(int64_t n, int64_t arcs, const int64_t *__restrict__ ptr,
                                                              const int32_t *__restrict__ adj, const int64_t *__restrict__ base,
                                                              int32_t *eid, int32_t *eu, int32_t *ea, int32_t *stamp) {
    GS_GRID_LOOP(a, arcs) {
        const int32_t u = gs_arc_row(ptr, n, a), v = adj[a];
        if (v > u) {
            const int64_t first = ptr[u + 1] - (base[u + 1] - base[u]);
            const int64_t e = base[u] + (a - first);
            eid[a] = (int32_t)e;
            eu[e] = u;
            ea[e] = (int32_t)a;
            stamp[e] = 0;
        } else {
            const int64_t first = ptr[v + 1] - (base[v + 1] - base[v]);
            eid[a] = (int32_t)(base[v] + (gs_lower_bound(adj, first, ptr[v + 1], u) - first));
        }
    }
}

__global__ __launch_bounds__(GS_BLOCK) void cr_support_kernel(int64_t edges, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                              const int32_t *__restrict__ eu, const int32_t *__restrict__ ea, int32_t *sup) {
    GS_GRID_LOOP(e, edges) {
        const GsRows w = gs_rows(ptr, eu[e], adj[ea[e]]);
        int32_t c = 0;
        gs_common_walk(adj, w.sb, w.se, w.lb, w.le, [&](int64_t, int64_t) { ++c; });
        sup[e] = c;
    }
}

__global__ __launch_bounds__(GS_BLOCK) void cr_edge_push_kernel(int64_t edges, const int64_t *__restrict__ ptr, const int32_t *__restrict__ adj,
                                                                const int32_t *__restrict__ eid, const int32_t *__restrict__ eu,
                                                                const int32_t *__restrict__ ea, int32_t *sup,
                                                                const int32_t *__restrict__ stamp, const CrCtl *c) {
    if (gs_flag(&c->done) || gs_flag(&c->selected) == 0) return;
    const int32_t r = c->r;
    GS_GRID_LOOP(e, edges) {
        if (stamp[e] != r) continue;
        const GsRows w = gs_rows(ptr, eu[e], adj[ea[e]]);
        gs_common_walk(adj, w.sb, w.se, w.lb, w.le, [&](int64_t k, int64_t at) {
            const int32_t e1 = eid[k], e2 = eid[at];   // the triangle's other two edges
            const int32_t g1 = stamp[e1], g2 = stamp[e2];
            if ((g1 != 0 && g1 != r) || (g2 != 0 && g2 != r)) return;   // dead before this round
            if ((g1 == r && e1 < e) || (g2 == r && e2 < e)) return;     // charged to a leaver of smaller id
            if (g1 == 0) atomicSub(&sup[e1], 1);
            if (g2 == 0) atomicSub(&sup[e2], 1);
        });
    }
}

// Steps until nobody is alive.  A step that removes nothing raises k, which stays below `items`, and a step that removes
// something removes at least one of `items`: 2 (items + 1) steps bound the loop from above.
template <class Push>
gh_status cr_peel_loop(gh_cent *h, int64_t items, int32_t *val, int32_t *stamp, CrCtl *d_ctl, int32_t bonus, int32_t *rounds, Push push) {
    const int grid = gs_blocks(items);
    cr_ctl_init_kernel<<<dim3(1), dim3(1), 0, h->stream>>>(d_ctl, (int32_t)items);
    GH_HIP(hipGetLastError());
    CrCtl ctl{};
    for (int64_t steps = 0;; steps += GS_CHECK_EVERY) {
        if (steps > 2 * (items + 1) + GS_CHECK_EVERY || ctl.rounds > items + 1) { h->err = "peel did not settle"; return GH_ERR_RUNTIME; }
        for (int i = 0; i < GS_CHECK_EVERY; ++i) {
            cr_select_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(items, val, stamp, d_ctl, bonus);
            push();
            cr_step_kernel<<<dim3(1), dim3(1), 0, h->stream>>>(d_ctl);
        }
        GH_HIP(hipGetLastError());
        GH_HIP(hipMemcpyAsync(&ctl, d_ctl, sizeof(CrCtl), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (ctl.done) break;
    }
    *rounds = ctl.rounds;
    return GH_OK;
}

gh_status cr_cores(gh_cent *h, int32_t *core, int32_t *layer, int32_t *n_rounds) {
    const int64_t n = h->n;
    gh_dev<int32_t> d_deg, d_stamp;
    gh_dev<CrCtl> d_ctl;
    if (!d_deg.alloc(4 * n) || !d_stamp.alloc(4 * n) || !d_ctl.alloc(sizeof(CrCtl))) {
        h->err = "hipMalloc failed for the vertex peel";
        return GH_ERR_NOMEM;
    }
    const int grid = gs_blocks(n);
    cr_degree_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, d_deg.p, d_stamp.p);
    GH_HIP(hipGetLastError());
    GH_TRY_ST(cr_peel_loop(h, n, d_deg.p, d_stamp.p, d_ctl.p, 0, n_rounds, [&]() {
        cr_vertex_push_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, h->d_adj.p, d_deg.p, d_stamp.p, d_ctl.p);
    }));
    if (core) GH_HIP(hipMemcpyAsync(core, d_deg.p, 4 * n, hipMemcpyDeviceToHost, h->stream));
    if (layer) GH_HIP(hipMemcpyAsync(layer, d_stamp.p, 4 * n, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

gh_status cr_truss(gh_cent *h, int32_t *truss, int32_t *n_rounds) {
    const int64_t n = h->n, edges = h->edges, arcs = 2 * edges;
    gh_dev<int32_t> d_eid, d_eu, d_ea, d_sup, d_stamp;
    gh_dev<CrCtl> d_ctl;
    if (!d_eid.alloc(4 * arcs) || !d_eu.alloc(4 * edges) || !d_ea.alloc(4 * edges) || !d_sup.alloc(4 * edges) ||
        !d_stamp.alloc(4 * edges) || !d_ctl.alloc(sizeof(CrCtl))) {
        h->err = "hipMalloc failed for the edge peel";
        return GH_ERR_NOMEM;
    }
    {   // edge ids; the scan's arrays go when they are built
        gh_dev<int64_t> d_up, d_base;
        gh_dev<char> d_tmp;
        size_t temp = 0;
        GH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, temp, (const int64_t *)nullptr, (int64_t *)nullptr, (int)(n + 1), h->stream));
        if (!d_up.alloc(8 * (n + 1)) || !d_base.alloc(8 * (n + 1)) || !d_tmp.alloc(temp)) {
            h->err = "hipMalloc failed for the edge ids";
            return GH_ERR_NOMEM;
        }
        cr_upper_count_kernel<<<dim3(gs_blocks(n + 1)), dim3(GS_BLOCK), 0, h->stream>>>(n, h->d_ptr.p, h->d_adj.p, d_up.p);
        GH_HIP(hipGetLastError());
        GH_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, temp, (const int64_t *)d_up.p, d_base.p, (int)(n + 1), h->stream));
        cr_edge_id_kernel<<<dim3(gs_blocks(arcs)), dim3(GS_BLOCK), 0, h->stream>>>(n, arcs, h->d_ptr.p, h->d_adj.p, d_base.p, d_eid.p, d_eu.p,
                                                                                   d_ea.p, d_stamp.p);
        GH_HIP(hipGetLastError());
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    const int grid = gs_blocks(edges);
    cr_support_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(edges, h->d_ptr.p, h->d_adj.p, d_eu.p, d_ea.p, d_sup.p);
    GH_HIP(hipGetLastError());
    GH_TRY_ST(cr_peel_loop(h, edges, d_sup.p, d_stamp.p, d_ctl.p, 2, n_rounds, [&]() {
        cr_edge_push_kernel<<<dim3(grid), dim3(GS_BLOCK), 0, h->stream>>>(edges, h->d_ptr.p, h->d_adj.p, d_eid.p, d_eu.p, d_ea.p, d_sup.p,
                                                                          d_stamp.p, d_ctl.p);
    }));
    GH_HIP(hipMemcpyAsync(truss, d_sup.p, 4 * edges, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

// The arc positions, edge ids and counters above are int32.
bool cr_fits(gh_cent *h) {
    if (2 * h->edges <= (int64_t)INT32_MAX && h->n < (int64_t)INT32_MAX) return true;
    h->err = "cores and trusses need at most 2^31 - 1 arcs, this graph has " + std::to_string(2 * h->edges);
    return false;
}

}  // namespace

extern "C" gh_status gh_cent_cores(gh_cent_handle h, int32_t *core, int32_t *layer, int32_t *n_rounds) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    int32_t rounds = 0;
    if (n_rounds) *n_rounds = 0;
    if (h->n == 0) return GH_OK;
    if (!cr_fits(h)) return GH_ERR_INVALID;
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    const gh_status st = cr_cores(h, core, layer, &rounds);
    if (st != GH_OK) { (void)hipStreamSynchronize(h->stream); return st; }
    if (n_rounds) *n_rounds = rounds;
    return GH_OK;
}

extern "C" gh_status gh_cent_truss(gh_cent_handle h, int32_t *truss, int32_t *n_rounds) {
    if (!h) { cent_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    int32_t rounds = 0;
    if (n_rounds) *n_rounds = 0;
    if (h->n == 0 || h->edges == 0) return GH_OK;
    if (!truss) { h->err = "truss must not be NULL"; return GH_ERR_INVALID; }
    if (!cr_fits(h)) return GH_ERR_INVALID;
    if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return GH_ERR_RUNTIME; }
    const gh_status st = cr_truss(h, truss, &rounds);
    if (st != GH_OK) { (void)hipStreamSynchronize(h->stream); return st; }
    if (n_rounds) *n_rounds = rounds;
    return GH_OK;
}
