// The graph plan of a float32 engine (engine.h gh_graph_plan), built on the host before anything is allocated: the internal
// vertex order, which endpoint owns an edge, the pull lists, the owned-edge tables, the vertex blocks of the fused
// workgroups, the KNN method GH_KNN_AUTO picks and the threshold subset's endpoints.  No HIP calls.
#include "common.h"
#include "engine.h"

#include <algorithm>

namespace {

// Pull lists of the rows [lo, hi) in the reference's summation order (pt.py:633-634): first the edges where the vertex is
// endpoint 0, then those where it is endpoint 1, each in edge-list order.  owner(e): the endpoint (0 / 1) that owns edge e,
// -1 neither; bit 31 of an entry marks the edges its row OWNS (emits the midpoint of, and searches in the KNN phase).
// eid: the edge id of every entry, or null.
template <class Owner>
void pull_lists(int64_t lo, int64_t hi, int64_t E, const int32_t *edges, const Owner &owner, std::vector<int32_t> &rowptr,
                std::vector<int32_t> &adj, std::vector<int32_t> *eid) {
    const int64_t rows = hi - lo;
    rowptr.assign((size_t)rows + 1, 0);
    for (int64_t e = 0; e < E; ++e) {
        const int32_t u = edges[2 * e], v = edges[2 * e + 1];
        if (u >= lo && u < hi) rowptr[(size_t)(u - lo) + 1]++;
        if (v >= lo && v < hi) rowptr[(size_t)(v - lo) + 1]++;
    }
    for (int64_t i = 0; i < rows; ++i) rowptr[(size_t)i + 1] += rowptr[(size_t)i];
    const size_t len = (size_t)std::max<int64_t>(rowptr[(size_t)rows], 1);
    adj.assign(len, 0);
    if (eid) eid->assign(len, 0);
    std::vector<int32_t> cur(rowptr.begin(), rowptr.end() - 1);
    for (int64_t e = 0; e < E; ++e) {
        const int32_t u = edges[2 * e], v = edges[2 * e + 1];
        if (u >= lo && u < hi) {
            const size_t at = (size_t)cur[(size_t)(u - lo)]++;
            adj[at] = (int32_t)((uint32_t)v | (owner(e) == 0 ? 0x80000000u : 0u));
            if (eid) (*eid)[at] = (int32_t)e;
        }
    }
    for (int64_t e = 0; e < E; ++e) {
        const int32_t u = edges[2 * e], v = edges[2 * e + 1];
        if (v >= lo && v < hi) {
            const size_t at = (size_t)cur[(size_t)(v - lo)]++;
            adj[at] = (int32_t)((uint32_t)u | (owner(e) == 1 ? 0x80000000u : 0u));
            if (eid) (*eid)[at] = (int32_t)e;
        }
    }
}

// Internal vertex order (include/graphem_hip.h GH_REORDER_*): breadth-first numbers, components in order of their smallest
// vertex, children in edge id order.  order[v] = internal number of vertex v.
std::vector<int32_t> bfs_order(int64_t n, int64_t E, const int32_t *edges) {
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t e = 0; e < E; ++e) { off[(size_t)edges[2 * e] + 1]++; off[(size_t)edges[2 * e + 1] + 1]++; }
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] += off[(size_t)i];
    std::vector<int32_t> nb((size_t)off[(size_t)n]);
    {
        std::vector<int64_t> cur(off.begin(), off.end() - 1);
        for (int64_t e = 0; e < E; ++e) {
            const int32_t u = edges[2 * e], v = edges[2 * e + 1];
            nb[(size_t)cur[(size_t)u]++] = v;
            nb[(size_t)cur[(size_t)v]++] = u;
        }
    }
    std::vector<int32_t> order((size_t)n, -1), queue((size_t)n);
    int64_t head = 0, tail = 0, next = 0;
    for (int64_t root = 0; root < n; ++root) {
        if (order[(size_t)root] >= 0) continue;
        order[(size_t)root] = (int32_t)next++;
        queue[(size_t)tail++] = (int32_t)root;
        while (head < tail) {
            const int32_t x = queue[(size_t)head++];
            for (int64_t j = off[(size_t)x]; j < off[(size_t)x + 1]; ++j) {
                const int32_t y = nb[(size_t)j];
                if (order[(size_t)y] < 0) { order[(size_t)y] = (int32_t)next++; queue[(size_t)tail++] = y; }
            }
        }
    }
    // Within blocks of 16384 consecutive breadth-first numbers, rows in order of falling degree: the lanes of a wave
    // walk their pull lists in lock-step, so a wave costs its LONGEST list.  G(n, p) at 1 M vertices (Poisson
    // degrees, mean 10): fused kernel 172.5 -> 163 us with blocks of 8 K - 32 K rows, 168 with 256, 170 - 172 with
    // 256 K or the whole graph (the breadth-first locality is gone); a regular graph is left as it is (stable sort).
    const int64_t B = 16384;
    std::vector<int32_t> inv((size_t)n);
    for (int64_t v = 0; v < n; ++v) inv[(size_t)order[(size_t)v]] = (int32_t)v;
    for (int64_t b0 = 0; b0 < n; b0 += B) {
        const int64_t b1 = std::min(n, b0 + B);
        std::stable_sort(inv.begin() + b0, inv.begin() + b1, [&](int32_t a, int32_t c) {
            return off[(size_t)a + 1] - off[(size_t)a] > off[(size_t)c + 1] - off[(size_t)c];
        });
    }
    for (int64_t i = 0; i < n; ++i) order[(size_t)inv[(size_t)i]] = (int32_t)i;
    return order;
}

// Which endpoint owns an edge.  GH_EDGES_RANGE: the edges [edge_lo, edge_hi), each owned by its endpoint 0.
// GH_EDGES_HASHED: a hash of the edge id picks the owning endpoint, so every rank owns ~E/world edges whatever the vertex
// numbering (with endpoint-0 ownership the low-numbered ranks of a u<v edge list hold most of the edges); an edge between
// a hub and a short row always belongs to the short row.
struct edge_owner {
    const gh_partition &part;
    const int32_t *edges;
    std::vector<int32_t> deg;   // over the WHOLE graph, so that every rank sees the same hubs
    int long_deg = 0;
    bool has_long = false;

    int operator()(int64_t e) const {
        if (part.edge_rule != GH_EDGES_HASHED) return e >= part.edge_lo && e < part.edge_hi ? 0 : -1;
        if (has_long) {
            const int32_t du = deg[(size_t)edges[2 * e]], dv = deg[(size_t)edges[2 * e + 1]];
            const bool lu = du > long_deg, lv = dv > long_deg;
            if (lu != lv) return lu ? 1 : 0;
            // between two long rows the one with FEWER neighbours owns the edge (equal degrees: the hash): a hub then owns
            // edges to bigger hubs only, and no row owns more than a fused workgroup's tile (a 1045-degree hub of a graph whose
            // rows are all long owned 520 edges by the hash alone and forced the whole engine onto its unfused kernels)
            if (lu && du != dv) return du > dv ? 1 : 0;
        }
        uint32_t x = (uint32_t)e * 0x9E3779B1u;
        x ^= x >> 15; x *= 0x85EBCA6Bu; x ^= x >> 13;
        return (int)(x >> 31);
    }
};

// Hubs (common.h GH_LONG_DEG): rows with more than gh_long_degree neighbours.  A graph that has any takes the flagged
// ownership rule (it lets the short endpoint of a hub's edge own it, so that no row owns more than a workgroup's tile);
// range partitions keep endpoint-0 ownership.
void find_hubs(const gh_engine *h, edge_owner &own) {
    own.deg.assign((size_t)h->n, 0);
    for (int64_t i = 0; i < 2 * h->E; ++i) own.deg[(size_t)own.edges[i]]++;
    for (int64_t i = 0; i < h->n && !own.has_long; ++i) own.has_long = own.deg[(size_t)i] > own.long_deg;
    if (own.part.edge_rule != GH_EDGES_HASHED) own.has_long = false;
}

// first_edge[i]: where the midpoints of row i's owned edges go.  Range rule, edges sorted by first endpoint (always true
// for the reference's CSR-order edge list): the owned edges of a row are consecutive ids and the offset is the first of
// them.  Hashed rule: a prefix count into the list own_eids of owned edge ids in (row, pull list) order.
void owned_edges(gh_engine *h, const std::vector<int32_t> &adj_eid, gh_graph_plan *g) {
    const int64_t rows = h->rows, E = h->E;
    g->first_edge.assign((size_t)rows + 1, 0);
    if (h->part.edge_rule == GH_EDGES_HASHED) {
        g->own_eids.reserve((size_t)(E / std::max<int64_t>(1, h->n / std::max<int64_t>(rows, 1)) + 16));
        for (int64_t i = 0; i < rows; ++i) {
            g->first_edge[(size_t)i] = (int32_t)g->own_eids.size();
            for (int32_t j = g->rowptr[(size_t)i]; j < g->rowptr[(size_t)i + 1]; ++j)
                if ((uint32_t)g->adj[(size_t)j] >> 31) g->own_eids.push_back(adj_eid[(size_t)j]);
        }
        g->first_edge[(size_t)rows] = (int32_t)g->own_eids.size();
        h->own_count = (int64_t)g->own_eids.size();
        h->mid_base = 0;
        h->fused_mid = true;
    } else {
        const int32_t *edges = g->edges;
        bool sorted = true;
        for (int64_t e = 1; e < E && sorted; ++e) sorted = edges[2 * e] >= edges[2 * (e - 1)];
        if (sorted) {
            int64_t e = 0;
            for (int64_t i = 0; i <= rows; ++i) {
                const int64_t x = h->part.row_lo + i;
                while (e < E && edges[2 * e] < x) ++e;
                g->first_edge[(size_t)i] = (int32_t)e;
            }
            h->fused_mid = g->first_edge[0] == h->part.edge_lo && g->first_edge[(size_t)rows] == h->part.edge_hi;
        }
        h->own_count = h->part.edge_hi - h->part.edge_lo;
        h->mid_base = h->part.edge_lo;
    }
}

// The own hub rows and the (hub-hub) edges they own, for spring_long_kernel / spring_row (hashed rule only).
void long_rows(gh_engine *h, gh_graph_plan *g) {
    const std::vector<int32_t> &rowptr = g->rowptr, &adj = g->adj;
    g->long_ownptr.push_back(0);
    g->long_eptr.push_back(0);
    for (int64_t i = 0; i < h->rows; ++i) {
        if (rowptr[(size_t)i + 1] - rowptr[(size_t)i] <= h->long_deg) continue;
        g->long_rows.push_back((int32_t)i);
        g->long_eptr.push_back(g->long_eptr.back() + (rowptr[(size_t)i + 1] - rowptr[(size_t)i]));
        for (int32_t j = rowptr[(size_t)i]; j < rowptr[(size_t)i + 1]; ++j)
            if ((uint32_t)adj[(size_t)j] >> 31) g->long_ownadj.push_back((int32_t)((uint32_t)adj[(size_t)j] & 0x7FFFFFFFu));
        g->long_ownptr.push_back((int32_t)g->long_ownadj.size());
    }
    const std::vector<int32_t> &eptr = g->long_eptr;
    h->nlong = (int)g->long_rows.size();
    h->long_entries = eptr.back();
    for (size_t r = 0; r + 1 < eptr.size(); ++r) h->long_max_deg = std::max(h->long_max_deg, (int)(eptr[r + 1] - eptr[r]));
    g->long_erow.resize((size_t)h->long_entries);   // list entry -> index of its long row (spares long_terms_kernel a binary search)
    for (size_t r = 0; r + 1 < eptr.size(); ++r)
        for (int32_t t = eptr[r]; t < eptr[r + 1]; ++t) g->long_erow[(size_t)t] = (int32_t)r;
    g->own_long.assign(g->own_eids.size() + 1, 0);   // owned-edge slots of the long rows
    for (int64_t i = 0; i < h->rows; ++i)
        if (rowptr[(size_t)i + 1] - rowptr[(size_t)i] > h->long_deg)
            for (int32_t sl = g->first_edge[(size_t)i]; sl < (i + 1 < h->rows ? g->first_edge[(size_t)i + 1] : (int32_t)g->own_eids.size()); ++sl)
                g->own_long[(size_t)sl] = 1;
}

// Vertex ranges of the fused spring+scan workgroups: as many consecutive own rows as hold at most TILE owned edges (and at
// most 1024 rows, 4 per thread).
void fused_blocks(gh_engine *h, gh_graph_plan *g) {
    const int tile = GH_FUSED_TILE;
    bool ok = h->fused_mid && gh_dim_templated(h->D);
    std::vector<int32_t> &vblock = g->vblock;
    if (ok) {
        vblock.push_back(0);
        int64_t i = 0;
        while (i < h->rows && ok) {
            int64_t j = i, cnt = 0;
            while (j < h->rows && j - i < 1024) {
                const int64_t own = g->first_edge[(size_t)j + 1] - g->first_edge[(size_t)j];
                if (own > tile) { ok = false; break; }  // a single row owns more than a tile: unfused path
                if (cnt + own > tile) break;
                cnt += own;
                ++j;
            }
            if (!ok) break;
            vblock.push_back((int32_t)j);
            i = j;
        }
    }
    h->fused_scan = ok;
    if (!ok) vblock.assign(1, 0);
    h->n_vblocks = (int)vblock.size() - 1;
}

}  // namespace

void gh_pull_lists(int64_t n, int64_t E, const int32_t *edges, std::vector<int32_t> &rowptr, std::vector<int32_t> &adj) {
    pull_lists(0, n, E, edges, [](int64_t) { return -1; }, rowptr, adj, nullptr);
}

void gh_plan_graph(gh_engine *h, const int32_t *edges, bool partitioned, int reorder, gh_graph_plan *g) {
    const int64_t n = h->n, E = h->E;
    // A whole-graph engine always takes the hashed rule: under "endpoint 0 owns" vertex i of a u < v edge list owns its
    // edges to higher-numbered neighbours only -- 8 for the first vertices of an 8-regular graph, 0 for the last -- so the
    // fused workgroups at the end of the vertex range held 1024 rows for a few hundred owned edges and took 31 us where the
    // median workgroup took 18 (tools/stamp_probe.py, 100 K vertices): they were the length of the kernel.
    if (!partitioned) h->part = gh_partition{0, n, 0, 0, GH_EDGES_HASHED};
    const bool hashed = h->part.edge_rule == GH_EDGES_HASHED;

    const bool l2_miss = (double)n * h->LD * sizeof(float) > 3.0 * 1024 * 1024;
    if (hashed && E > 0 && (reorder == GH_REORDER_BFS || (reorder == GH_REORDER_AUTO && l2_miss))) {
        h->order_host = bfs_order(n, E, edges);
        g->internal.resize((size_t)E * 2);
        for (int64_t i = 0; i < 2 * E; ++i) g->internal[(size_t)i] = h->order_host[(size_t)edges[i]];
        edges = g->internal.data();  // everything below works on internal vertex numbers
    }
    g->edges = edges;

    edge_owner own{h->part, edges};
    h->long_deg = own.long_deg = gh_long_degree(n, E);
    find_hubs(h, own);

    std::vector<int32_t> adj_eid;
    pull_lists(h->part.row_lo, h->part.row_hi, E, edges, own, g->rowptr, g->adj, hashed ? &adj_eid : nullptr);
    h->adj_len = g->rowptr[(size_t)h->rows];
    owned_edges(h, adj_eid, g);
    if (own.has_long) long_rows(h, g);
    fused_blocks(h, g);
}

// GH_KNN_AUTO: exact methods only.  Up to 8 components and thousands of queries over >= 262144 searched (own) edges: the
// inverted file in its exact mode (rr1m, scan / exact IVF us per iteration: D = 3 S = 4096 1063 / 591, 16384 3691 / 766 (grid
// 1926); D = 6 S = 16384 5059 / 1401; D = 8 5264 / 2135; 100 K vertices D = 3 S = 4096 384 / 191;
// profiles/r03/knn_method_sweep.log); else the grid for <= 3 components from 12288 queries on; else the scan.  With
// GH_DIST_CDIST always the scan: the other searches know exact distances only.
void gh_auto_knn_method(gh_engine *h) {
    const int D = h->D;
    const bool ivf = !h->cdist && D >= 2 && D <= 8 && h->S >= (D <= 4 ? 4096 : 8192) && h->own_count >= 262144;
    h->prm.knn_method = h->cdist ? GH_KNN_SCAN : ivf ? GH_KNN_IVF : (D <= 3 && h->S >= 12288) ? GH_KNN_GRID : GH_KNN_SCAN;
    if (ivf) { h->prm.ivf_probes = -1; h->prm.ivf_lists = 0; }
}

void gh_plan_threshold_subset(const gh_engine *h, gh_graph_plan *g) {
    g->sub_uv.resize((size_t)h->plan.thr_M1 * 2);
    const bool hashed = h->part.edge_rule == GH_EDGES_HASHED;
    for (int64_t j = 0; j < h->plan.thr_M1; ++j) {   // every thr_stride-th own edge
        const int64_t e = hashed ? (int64_t)g->own_eids[(size_t)(j * h->plan.thr_stride)] : h->part.edge_lo + j * h->plan.thr_stride;
        g->sub_uv[(size_t)(2 * j)] = g->edges[2 * e];
        g->sub_uv[(size_t)(2 * j + 1)] = g->edges[2 * e + 1];
    }
}
