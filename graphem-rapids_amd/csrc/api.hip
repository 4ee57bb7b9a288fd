// C ABI of libgraphem_hip.so (include/graphem_hip.h): handle lifetime, host<->device
// copies, the iteration driver and the per-phase entry points.
#include "common.h"
#include "engine.h"
#include "qcell_core.h"

#include "torch_randperm.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <stdlib.h>
#include <string.h>

static thread_local std::string g_create_error;
void gh_set_create_error(const std::string &msg) { g_create_error = msg; }

// ---- timing ------------------------------------------------------------------------
gh_scope::gh_scope(gh_engine *h_, const char *name, hipStream_t on) : h(h_), stream(on ? on : h_->stream) {
    if (!h->timing) return;
    for (size_t i = 0; i < h->timers.size(); ++i)
        if (h->timers[i].name == name) slot = (int)i;
    if (slot < 0) {
        h->timers.emplace_back();
        h->timers.back().name = name;
        slot = (int)h->timers.size() - 1;
    }
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, stream);
}
gh_scope::~gh_scope() {
    if (slot < 0) return;
    (void)hipEventRecord(b, stream);
    h->timers[slot].pending.emplace_back(a, b);
}

static void resolve_timers(gh_engine *h) {
    for (auto &t : h->timers) {
        for (auto &p : t.pending) {
            float ms = 0.f;
            (void)hipEventSynchronize(p.second);
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) { t.total_ms += ms; t.launches += 1; }
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        t.pending.clear();
    }
}

// ---- helpers -----------------------------------------------------------------------
static gh_status check_handle(gh_engine *h) {
    if (!h) return GH_ERR_INVALID;
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) {
        h->err = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return GH_ERR_HIP;
    }
    return GH_OK;
}

// Entry points of the float32 engine's internals have no meaning on a float64 engine (f64.hip).
static gh_status reject_f64(gh_engine *h, const char *what) {
    if (!h->f64) return GH_OK;
    h->err = std::string(what) + " is not available on a float64 engine";
    return GH_ERR_INVALID;
}

// ---- lifetime ----------------------------------------------------------------------
gh_status gh_check_create_args(int device_id, int64_t n, int32_t D, int64_t E, const int32_t *edges, const gh_params *params,
                               int f64_max_D, double f64_k_attr) {
    auto fail = [&](gh_status st, const std::string &msg) { g_create_error = msg; return st; };
    const bool f64 = f64_max_D > 0;
    if (n <= 0) return fail(GH_ERR_INVALID, "Adjacency matrix cannot be empty");
    if (D <= 0) return fail(GH_ERR_INVALID, "Number of components must be positive, got " + std::to_string(D));
    if (f64 && D > f64_max_D) return fail(GH_ERR_INVALID, "the float64 engine takes up to " + std::to_string(f64_max_D) + " components");
    if (!params) return fail(GH_ERR_INVALID, "params is NULL");
    if ((f64 ? f64_k_attr : params->k_attr) < 0) return fail(GH_ERR_INVALID, "Attractive force constant k_attr must be non-negative");
    if (E < 0 || (E > 0 && !edges)) return fail(GH_ERR_INVALID, "edges is NULL");
    if (params->n_neighbors < 0 || params->sample_size < 0) return fail(GH_ERR_INVALID, "negative n_neighbors / sample_size");
    const int64_t K = (int64_t)params->n_neighbors + 1;
    if (f64 && K > 256) return fail(GH_ERR_INVALID, "the float64 engine takes up to 255 neighbours");   // (before the size check)
    if (E >= ((int64_t)1 << 30) || n >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "graph too large for int32 ids");
    if (!f64 && K > GH_SEL_BUF - GH_SEL_CHUNK) return fail(GH_ERR_INVALID, "n_neighbors too large for the HIP backend (max 2047)");
    for (int64_t e = 0; e < E; ++e) {
        const int32_t u = edges[2 * e], v = edges[2 * e + 1];
        if (u < 0 || v < 0 || u >= n || v >= n) return fail(GH_ERR_INVALID, "edge endpoint out of range");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GH_ERR_HIP, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(GH_ERR_RUNTIME, "invalid device ordinal " + std::to_string(device_id));
    return GH_OK;
}

// Environment switches of an engine, read once at creation (include/graphem_hip.h lists them).
struct create_switches {
    bool no_presetup = false;   // GRAPHEM_HIP_NO_PRESETUP: keep the next iteration's KNN set-up out of the normalise launch
                                // (so that per-query flags survive a step for inspection)
    const char *reorder = nullptr;   // GRAPHEM_HIP_REORDER=1 | 2 overrides gh_params.reorder (tests / A-B runs: off, breadth-first)
    int tau_separate = -1;      // GRAPHEM_HIP_TAU_SEPARATE=1 | 0: thresholds in a launch of their own | in the fused one; -1: by size
    bool stamps = false;        // GRAPHEM_HIP_STAMPS: wall-clock stamps of the fused launch's workgroups
    int compact_gather = -1;    // GRAPHEM_HIP_COMPACT_GATHER=1 | 0: the fused kernel reads position rows from the sector-packed table |
                                // from the padded positions; -1: where the packed form was measured ahead
    int coarse_tau = -1;        // GRAPHEM_HIP_COARSE_TAU=1 | 0: the query-cell launch takes its thresholds from coarse group minima | a
                                // threshold launch of its own from the fine ones; -1: wherever the coarse form can serve
};
static create_switches read_switches() {
    create_switches sw;
    sw.no_presetup = getenv("GRAPHEM_HIP_NO_PRESETUP") != nullptr;
    sw.reorder = getenv("GRAPHEM_HIP_REORDER");
    if (const char *e = getenv("GRAPHEM_HIP_TAU_SEPARATE")) sw.tau_separate = atoi(e) != 0;
    sw.stamps = getenv("GRAPHEM_HIP_STAMPS") != nullptr;
    if (const char *e = getenv("GRAPHEM_HIP_COARSE_TAU")) sw.coarse_tau = atoi(e) != 0;
    if (const char *e = getenv("GRAPHEM_HIP_COMPACT_GATHER")) sw.compact_gather = atoi(e) != 0;
    return sw;
}

// Device buffers of the engine, in the order they have always been allocated, and the plan's arrays on them.
static gh_status allocate_and_upload(gh_engine *h, const gh_graph_plan &g, const create_switches &sw) {
    const int64_t n = h->n, E = h->E;
    const int D = h->D;
    const bool hashed = h->part.edge_rule == GH_EDGES_HASHED;
    const size_t nLD = (size_t)n * h->LD, S = (size_t)h->S;
    gh_status st;
#define GH_A(p, count, zero) GH_TRY_ST(gh_alloc(h, h->p, (count), (zero)))
    GH_A(d_edges, (size_t)E * 2, false);
    GH_A(d_rowptr, (size_t)h->rows + 1, false);
    GH_A(d_adj, (size_t)h->adj_len, false);
    GH_A(d_first_edge, (size_t)h->rows + 1, true);
    GH_A(d_mid, (size_t)h->own_count * h->LD, true);
    GH_A(d_Fs, (size_t)h->rows * h->LD, true);
    // candidate lists and the threshold subset exist only for the filtered scan (64 KiB per query)
    GH_A(d_gmin, (size_t)gh_gmin_floats(h), true);
    GH_A(d_sub_uv, (size_t)h->plan.thr_M1 * 2, false);
    // (a whole-graph engine's stats_fix launch stages the rows of the next set-up's queries: forces.hip)
    if (h->plan.stage_rows) GH_A(d_setup_rows, 2 * S * h->LD, true);
    if (hashed) GH_A(d_own_eids, g.own_eids.size() + 1, true);
    if (h->nlong) {
        GH_A(d_long_rows, g.long_rows.size(), false);
        GH_A(d_long_ownptr, g.long_ownptr.size(), false);
        GH_A(d_long_ownadj, g.long_ownadj.size() + 1, true);
        GH_A(d_long_eptr, g.long_eptr.size(), false);
        GH_A(d_long_erow, g.long_erow.size() + 1, false);
        GH_A(d_long_terms, (size_t)h->long_entries * D, false);
        GH_A(d_own_long, g.own_long.size(), false);
    }
    GH_A(d_vblock, g.vblock.size(), false);
    GH_A(d_pos, (size_t)h->pos_rows * h->LD, true);
    GH_TRY_ST(gh_ensure_compact_table(h));
    GH_A(d_new_buf, (size_t)h->rows * h->LD, true);
    h->d_new = h->d_new_buf.p;
    GH_A(d_tmpF, nLD, true);
    GH_A(d_tmpF2, nLD, true);
    GH_A(d_io, (size_t)n * D, false);
    GH_A(d_acc, nLD, true);
    GH_A(d_tflag, (size_t)n, true);
    GH_A(d_touched, 4 * S * (size_t)h->k, false);
    GH_A(d_tcount, 1, true);
    GH_A(d_sampled, S, true);
    GH_A(d_q, S * (size_t)(h->LD + 4), true);
    GH_A(d_qscan, S * (size_t)(h->LD + 4), true);
    GH_A(d_qA, S * 16, true);
    GH_A(d_qexact, S + 1, true);
    if ((st = gh_alloc(h, h->d_cand, h->plan.lists() ? S * GH_CAND_CAP : 1, false)) != GH_OK) {
        h->err = "hipMalloc of the KNN candidate lists failed: sample_size = " + std::to_string(h->S) + " needs " +
                 std::to_string((S * GH_CAND_CAP * sizeof(uint64_t)) >> 20) + " MiB (128 KiB per sampled midpoint)";
        return st;
    }
    GH_A(d_cnt, S * GH_CNT_STRIDE, true);
    GH_A(d_ovf, S, true);
    GH_A(d_sel_redo, S, true);
    GH_A(d_tq_count, S >= 2048 ? S : 1, true);
    GH_A(d_tq_base, S >= 2048 ? S : 1, true);
    GH_A(d_tq_touched, S >= 2048 ? 4 * S * (size_t)std::max(h->k, 1) : 1, false);
    GH_A(d_dbg_cnt, 2 * S, true);
    GH_A(d_partial, S * (size_t)(h->K + (h->cd_part ? 2 : 0)), true);
    GH_A(d_merged, S * (size_t)h->K, true);
    GH_A(d_iscratch, S * (size_t)h->k * h->LD, false);
    h->nblocks_update = (int)((h->rows + 255) / 256);
    GH_A(d_blockstats, (size_t)std::max(std::max(h->nblocks_update, h->n_vblocks), 1) * 2 * h->LD, true);
    GH_A(d_stats_buf, (size_t)gh_stats_rows(h->LD) * h->LD, true);
    h->d_stats = h->d_stats_buf.p;
    h->sample = gh_ids{GH_IDS_GIVEN, h->d_sampled.p};
    auto up = [&](void *dst, const void *src, size_t bytes) {
        return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    };
    auto up32 = [&](void *dst, const std::vector<int32_t> &v) { return up(dst, v.data(), sizeof(int32_t) * v.size()); };
    if (!up(h->d_edges.p, g.edges, sizeof(int32_t) * 2 * (size_t)E) || !up32(h->d_rowptr.p, g.rowptr) ||
        !up(h->d_adj.p, g.adj.data(), sizeof(int32_t) * (size_t)h->adj_len) || !up32(h->d_first_edge.p, g.first_edge) ||
        !up32(h->d_vblock.p, g.vblock) || (hashed && !up32(h->d_own_eids.p, g.own_eids)) ||
        (h->nlong && (!up32(h->d_long_rows.p, g.long_rows) || !up32(h->d_long_ownptr.p, g.long_ownptr) ||
                      !up32(h->d_long_eptr.p, g.long_eptr) || !up32(h->d_long_erow.p, g.long_erow) ||
                      !up32(h->d_long_ownadj.p, g.long_ownadj) || !up(h->d_own_long.p, g.own_long.data(), g.own_long.size()))) ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        h->err = "upload of the graph failed";
        return GH_ERR_HIP;
    }
    GH_TRY_ST(gh_grid_alloc(h));
    GH_TRY_ST(gh_ivf_alloc(h));
    GH_TRY_ST(gh_cdist_alloc(h));
    GH_A(d_tau_flag, 1, true);
    GH_A(d_wait_failed, 1, true);
    GH_A(d_qcell, GH_QC_WORDS, true);
    GH_A(d_qc_flag, 1, true);
    {   // the coarse table, every entry empty (also where AUTO does not take it: gh_set_scan_filter / gh_set_coarse_tau may)
        const size_t words = h->plan.coarse_ok ? 2 * (size_t)GH_CT_M * S : 1;
        GH_A(d_cmin, words, false);
        GH_HIP(hipMemsetAsync(h->d_cmin.p, 0xFF, sizeof(uint32_t) * words, h->stream));
    }
    if (sw.stamps) GH_A(d_stamps, ((size_t)std::max(h->n_vblocks, 1) + GH_STAMP_EXTRA) * 8, true);
#undef GH_A
    if (h->plan.thr_M1 > 0 && hipMemcpy(h->d_sub_uv.p, g.sub_uv.data(), sizeof(int32_t) * g.sub_uv.size(), hipMemcpyHostToDevice) != hipSuccess) {
        h->err = "upload of the threshold subset failed";
        return GH_ERR_HIP;
    }
    if (!h->order_host.empty()) {
        GH_TRY_ST(gh_alloc(h, h->d_order, (size_t)n, false));
        if (hipMemcpy(h->d_order.p, h->order_host.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
            h->err = "upload of the vertex order failed";
            return GH_ERR_HIP;
        }
    }
    return GH_OK;
}

// The sector-packed gather table exists where the plan asks for it (common.h gh_cg_slot), zeroed once: its pad dwords and
// the rows behind the n-th are never written.  A new table holds no positions yet.
gh_status gh_ensure_compact_table(gh_engine *h) {
    if (!h->plan.compact_gather || h->d_cg.p) return GH_OK;
    gh_step_compact_valid(h, false);
    return gh_alloc(h, h->d_cg, (size_t)gh_cg_bytes(h->n) / sizeof(float), true);
}

extern "C" gh_status gh_create(gh_handle *out, int device_id, int64_t n, int32_t D, int64_t E, const int32_t *edges,
                               const gh_params *params, const gh_partition *part) {
    if (!out) return GH_ERR_INVALID;
    *out = nullptr;
    GH_TRY_ST(gh_check_create_args(device_id, n, D, E, edges, params));
    auto fail = [&](gh_status st, const std::string &msg) { g_create_error = msg; return st; };
    std::unique_ptr<gh_engine> owner(new (std::nothrow) gh_engine());
    gh_engine *h = owner.get();
    if (!h) return fail(GH_ERR_NOMEM, "out of host memory");
    auto refuse = [&](const char *msg) { return fail(GH_ERR_INVALID, msg); };
    h->device = device_id;
    h->n = n; h->E = E; h->D = D; h->LD = gh_ld(D);
    h->prm = *params;
    h->k = params->n_neighbors; h->K = h->k + 1;
    h->S = std::min<int64_t>(params->sample_size, E);
    const bool auto_method = params->knn_method != GH_KNN_SCAN && params->knn_method != GH_KNN_GRID && params->knn_method != GH_KNN_IVF;
    if (params->knn_distance != GH_DIST_EXACT && params->knn_distance != GH_DIST_CDIST) return refuse("unknown knn_distance");
    h->cdist = params->knn_distance == GH_DIST_CDIST;
    h->cd_part = h->cdist && part != nullptr;
    if (h->cdist && !auto_method && params->knn_method != GH_KNN_SCAN)   // (an explicit request must not be dropped silently)
        return refuse("knn_distance = GH_DIST_CDIST re-values the candidates of GH_KNN_SCAN: it cannot be combined with GH_KNN_GRID / GH_KNN_IVF");
    h->Ksel = h->K + (h->cdist ? 1 : 0);
    if (part) h->part = *part;
    else h->part = gh_partition{0, n, 0, E, GH_EDGES_RANGE};
    if (h->part.edge_rule == GH_EDGES_HASHED) h->part.edge_lo = h->part.edge_hi = 0;  // not used by this rule
    if (h->part.row_lo < 0 || h->part.row_hi > n || h->part.row_lo > h->part.row_hi || h->part.edge_lo < 0 ||
        h->part.edge_hi > E || h->part.edge_lo > h->part.edge_hi ||
        (h->part.edge_rule != GH_EDGES_RANGE && h->part.edge_rule != GH_EDGES_HASHED))
        return refuse("partition out of range");
    h->rows = h->part.row_hi - h->part.row_lo;

    if (hipSetDevice(device_id) != hipSuccess) return fail(GH_ERR_HIP, "");
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return fail(GH_ERR_HIP, "hipStreamCreate failed");
    h->stream = h->own_stream;
    h->pos_rows = n + GH_POS_PAD_ROWS;
    const create_switches sw = read_switches();
    h->requests.no_presetup = sw.no_presetup;
    h->requests.tau_place = sw.tau_separate < 0 ? GH_TAU_BY_SIZE : sw.tau_separate ? GH_TAU_SEPARATE : GH_TAU_EMBEDDED;
    h->requests.coarse_mode = sw.coarse_tau < 0 ? GH_COARSE_AUTO : sw.coarse_tau ? GH_COARSE_ON : GH_COARSE_OFF;
    h->requests.compact_gather = sw.compact_gather < 0 ? GH_COMPACT_AUTO : sw.compact_gather ? GH_COMPACT_ON : GH_COMPACT_OFF;

    gh_graph_plan g;   // vertex order, ownership, pull lists, owned edges, fused blocks (graph_plan.hip)
    gh_plan_graph(h, edges, part != nullptr, sw.reorder ? atoi(sw.reorder) : params->reorder, &g);
    if (auto_method) gh_auto_knn_method(h);   // on the edges this engine searches: known only now
    gh_replan(h);                             // (step_plan.h) the method, own_count, fused_scan, Ksel and S are final here
    gh_plan_threshold_subset(h, &g);

    const gh_status st = allocate_and_upload(h, g, sw);
    if (st != GH_OK) return fail(st, h->err);
    *out = owner.release();
    return GH_OK;
}

gh_engine::~gh_engine() {
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

extern "C" void gh_destroy(gh_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    resolve_timers(h);
    delete h;
}

extern "C" const char *gh_last_error(gh_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// ---- positions ---------------------------------------------------------------------
extern "C" gh_status gh_set_positions(gh_handle h, const float *pos) {
    GH_TRY_ST(check_handle(h));
    if (h->f64) return pos ? gh_f64_set_positions_f32(h, pos) : GH_ERR_INVALID;
    if (!pos) { h->err = "positions is NULL"; return GH_ERR_INVALID; }
    gh_set_lookahead(h, nullptr);
    GH_HIP(hipMemcpyAsync(h->d_io.p, pos, sizeof(float) * (size_t)h->n * h->D, hipMemcpyHostToDevice, h->stream));
    float *cg = h->plan.compact_gather ? h->d_cg.p : nullptr;
    gh_step_compact_valid(h, false);
    GH_TRY_ST(gh_launch_pad(h, h->d_io.p, h->d_pos.p, cg));
    gh_step_compact_valid(h, cg != nullptr);
    GH_HIP(hipStreamSynchronize(h->stream));  // the host buffer may be released by the caller
    return GH_OK;
}

static gh_status download_padded(gh_engine *h, const float *d_src, float *host) {
    GH_TRY_ST(gh_launch_unpad(h, d_src, h->d_io.p));
    GH_HIP(hipMemcpyAsync(host, h->d_io.p, sizeof(float) * (size_t)h->n * h->D, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

static gh_plan_input plan_input_of(const gh_engine *h) {
    gh_plan_input in;
    in.n = h->n; in.rows = h->rows; in.E = h->E; in.own_count = h->own_count; in.S = h->S;
    in.D = h->D; in.LD = h->LD; in.k = h->k; in.K = h->K; in.Ksel = h->Ksel;
    in.knn_method = h->prm.knn_method;
    in.cdist = h->cdist; in.cd_part = h->cd_part;
    in.fused_scan = h->fused_scan; in.n_vblocks = h->n_vblocks;
    in.layout = h->xch.lay.form;
    return in;
}
void gh_replan(gh_engine *h) {
    const gh_tau_form was = h->plan.tau;
    h->plan = gh_make_step_plan(plan_input_of(h), h->requests);
    // a set-up done ahead for the other threshold placement would not have zeroed the producers' counter, one for the other
    // form of the group minima has left the wrong ones: done again
    if (h->plan.tau != was) gh_drop_lookahead(h);
}

// A workgroup of a fused launch gave up waiting for that launch's thresholds (tau_core.h) or query-cell table (fused.hip):
// whatever was computed since is not to be trusted.  Cannot happen while workgroups are started in index order; checked
// where the host synchronises.
static gh_status check_device_waits(gh_engine *h) {
    const bool cells = h->plan.prefilter == GH_PRE_CELLS;
    if (h->plan.search != GH_SEARCH_FUSED || !(h->plan.tau == GH_TAUF_EMBEDDED || cells) || !h->d_wait_failed.p) return GH_OK;
    int32_t failed = 0;
    GH_HIP(hipMemcpyAsync(&failed, h->d_wait_failed.p, sizeof(failed), hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    if (failed) {
        // reported once: the flag is cleared and the engine goes on without the form whose wait failed.  A failed table wait
        // leaves the split-f16 filter, with the thresholds wherever the creation-time placement puts them (inside the fused
        // launch on small graphs: its first workgroups are waited for).  A failed threshold wait leaves a threshold launch
        // of its own, and with the filter on AUTO that brings the query-cell table with it -- whose workgroups wait for the
        // launch's first one -- exactly the state GRAPHEM_HIP_TAU_SEPARATE=1 creates (NOTES.md "Recovery after a failed wait").
        // Either way whatever was set up ahead is dropped: the caller has to set the positions again.
        GH_HIP(hipMemsetAsync(h->d_wait_failed.p, 0, sizeof(int32_t), h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (cells) h->requests.scan_filter = GH_FILTER_MFMA;
        else h->requests.tau_place = GH_TAU_SEPARATE;
        gh_replan(h);
        gh_drop_lookahead(h);
        gh_step_compact_valid(h, false);
        if (cells) {
            h->err = "a workgroup of the fused spring+scan launch timed out waiting for the query-cell table of its own "
                     "launch; results since the last successful gh_sync / gh_get_positions are invalid -- set the positions "
                     "again.  The engine now uses the split-f16 pre-filter (GH_FILTER_MFMA); please report this";
            return GH_ERR_RUNTIME;
        }
        h->err = "a workgroup of the fused spring+scan launch timed out waiting for the thresholds of its own launch; "
                 "results since the last successful gh_sync / gh_get_positions are invalid -- set the positions again. "
                 "The engine now computes the thresholds in a launch of their own (as GRAPHEM_HIP_TAU_SEPARATE=1 does); "
                 "please report this";
        return GH_ERR_RUNTIME;
    }
    return GH_OK;
}

extern "C" gh_status gh_get_positions(gh_handle h, float *pos) {
    GH_TRY_ST(check_handle(h));
    if (h->f64) return pos ? gh_f64_get_positions_f32(h, pos) : GH_ERR_INVALID;
    if (!pos) { h->err = "positions is NULL"; return GH_ERR_INVALID; }
    GH_TRY_ST(check_device_waits(h));
    return download_padded(h, h->d_pos.p, pos);
}

extern "C" float *gh_positions_device(gh_handle h) {
    if (!h || h->f64) return nullptr;
    gh_step_pos_shared(h);   // the caller may write the rows whenever it likes: the sector-packed copy is not read again
    return h->d_pos.p;
}
extern "C" gh_status gh_vertex_order(gh_handle h, int32_t *order) {
    GH_TRY_ST(check_handle(h));
    if (!order) { h->err = "order is NULL"; return GH_ERR_INVALID; }
    for (int64_t i = 0; i < h->n; ++i) order[i] = h->order_host.empty() ? (int32_t)i : h->order_host[(size_t)i];
    return GH_OK;
}
extern "C" const float *gh_positions_unpadded_device(gh_handle h) {
    if (!h || h->f64 || hipSetDevice(h->device) != hipSuccess) return nullptr;
    if (gh_launch_unpad(h, h->d_pos.p, h->d_io.p) != GH_OK) return nullptr;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return nullptr;
    return h->d_io.p;
}
extern "C" int32_t gh_row_stride(gh_handle h) { return h ? h->LD : 0; }

// ---- the loop ----------------------------------------------------------------------
static bool whole_graph(gh_engine *h) {
    return h->part.row_lo == 0 && h->part.row_hi == h->n &&
           (h->part.edge_rule == GH_EDGES_HASHED || (h->part.edge_lo == 0 && h->part.edge_hi == h->E));
}
// gh_step / gh_run / the per-phase entry points merge with world = 1 and normalise with the own rows'
// statistics: on a row partition that would silently corrupt the positions.
static gh_status check_whole(gh_engine *h, const char *what) {
    if (whole_graph(h) && h->xch.is(GH_LAYOUT_NONE)) return GH_OK;
    h->err = std::string(what) + " needs the whole graph on one rank; a partitioned engine runs gh_step_begin / "
             "gh_step_merge / gh_step_finish_gathered (or gh_run_partitioned)";
    return GH_ERR_INVALID;
}
static gh_status check_k(gh_engine *h) {
    if ((int64_t)h->K > h->E) {
        h->err = "selected index k out of range";  // torch.topk's message (pt.py:583)
        return GH_ERR_K_TOO_LARGE;
    }
    return GH_OK;
}

// The source of an iteration's ids given the caller's (validated, uploaded to d_sampled), or the engine's own when
// there are none or S >= E (the reference uses arange, pt.py:412).
static gh_status caller_ids(gh_engine *h, const int32_t *host_ids, gh_ids *src) {
    *src = gh_own_ids(h);
    if (!host_ids || src->mode == GH_IDS_ARANGE) return GH_OK;
    for (int64_t i = 0; i < h->S; ++i)
        if (host_ids[i] < 0 || host_ids[i] >= h->E) { h->err = "sampled edge id out of range"; return GH_ERR_INVALID; }
    // a set-up done ahead (inside the last normalise launch) left ITS ids in d_sampled and built the query
    // records from them: overwriting the ids makes it stale
    gh_set_lookahead(h, nullptr);
    GH_HIP(hipMemcpyAsync(h->d_sampled.p, host_ids, sizeof(int32_t) * (size_t)h->S, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *src = gh_ids{GH_IDS_GIVEN, h->d_sampled.p};
    return GH_OK;
}

// Spring forces of the own rows -> d_Fs and this rank's K best keys per query -> d_partial.
// fuse_intersect: single-rank step, the KNN kernels also run the intersection phase.
static gh_status step_begin_launches(gh_engine *h, bool fuse_intersect);
static gh_status step_begin(gh_engine *h, bool fuse_intersect) {
    gh_step_reset(h);
    GH_TRY_ST(step_begin_launches(h, fuse_intersect));
    // form D: new0 = pos + Fs of the own rows is in their block -- written by the fused kernel, or (a rank too small for it;
    // every rank must send at the same point of the iteration) by a launch of its own -- and may travel now
    if (h->xch.is(GH_LAYOUT_OVERLAP)) {
        if (!h->step.new0_ready) GH_TRY_ST(gh_launch_new0(h));
        gh_step_set_rows_early(h, true);
    }
    return GH_OK;
}
static gh_status step_begin_launches(gh_engine *h, bool fuse_intersect) {
    switch (h->plan.search) {
    case GH_SEARCH_NONE:   // nothing sampled / no neighbours asked for: spring forces only
        h->sample.mode = GH_IDS_GIVEN;
        gh_step_intersect_done(h);
        GH_HIP(hipMemsetAsync(h->d_tcount.p, 0, sizeof(int32_t), h->stream));
        return gh_launch_spring_mid(h);
    case GH_SEARCH_GRID:   // sub-quadratic search: thresholds, own midpoints to memory, grid build + cell search
        GH_TRY_ST(gh_knn_prepare(h));          // query records only: the thresholds come from the grid itself
        GH_TRY_ST(gh_launch_spring_mid(h));
        GH_TRY_ST(gh_grid_search(h));
        return gh_knn_finish(h, true, fuse_intersect);
    case GH_SEARCH_IVF:    // inverted-file search (approximate: probed lists only; ivf.hip)
        GH_TRY_ST(gh_knn_prepare(h));          // query records only
        GH_TRY_ST(gh_launch_spring_mid(h));
        GH_TRY_ST(gh_ivf_search(h));
        return gh_knn_finish(h, true, fuse_intersect);
    case GH_SEARCH_FUSED:
        GH_TRY_ST(gh_knn_prepare(h));
        // (else: the first workgroups of the fused launch, tau_core.h, or the first one of its query-cell form, qcell_core.h)
        if (h->plan.tau == GH_TAUF_LAUNCH) GH_TRY_ST(gh_knn_thresholds(h));
        GH_TRY_ST(gh_launch_spring_scan(h));
        return gh_knn_finish(h, false, fuse_intersect);
    case GH_SEARCH_SCAN:
    case GH_SEARCH_BLOCK:
        break;
    }
    GH_TRY_ST(gh_launch_spring_mid(h));
    return gh_knn_local(h, fuse_intersect);
}

// next: the ids the finish will set the next iteration up from (presetup_ids), when the caller knows them by now.
gh_status gh_step_merge_keys(gh_engine *h, const uint64_t *gathered, int world, const gh_ids *next) {
    GH_TRY_ST(gh_knn_merge(h, gathered, world, !h->step.intersect_done));
    if (!h->step.intersect_done) GH_TRY_ST(gh_launch_intersect(h));
    GH_TRY_ST(gh_launch_integrate(h, next));
    return GH_OK;
}

// next: the source of the next iteration's ids, or null.  The normalise launch of a single-rank step on the fused path
// then also runs that iteration's KNN set-up (gh_launch_normalise); gh_knn_prepare falls back to its own kernel when the
// next step turns out different.  presetup_ids: `next` where that applies, else null.
static const gh_ids *presetup_ids(const gh_engine *h, const gh_ids *next) {
    return h->plan.presetup ? next : nullptr;
}
// The finish of every step.  The next iteration's set-up rides in the normalise launch where the plan allows: from `next`
// after a single-rank finish; after an all-rows finish, from the engine's own draw when this step drew its own ids (a rank
// that drew this step's ids on the device will do so again); never under form C.
gh_status gh_step_finish_as(gh_engine *h, gh_finish_kind kind, const gh_ids *next, const double *stats_all) {
    const gh_ids own = gh_own_ids(h);
    bool with_cleanup = true;   // the normalise launch also zeroes what the intersection phase touched
    if (kind == GH_FINISH_OWN) next = presetup_ids(h, next);
    else next = kind == GH_FINISH_ALL_ROWS && h->step.own_ids && h->plan.presetup_gathered ? &own : nullptr;
    if (kind == GH_FINISH_ALL_ROWS && h->xch.is(GH_LAYOUT_OVERLAP)) {
        GH_TRY_ST(gh_launch_patch_rows(h));
        with_cleanup = !h->step.rows_early;   // (the patch launch has zeroed the accumulators of a step whose rows went early)
    }
    GH_TRY_ST(gh_launch_normalise(h, kind, with_cleanup, next, stats_all));
    gh_step_set_rows_early(h, false);
    h->iter += 1;
    return GH_OK;
}

// The iteration driver of gh_step, gh_run and gh_run_torch_sampled: iteration t takes its ids from src_of_row(t), after
// before_row(t).  Its normalise launch sets up the next iteration: row t + 1; after the last row, the engine's own draw
// when the run draws its own ids (a caller that gave ids will give them again), else nothing.
template <class Src, class Before>
static gh_status run_iterations(gh_engine *h, int32_t iters, bool draws_own, Src src_of_row, Before before_row) {
    const gh_ids own = gh_own_ids(h);
    auto loop = [&]() -> gh_status {
        for (int32_t t = 0; t < iters; ++t) {
            GH_TRY_ST(before_row(t));
            h->sample = src_of_row(t);
            GH_TRY_ST(step_begin(h, true));
            // (named before the statistics launch, which stages the rows of that set-up: before_row(t) has made row t + 1 available)
            const gh_ids next = t + 1 < iters ? src_of_row(t + 1) : own;
            const gh_ids *next_ids = t + 1 < iters || draws_own ? &next : nullptr;
            GH_TRY_ST(gh_step_merge_keys(h, h->d_partial.p, 1, presetup_ids(h, next_ids)));
            GH_TRY_ST(gh_step_finish_as(h, GH_FINISH_OWN, next_ids));
        }
        return GH_OK;
    };
    const gh_status st = loop();
    h->sample = gh_ids{GH_IDS_GIVEN, h->d_sampled.p};  // (not a row of d_stream_ids, which a later run may replace)
    return st;
}
static gh_status nothing_before(int32_t) { return GH_OK; }

extern "C" gh_status gh_step(gh_handle h, const int32_t *sampled) {
    GH_TRY_ST(check_handle(h));
    if (h->f64) return gh_f64_step(h, sampled);
    GH_TRY_ST(check_whole(h, "gh_step"));
    GH_TRY_ST(check_k(h));
    gh_ids src;
    GH_TRY_ST(caller_ids(h, sampled, &src));
    return run_iterations(h, 1, sampled == nullptr, [&](int32_t) { return src; }, nothing_before);
}

// d_stream_ids with room for `words` ids (a smaller buffer is released once the stream has drained).
static gh_status ensure_stream_ids(gh_engine *h, size_t words) {
    if (words <= h->stream_ids_cap) return GH_OK;
    if (h->d_stream_ids.p) { GH_HIP(hipStreamSynchronize(h->stream)); h->d_stream_ids.reset(); h->stream_ids_cap = 0; }
    GH_TRY_ST(gh_alloc(h, h->d_stream_ids, words, false));
    h->stream_ids_cap = words;
    return GH_OK;
}

// Uploads an (iters, S) host id stream for a run (validated); *d_ids = nullptr when the run draws its own ids
// (no stream given, or S >= E where the reference uses arange, pt.py:412).
gh_status gh_upload_sample_stream(gh_engine *h, int32_t iters, const int32_t *sample_stream, int32_t **d_ids) {
    *d_ids = nullptr;
    if (!sample_stream || h->S >= h->E || iters <= 0) return GH_OK;
    const size_t cnt = (size_t)iters * (size_t)h->S;
    for (size_t i = 0; i < cnt; ++i)
        if (sample_stream[i] < 0 || sample_stream[i] >= h->E) { h->err = "sampled edge id out of range"; return GH_ERR_INVALID; }
    GH_TRY_ST(ensure_stream_ids(h, cnt));
    GH_HIP(hipMemcpyAsync(h->d_stream_ids.p, sample_stream, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    *d_ids = h->d_stream_ids.p;
    return GH_OK;
}

extern "C" gh_status gh_run(gh_handle h, int32_t iters, const int32_t *sample_stream) {
    GH_TRY_ST(check_handle(h));
    if (h->f64) return iters < 0 ? GH_ERR_INVALID : gh_f64_run(h, iters, sample_stream);
    if (iters < 0) { h->err = "negative iteration count"; return GH_ERR_INVALID; }
    if (iters == 0) return GH_OK;
    GH_TRY_ST(check_whole(h, "gh_run"));
    GH_TRY_ST(check_k(h));
    int32_t *d_ids = nullptr;
    GH_TRY_ST(gh_upload_sample_stream(h, iters, sample_stream, &d_ids));
    const gh_ids own = gh_own_ids(h);
    auto src = [&](int32_t t) { return d_ids ? gh_ids{GH_IDS_GIVEN, d_ids + (size_t)t * h->S} : own; };
    return run_iterations(h, iters, d_ids == nullptr, src, nothing_before);
}

extern "C" gh_status gh_set_cdist_replay(gh_handle h, int32_t all_ties) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_set_cdist_replay"));
    if (!h->cdist) { h->err = "gh_set_cdist_replay: not a GH_DIST_CDIST engine"; return GH_ERR_INVALID; }
    h->cd_all_ties = all_ties != 0;
    return GH_OK;
}

extern "C" gh_status gh_set_scan_filter(gh_handle h, int32_t mode) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_set_scan_filter"));
    if (mode != GH_FILTER_AUTO && mode != GH_FILTER_MFMA && mode != GH_FILTER_CELLS) {
        h->err = "gh_set_scan_filter: mode must be GH_FILTER_AUTO, GH_FILTER_MFMA or GH_FILTER_CELLS";
        return GH_ERR_INVALID;
    }
    if (mode == GH_FILTER_CELLS && !h->plan.cells_ok) {
        h->err = "gh_set_scan_filter: the query-cell filter needs a fused engine with n_components <= 3 and 1 <= sample_size <= " +
                 std::to_string(GH_QC_SMAX);
        return GH_ERR_INVALID;
    }
    h->requests.scan_filter = mode;
    gh_replan(h);
    return GH_OK;
}

extern "C" gh_status gh_set_coarse_tau(gh_handle h, int32_t mode) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_set_coarse_tau"));
    if (mode != GH_COARSE_AUTO && mode != GH_COARSE_OFF && mode != GH_COARSE_ON) {
        h->err = "gh_set_coarse_tau: mode must be GH_COARSE_AUTO, GH_COARSE_OFF or GH_COARSE_ON";
        return GH_ERR_INVALID;
    }
    h->requests.coarse_mode = mode;
    gh_replan(h);
    return GH_OK;
}
extern "C" gh_status gh_set_compact_gather(gh_handle h, int32_t mode) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_set_compact_gather"));
    if (mode != GH_COMPACT_AUTO && mode != GH_COMPACT_OFF && mode != GH_COMPACT_ON) {
        h->err = "gh_set_compact_gather: mode must be GH_COMPACT_AUTO, GH_COMPACT_OFF or GH_COMPACT_ON";
        return GH_ERR_INVALID;
    }
    h->requests.compact_gather = mode;
    gh_replan(h);
    // a table that was out of use did not follow the positions: the next finish (or gh_set_positions) fills it
    gh_step_compact_valid(h, false);
    return gh_ensure_compact_table(h);
}
extern "C" gh_status gh_get_compact_gather(gh_handle h, int32_t *in_use) {
    GH_TRY_ST(check_handle(h));
    if (!in_use) { h->err = "in_use is NULL"; return GH_ERR_INVALID; }
    *in_use = !h->f64 && h->plan.compact_gather && !h->step.pos_shared ? 1 : 0;
    return GH_OK;
}
extern "C" gh_status gh_compact_gather_launches(gh_handle h, int64_t *packed) {
    GH_TRY_ST(check_handle(h));
    if (!packed) { h->err = "packed is NULL"; return GH_ERR_INVALID; }
    *packed = h->f64 ? 0 : h->compact_launches;
    return GH_OK;
}
extern "C" gh_status gh_compact_slots(int64_t v0, int64_t count, int64_t *out) {
    if (!out || v0 < 0 || count < 0 || v0 + count > 0x100000000ll) return GH_ERR_INVALID;
    for (int64_t i = 0; i < count; ++i) out[i] = (int64_t)gh_cg_slot((uint32_t)(v0 + i));
    return GH_OK;
}
extern "C" int64_t gh_compact_slot(int64_t v) { return v < 0 || v > 0xFFFFFFFFll ? -1 : (int64_t)gh_cg_slot((uint32_t)v); }
extern "C" int64_t gh_compact_bytes(int64_t n) { return n < 0 ? -1 : gh_cg_bytes(n); }
extern "C" gh_status gh_get_coarse_tau(gh_handle h, int32_t *in_use) {
    GH_TRY_ST(check_handle(h));
    if (!in_use) { h->err = "in_use is NULL"; return GH_ERR_INVALID; }
    *in_use = !h->f64 && h->plan.tau == GH_TAUF_COARSE ? 1 : 0;
    return GH_OK;
}
extern "C" gh_status gh_debug_coarse_table(gh_handle h, uint32_t *out, int64_t count) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_debug_coarse_table"));
    if (!out || count != 2 * (int64_t)GH_CT_M * h->S || !h->plan.coarse_ok) {
        h->err = "gh_debug_coarse_table: needs an engine the coarse thresholds can serve and room for 2 * 64 * sample_size words";
        return GH_ERR_INVALID;
    }
    GH_HIP(hipMemcpyAsync(out, h->d_cmin.p, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_get_scan_filter(gh_handle h, int32_t *mode) {
    GH_TRY_ST(check_handle(h));
    if (!mode) { h->err = "mode is NULL"; return GH_ERR_INVALID; }
    const gh_prefilter f = h->f64 ? GH_PRE_NONE : h->plan.prefilter;
    *mode = f == GH_PRE_CELLS ? GH_FILTER_CELLS : f == GH_PRE_SPLIT_F16 ? GH_FILTER_MFMA : GH_FILTER_AUTO;
    return GH_OK;
}

extern "C" gh_status gh_qcell_probe(const float *bounds, int32_t D, const float *q, const float *tau, const float *m, int64_t n,
                                    float *d2, int32_t *cells) {
    if (!bounds || !q || !tau || !m || !d2 || !cells || D < 1 || D > 3 || n < 0) return GH_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        float acc = 0.0f;
        for (int d = 0; d < D; ++d) {
            const float df = q[i * D + d] - m[i * D + d];   // park's chain (fused.hip)
            acc = fmaf(df, df, acc);
            const float *b = bounds + d * (GH_QC_G - 1);
            int lo, hi;
            gh_qc_axis_box(b, q[i * D + d], tau[i], lo, hi);
            cells[(i * D + d) * 3] = gh_qc_axis_cell(b, m[i * D + d]);
            cells[(i * D + d) * 3 + 1] = lo;
            cells[(i * D + d) * 3 + 2] = hi;
        }
        d2[i] = acc;
    }
    return GH_OK;
}

// ---- the reference's own sampler, drawn beside the loop (pt.py:403-413) ---------------------------------------------
extern "C" gh_status gh_torch_randperm_prefix(uint8_t *rng_state, int64_t state_bytes, int64_t n, int64_t S, int32_t iters,
                                              int32_t *ids) {
    if (!rng_state || state_bytes != GH_TORCH_RNG_STATE_BYTES || n < 0 || n >= ((int64_t)1 << 31) || S < 0 || S > n || iters < 0 ||
        (!ids && iters > 0 && S > 0))
        return GH_ERR_INVALID;
    gh_mt19937 mt;
    if (!gh_mt_load(&mt, rng_state)) return GH_ERR_INVALID;
    std::vector<int64_t> scratch((size_t)gh_rp_scratch_words(S));
    for (int32_t t = 0; t < iters; ++t) gh_torch_randperm_prefix_one(&mt, n, S, ids + (size_t)t * (size_t)S, scratch.data());
    gh_mt_store(&mt, rng_state);
    return GH_OK;
}
extern "C" const char *gh_torch_randperm_isa(void) { return gh_mt_isa(); }

// iters iterations whose sample ids are torch.randperm(E)[:S] of the generator state handed in -- what run_layout of the
// reference's CPU backend consumes (one randperm per iteration, pt.py:409) -- drawn by a host thread into a circular host
// buffer while this thread enqueues: before iteration t goes out, the rows drawn so far (at least row t + 1, whose query
// records the normalise launch of iteration t sets up; at most GH_RING_CHUNK at a time) are copied to a pinned slot and
// from there, in one copy on the engine's stream, into a device ring of GH_DEV_RING rows.  The GPU starts after ONE draw;
// when the producer is ahead the uploads are whole slots, when it is the bottleneck they are single rows.  The only host
// synchronisation with the stream is for a pinned slot to come back (GH_RING_SLOTS uploads later).
#define GH_DEV_RING 128    /* rows of the device ring: a row is overwritten GH_DEV_RING - GH_RING_CHUNK - 1 iterations after its own at the earliest */
#define GH_HOST_RING 256   /* rows the producer may be ahead of the uploads */
extern "C" gh_status gh_run_torch_sampled(gh_handle h, int32_t iters, uint8_t *rng_state, int64_t state_bytes) {
    GH_TRY_ST(check_handle(h));
    if (iters < 0) { h->err = "negative iteration count"; return GH_ERR_INVALID; }
    if (!rng_state || state_bytes != GH_TORCH_RNG_STATE_BYTES) { h->err = "rng_state must be the 5056 bytes of torch.get_rng_state()"; return GH_ERR_INVALID; }
    if (iters == 0) return GH_OK;
    if (h->S >= h->E) return gh_run(h, iters, nullptr);   // arange(E): no randomness consumed (pt.py:412)
    gh_mt19937 mt;
    if (!gh_mt_load(&mt, rng_state)) { h->err = "rng_state is not a torch CPU generator state (mt19937, legacy layout)"; return GH_ERR_INVALID; }
    const size_t S = (size_t)h->S;
    if (h->f64) {   // (the float64 engine takes host ids step by step: drawn up front)
        std::vector<int32_t> ids((size_t)iters * S);
        std::vector<int64_t> scratch((size_t)gh_rp_scratch_words(h->S));
        for (int32_t t = 0; t < iters; ++t) gh_torch_randperm_prefix_one(&mt, h->E, h->S, ids.data() + (size_t)t * S, scratch.data());
        GH_TRY_ST(gh_f64_run(h, iters, ids.data()));
        gh_mt_store(&mt, rng_state);
        return GH_OK;
    }
    GH_TRY_ST(check_whole(h, "gh_run_torch_sampled"));
    GH_TRY_ST(check_k(h));
    const size_t ring_words = (size_t)GH_RING_SLOTS * GH_RING_CHUNK * S;
    if (h->ring.cap < ring_words) {
        GH_HIP(hipStreamSynchronize(h->stream));
        if (h->ring.host) { (void)hipHostFree(h->ring.host); h->ring.host = nullptr; h->ring.cap = 0; }
        GH_HIP(hipHostMalloc(reinterpret_cast<void **>(&h->ring.host), ring_words * sizeof(int32_t), hipHostMallocDefault));
        h->ring.cap = ring_words;
        h->ring.uploads = 0;   // (no copy out of the old slots is pending: the stream has drained)
        for (hipEvent_t &e : h->ring.ev)
            if (!e) GH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    GH_TRY_ST(ensure_stream_ids(h, (size_t)GH_DEV_RING * S));

    std::vector<int32_t> hbuf((size_t)GH_HOST_RING * S);
    std::mutex mu;
    std::condition_variable cv;
    int32_t drawn = 0;      // rows in hbuf (producer -> this thread)
    int32_t taken = 0;      // rows copied out of hbuf (this thread -> producer)
    bool stop = false;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    const clk::time_point t_begin = clk::now();
    double draw_ms = 0.0, slot_wait_ms = 0.0, main_wait_ms = 0.0;
    std::thread producer([&]() {
        std::vector<int64_t> scratch((size_t)gh_rp_scratch_words(h->S));
        for (int32_t t = 0; t < iters; ++t) {
            if (t >= GH_HOST_RING) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || taken > t - GH_HOST_RING; });
                if (stop) return;
            }
            const clk::time_point t0 = clk::now();
            gh_torch_randperm_prefix_one(&mt, h->E, h->S, hbuf.data() + (size_t)(t % GH_HOST_RING) * S, scratch.data());
            draw_ms += ms_since(t0);
            {
                std::lock_guard<std::mutex> lk(mu);
                drawn = t + 1;
                if (stop) return;
            }
            cv.notify_all();
        }
    });
    int32_t uploaded = 0;
    // rows [uploaded, uploaded + m) -> device ring; m >= 1 once row `need` is drawn
    auto upload_through = [&](int32_t need) -> gh_status {
        while (uploaded <= need) {
            int32_t have;
            {
                const clk::time_point t0 = clk::now();
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return drawn > uploaded; });
                have = drawn;
                main_wait_ms += ms_since(t0);
            }
            int32_t m = std::min<int32_t>(have - uploaded, GH_RING_CHUNK);
            m = std::min<int32_t>(m, GH_DEV_RING - uploaded % GH_DEV_RING);     // neither ring wraps inside one copy
            m = std::min<int32_t>(m, GH_HOST_RING - uploaded % GH_HOST_RING);
            // a slot is reused once its last copy has run -- also one enqueued by an earlier call, which returns undrained
            const int slot = (int)(h->ring.uploads % GH_RING_SLOTS);
            if (h->ring.uploads >= GH_RING_SLOTS) {
                const clk::time_point t0 = clk::now();
                GH_HIP(hipEventSynchronize(h->ring.ev[slot]));
                slot_wait_ms += ms_since(t0);
            }
            int32_t *pin = h->ring.host + (size_t)slot * GH_RING_CHUNK * S;
            memcpy(pin, hbuf.data() + (size_t)(uploaded % GH_HOST_RING) * S, sizeof(int32_t) * (size_t)m * S);
            GH_HIP(hipMemcpyAsync(h->d_stream_ids.p + (size_t)(uploaded % GH_DEV_RING) * S, pin, sizeof(int32_t) * (size_t)m * S, hipMemcpyHostToDevice, h->stream));
            GH_HIP(hipEventRecord(h->ring.ev[slot], h->stream));
            uploaded += m;
            ++h->ring.uploads;
            {
                std::lock_guard<std::mutex> lk(mu);
                taken = uploaded;
            }
            cv.notify_all();
        }
        return GH_OK;
    };
    auto row = [&](int32_t t) { return gh_ids{GH_IDS_GIVEN, h->d_stream_ids.p + (size_t)(t % GH_DEV_RING) * S}; };
    // this iteration's ids, and the next one's for its normalise launch
    auto upload = [&](int32_t t) { return upload_through(std::min(t + 1, iters - 1)); };
    const gh_status st = run_iterations(h, iters, false, row, upload);
    {
        std::lock_guard<std::mutex> lk(mu);
        stop = st != GH_OK;
    }
    cv.notify_all();
    producer.join();
    h->sampler_stats[0] = draw_ms; h->sampler_stats[1] = slot_wait_ms; h->sampler_stats[2] = main_wait_ms; h->sampler_stats[3] = ms_since(t_begin);
    if (st != GH_OK) return st;
    gh_mt_store(&mt, rng_state);
    return GH_OK;
}

extern "C" gh_status gh_sampler_stats(gh_handle h, double *out4) {
    GH_TRY_ST(check_handle(h));
    if (!out4) { h->err = "out4 is NULL"; return GH_ERR_INVALID; }
    for (int i = 0; i < 4; ++i) out4[i] = h->sampler_stats[i];
    return GH_OK;
}

extern "C" gh_status gh_sync(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    GH_HIP(hipStreamSynchronize(h->stream));
    resolve_timers(h);
    return check_device_waits(h);
}

// ---- multi-GPU split step ----------------------------------------------------------
extern "C" gh_status gh_step_begin(gh_handle h, const int32_t *sampled) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_step_begin"));
    GH_TRY_ST(check_k(h));
    gh_step_own_ids(h, sampled == nullptr);
    GH_TRY_ST(caller_ids(h, sampled, &h->sample));
    return step_begin(h, false);
}
// Part 1 of a split step with the ids already on the device (a row of an uploaded stream), or nullptr: the
// engine draws them itself, identically on every rank (comm.hip gh_run_partitioned).
gh_status gh_step_begin_device_ids(gh_engine *h, int32_t *dev_ids) {
    GH_TRY_ST(check_k(h));
    gh_step_own_ids(h, dev_ids == nullptr);
    h->sample = dev_ids ? gh_ids{GH_IDS_GIVEN, dev_ids} : gh_own_ids(h);   // (gh_upload_sample_stream gives none when S >= E)
    return step_begin(h, false);
}
extern "C" gh_status gh_set_stream(gh_handle h, void *hip_stream, int32_t use_own) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_set_stream"));
    GH_HIP(hipStreamSynchronize(h->stream));
    resolve_timers(h);
    h->stream = use_own ? h->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
    return GH_OK;
}
extern "C" int64_t gh_positions_rows_allocated(gh_handle h) { return h ? h->pos_rows : 0; }
extern "C" uint64_t *gh_knn_partial_device(gh_handle h) { return h ? h->d_partial.p : nullptr; }
extern "C" const uint64_t *gh_knn_merged_device(gh_handle h) { return h ? h->d_keys_cur : nullptr; }
extern "C" int32_t gh_knn_partial_cols(gh_handle h) { return h ? h->K + (h->cd_part ? 2 : 0) : 0; }
extern "C" gh_status gh_step_merge(gh_handle h, const uint64_t *gathered, int32_t world) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_step_merge"));
    if (!gathered || world < 1) { h->err = "bad gathered buffer / world size"; return GH_ERR_INVALID; }
    return gh_step_merge_keys(h, gathered, world);
}
extern "C" double *gh_stats_partial_device(gh_handle h) { return h ? h->d_stats : nullptr; }
extern "C" int32_t gh_stats_rows(gh_handle h) { return h ? gh_stats_rows(h->LD) : 0; }
extern "C" gh_status gh_step_finish(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_step_finish"));
    return gh_step_finish_as(h, GH_FINISH_OWN);
}

// The one layout setter (name: the call, for the messages): the value from exchange_layout.h, the buffers it sizes, and the
// views d_new / d_stats moved to the engine's own block (forms B and D).
static gh_status set_layout(gh_engine *h, const char *name, int form, int32_t world, int32_t rank, int64_t chunk) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, name));
    gh_exchange &x = h->xch;
    gh_exchange_layout l;
    GH_TRY_ST(gh_make_exchange_layout({h->n, h->pos_rows, h->D, h->LD, h->S, h->k, h->part.row_lo, h->part.row_hi}, x.lay.form, form,
                                      world, rank, chunk, &l, &h->err));
    const bool views_move = form != GH_LAYOUT_RANK;
    if (views_move) GH_HIP(hipStreamSynchronize(h->stream));
    if (l.rows_floats) GH_TRY_ST(gh_alloc(h, x.d_rows, (size_t)l.rows_floats, true));
    if (l.late_all_doubles) GH_TRY_ST(gh_alloc(h, x.d_late, (size_t)l.late_all_doubles, true));
    if (l.packed_floats) GH_TRY_ST(gh_alloc(h, x.d_packed, (size_t)l.packed_floats, true));
    if (form == GH_LAYOUT_OVERLAP) GH_HIP(hipStreamSynchronize(h->stream));   // (a side stream will read them)
    x.lay = l;
    x.packed_exchange = l.packed_default;
    if (views_move) {
        h->d_new = x.d_rows.p + l.own_rows;
        h->d_stats = x.stats_buffer() + l.own_stats;
    }
    gh_replan(h);
    return GH_OK;
}
extern "C" gh_status gh_gather_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk) { return set_layout(h, "gh_gather_layout", GH_LAYOUT_GATHERED, world, rank, chunk); }
extern "C" gh_status gh_rank_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk) { return set_layout(h, "gh_rank_layout", GH_LAYOUT_RANK, world, rank, chunk); }
// Form D: form B's finish (every rank normalises all n rows from the gathered un-normalised rows) with the big collective
// moved to the front of the KNN tail -- see include/graphem_hip.h.
extern "C" gh_status gh_overlap_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk) { return set_layout(h, "gh_overlap_layout", GH_LAYOUT_OVERLAP, world, rank, chunk); }
extern "C" float *gh_rows_all_device(gh_handle h) { return h && h->xch.is(GH_LAYOUT_OVERLAP) ? h->xch.travelling_rows() : nullptr; }
extern "C" int32_t gh_rows_all_row_floats(gh_handle h) { return h && h->xch.is(GH_LAYOUT_OVERLAP) ? h->xch.lay.row_floats : 0; }
extern "C" double *gh_stats_all_device(gh_handle h) { return h && h->xch.is(GH_LAYOUT_OVERLAP) ? h->xch.d_late.p : nullptr; }
extern "C" int64_t gh_stats_all_block_doubles(gh_handle h) { return h && h->xch.is(GH_LAYOUT_OVERLAP) ? h->xch.lay.late_doubles : 0; }
extern "C" int32_t gh_step_rows_early(gh_handle h) { return h && h->xch.is(GH_LAYOUT_OVERLAP) && h->step.rows_early ? 1 : 0; }
extern "C" gh_status gh_step_pack_rows(gh_handle h, void *hip_stream, int32_t use_engine_stream) {
    GH_TRY_ST(check_handle(h));
    if (!h->xch.is(GH_LAYOUT_OVERLAP)) { h->err = "gh_overlap_layout has not been called"; return GH_ERR_INVALID; }
    return gh_launch_pack_rows(h, use_engine_stream ? h->stream : reinterpret_cast<hipStream_t>(hip_stream));
}
extern "C" gh_status gh_step_finish_overlap(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    if (!h->xch.is(GH_LAYOUT_OVERLAP)) { h->err = "gh_overlap_layout has not been called"; return GH_ERR_INVALID; }
    return gh_step_finish_as(h, GH_FINISH_ALL_ROWS);
}

extern "C" gh_status gh_set_packed_rows(gh_handle h, int32_t on) {
    GH_TRY_ST(check_handle(h));
    if (on && !(h->xch.is(GH_LAYOUT_RANK) && h->xch.d_packed.p)) { h->err = "no packed block exchange for this engine (needs gh_rank_layout with world > 1 and fewer components than the row stride)"; return GH_ERR_INVALID; }
    h->xch.packed_exchange = on != 0;
    return GH_OK;
}
extern "C" float *gh_rows_packed_device(gh_handle h) { return h && h->xch.packed_exchange ? h->xch.d_packed.p : nullptr; }
extern "C" gh_status gh_step_unpack_rows(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    if (!h->xch.is(GH_LAYOUT_RANK)) { h->err = "gh_rank_layout has not been called"; return GH_ERR_INVALID; }
    if (!h->xch.packed_exchange) { h->err = "the packed block exchange is not in use (gh_set_packed_rows)"; return GH_ERR_INVALID; }
    return gh_launch_unpack_rows(h);
}
extern "C" gh_status gh_step_finish_own(gh_handle h, const double *stats_all, int32_t world) {
    GH_TRY_ST(check_handle(h));
    if (!h->xch.is(GH_LAYOUT_RANK)) { h->err = "gh_rank_layout has not been called"; return GH_ERR_INVALID; }
    if (!stats_all || world != h->xch.lay.world) { h->err = "bad statistics buffer / world size"; return GH_ERR_INVALID; }
    return gh_step_finish_as(h, GH_FINISH_OWN_ALL_STATS, nullptr, stats_all);
}
extern "C" void *gh_gather_buffer_device(gh_handle h) { return h && h->xch.is(GH_LAYOUT_GATHERED) ? h->xch.d_rows.p : nullptr; }
extern "C" int64_t gh_gather_slot_bytes(gh_handle h) { return h ? h->xch.lay.slot_bytes : 0; }
extern "C" gh_status gh_step_finish_gathered(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    if (!h->xch.is(GH_LAYOUT_GATHERED)) { h->err = "gh_gather_layout has not been called"; return GH_ERR_INVALID; }
    return gh_step_finish_as(h, GH_FINISH_ALL_ROWS);
}

extern "C" gh_status gh_radial_topk(gh_handle h, int32_t k, int32_t *ids) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_radial_topk"));
    if (!ids) { h->err = "ids is NULL"; return GH_ERR_INVALID; }
    if (k < 1 || k > 64 || k > h->n) { h->err = "gh_radial_topk: k must be in [1, min(n, 64)]"; return GH_ERR_INVALID; }
    int nparts = (int)((h->n + 2047) / 2048);
    if (nparts > 256) nparts = 256;
    gh_dev<uint64_t> d_part;
    gh_dev<int32_t> d_ids;
    GH_TRY_ST(gh_alloc(h, d_part, (size_t)nparts * k, false));
    gh_status st = gh_alloc(h, d_ids, (size_t)k, false);
    if (st == GH_OK) st = gh_radial_topk_device(h, k, d_part.p, nparts, d_ids.p);
    if (st == GH_OK && hipMemcpyAsync(ids, d_ids.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, h->stream) != hipSuccess) {
        h->err = "gh_radial_topk: copy failed";
        st = GH_ERR_HIP;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess && st == GH_OK) { h->err = "gh_radial_topk: sync failed"; st = GH_ERR_HIP; }
    return st;   // (the stream has drained: the temporaries may go)
}

// ---- per-phase entry points --------------------------------------------------------

extern "C" gh_status gh_spring_forces(gh_handle h, float *F) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_spring_forces (use gh_spring_forces_f64)"));
    if (!F) { h->err = "F is NULL"; return GH_ERR_INVALID; }
    GH_TRY_ST(gh_launch_spring_only(h, h->d_tmpF.p));
    return download_padded(h, h->d_tmpF.p, F);
}

extern "C" gh_status gh_knn_midpoints(gh_handle h, const int32_t *sampled, int32_t *knn) {
    GH_TRY_ST(check_handle(h));
    if (h->f64) return knn ? gh_f64_knn_midpoints(h, sampled, knn) : GH_ERR_INVALID;
    if (!knn) { h->err = "knn is NULL"; return GH_ERR_INVALID; }
    GH_TRY_ST(check_whole(h, "gh_knn_midpoints"));
    GH_TRY_ST(check_k(h));
    if (!sampled && h->S < h->E) { h->err = "sampled is NULL"; return GH_ERR_INVALID; }
    GH_TRY_ST(caller_ids(h, sampled, &h->sample));
    GH_TRY_ST(step_begin(h, false));  // the same kernels a step runs (spring forces are a by-product)
    const uint64_t *d_keys = h->d_partial.p;
    if (h->cd_part) {   // a GH_DIST_CDIST engine created with a (whole-graph) partition: its rows are decided at the merge
        GH_TRY_ST(gh_knn_merge(h, h->d_partial.p, 1, false));   // (no intersection phase here)
        d_keys = h->d_merged.p;
    }
    std::vector<uint64_t> keys((size_t)h->S * h->K);
    GH_HIP(hipMemcpyAsync(keys.data(), d_keys, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    for (int64_t s = 0; s < h->S; ++s)  // column 0 dropped blindly (pt.py:421)
        for (int c = 1; c < h->K; ++c) knn[s * h->k + (c - 1)] = (int32_t)(keys[(size_t)s * h->K + c] & 0xFFFFFFFFu);
    return GH_OK;
}

extern "C" gh_status gh_intersection_forces(gh_handle h, const int32_t *sampled, const int32_t *knn, float *F) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_intersection_forces (use gh_intersection_forces_f64)"));
    if (!knn || !F) { h->err = "NULL argument"; return GH_ERR_INVALID; }
    GH_TRY_ST(check_whole(h, "gh_intersection_forces"));
    if (!sampled && h->S < h->E) { h->err = "sampled is NULL"; return GH_ERR_INVALID; }
    for (int64_t i = 0; i < h->S * h->k; ++i)
        if (knn[i] < 0 || knn[i] >= h->E) { h->err = "neighbour edge id out of range"; return GH_ERR_INVALID; }
    GH_TRY_ST(caller_ids(h, sampled, &h->sample));
    GH_TRY_ST(gh_ensure_sample(h));
    std::vector<uint64_t> keys((size_t)h->S * h->K, 0);  // the kernel reads ids from key columns 1..k
    for (int64_t s = 0; s < h->S; ++s)
        for (int c = 1; c < h->K; ++c) keys[(size_t)s * h->K + c] = (uint32_t)knn[s * h->k + (c - 1)];
    GH_HIP(hipMemcpyAsync(h->d_merged.p, keys.data(), sizeof(uint64_t) * keys.size(), hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    h->d_keys_cur = h->d_merged.p;
    GH_TRY_ST(gh_launch_intersect(h));
    GH_TRY_ST(gh_launch_inter_to_dense(h, h->d_tmpF.p));
    GH_TRY_ST(gh_launch_inter_cleanup(h));
    return download_padded(h, h->d_tmpF.p, F);
}

extern "C" gh_status gh_integrate_normalise(gh_handle h, const float *Fs, const float *Fi, float *out) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_integrate_normalise"));
    if (!Fs || !Fi || !out) { h->err = "NULL argument"; return GH_ERR_INVALID; }
    GH_TRY_ST(check_whole(h, "gh_integrate_normalise"));
    const size_t bytes = sizeof(float) * (size_t)h->n * h->D;
    GH_HIP(hipMemcpyAsync(h->d_io.p, Fs, bytes, hipMemcpyHostToDevice, h->stream));
    GH_TRY_ST(gh_launch_pad(h, h->d_io.p, h->d_tmpF.p));
    GH_HIP(hipStreamSynchronize(h->stream));
    GH_HIP(hipMemcpyAsync(h->d_io.p, Fi, bytes, hipMemcpyHostToDevice, h->stream));
    GH_TRY_ST(gh_launch_pad(h, h->d_io.p, h->d_tmpF2.p));
    GH_HIP(hipStreamSynchronize(h->stream));
    GH_TRY_ST(gh_launch_integrate_given(h, h->d_tmpF.p, h->d_tmpF2.p));
    // normalise into scratch so the current positions stay unchanged
    GH_HIP(hipMemcpyAsync(h->d_tmpF.p, h->d_pos.p, sizeof(float) * (size_t)h->n * h->LD, hipMemcpyDeviceToDevice, h->stream));
    GH_TRY_ST(gh_launch_normalise(h, GH_FINISH_OWN, false));
    GH_TRY_ST(gh_launch_unpad(h, h->d_pos.p, h->d_io.p));
    GH_HIP(hipMemcpyAsync(out, h->d_io.p, bytes, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(h->d_pos.p, h->d_tmpF.p, sizeof(float) * (size_t)h->n * h->LD, hipMemcpyDeviceToDevice, h->stream));
    gh_step_compact_valid(h, false);   // (the normalise launch wrote the scratch result into the sector-packed table as well)
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

// ---- instrumentation ---------------------------------------------------------------
extern "C" gh_status gh_timing_enable(gh_handle h, int32_t on) {
    GH_TRY_ST(check_handle(h));
    h->timing = on != 0;
    return GH_OK;
}
extern "C" gh_status gh_timing_reset(gh_handle h) {
    GH_TRY_ST(check_handle(h));
    GH_HIP(hipStreamSynchronize(h->stream));
    resolve_timers(h);
    h->timers.clear();
    return GH_OK;
}
extern "C" int32_t gh_timing_count(gh_handle h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    resolve_timers(h);
    return (int32_t)h->timers.size();
}
extern "C" gh_status gh_timing_get(gh_handle h, int32_t i, const char **name, double *total_ms, int64_t *launches) {
    if (!h) return GH_ERR_INVALID;
    if (i < 0 || i >= (int32_t)h->timers.size()) { h->err = "timer index out of range"; return GH_ERR_INVALID; }
    if (name) *name = h->timers[(size_t)i].name.c_str();
    if (total_ms) *total_ms = h->timers[(size_t)i].total_ms;
    if (launches) *launches = h->timers[(size_t)i].launches;
    return GH_OK;
}

// Diagnostic builds of a run (GRAPHEM_HIP_STAMPS set at gh_create): wall-clock stamps (100 MHz) of the last fused
// launch, 8 per workgroup: start, after the spring phase, after its barrier, scan operands ready, scan done, hits flushed;
// after those n_vblocks records, GH_STAMP_EXTRA records of the last normalise launch's first workgroups (set-up
// workgroups first): start, mean / std known, [tile staged], end, -, -, 1 = set-up / 2 = normalising.
extern "C" gh_status gh_debug_stamps(gh_handle h, unsigned long long *out, int64_t count) {
    GH_TRY_ST(check_handle(h));
    if (!h->d_stamps.p) { h->err = "GRAPHEM_HIP_STAMPS was not set when the engine was created"; return GH_ERR_INVALID; }
    const int64_t have = ((int64_t)std::max(h->n_vblocks, 1) + GH_STAMP_EXTRA) * 8;
    GH_HIP(hipStreamSynchronize(h->stream));
    GH_HIP(hipMemcpy(out, h->d_stamps.p, sizeof(unsigned long long) * (size_t)std::min(count, have), hipMemcpyDeviceToHost));
    return GH_OK;
}

extern "C" gh_status gh_knn_last_counts(gh_handle h, int32_t *subset_counts, int32_t *final_counts, int32_t *overflow) {
    GH_TRY_ST(check_handle(h));
    GH_TRY_ST(reject_f64(h, "gh_knn_last_counts"));
    const size_t bytes = sizeof(int32_t) * (size_t)h->S;
    if (subset_counts) GH_HIP(hipMemcpyAsync(subset_counts, h->d_dbg_cnt.p, bytes, hipMemcpyDeviceToHost, h->stream));
    if (final_counts) GH_HIP(hipMemcpyAsync(final_counts, h->d_dbg_cnt.p + h->S, bytes, hipMemcpyDeviceToHost, h->stream));
    if (overflow) GH_HIP(hipMemcpyAsync(overflow, h->d_ovf.p, bytes, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_knn_cdist_stats(gh_handle h, int32_t *full_pass_rows, int32_t *unresolved_tie_rows) {
    GH_TRY_ST(check_handle(h));
    int32_t rare = 0, stat = 0;
    if (h->cdist && h->d_rare.p) {
        const int32_t *hdr = h->d_cd_stat.p + 4 * (h->cd_set ^ 1);  // the counters of the last search
        GH_HIP(hipMemcpyAsync(&rare, hdr, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipMemcpyAsync(&stat, hdr + 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        if (!h->plan.lists()) rare = (int32_t)h->S;   // a graph too small for the filtered scan: every row
    }
    if (full_pass_rows) *full_pass_rows = rare;
    if (unresolved_tie_rows) *unresolved_tie_rows = stat;
    return GH_OK;
}

extern "C" gh_status gh_knn_points(int device_id, const float *q, int64_t nq, const float *ref, int64_t nref,
                                   int32_t D, int32_t k, int64_t *out) {
    auto fail = [&](gh_status st, const std::string &msg) { g_create_error = msg; return st; };
    if (!q || !ref || !out || nq < 0 || nref < 0 || D <= 0 || k <= 0) return fail(GH_ERR_INVALID, "bad argument");
    if ((int64_t)k > nref) return fail(GH_ERR_K_TOO_LARGE, "selected index k out of range");
    if (k > GH_SEL_BUF - GH_SEL_CHUNK) return fail(GH_ERR_INVALID, "k too large for the HIP backend (max 2048)");
    if (nref >= ((int64_t)1 << 31)) return fail(GH_ERR_INVALID, "too many reference points");
    if (hipSetDevice(device_id) != hipSuccess) return fail(GH_ERR_RUNTIME, "invalid device ordinal " + std::to_string(device_id));
    gh_dev<float> d_q, d_ref;
    gh_dev<uint64_t> d_keys;
    std::vector<uint64_t> keys((size_t)nq * k);
    gh_status st = GH_OK;
    std::string err;
    if (!d_q.alloc(sizeof(float) * (size_t)nq * D) || !d_ref.alloc(sizeof(float) * (size_t)nref * D) ||
        !d_keys.alloc(sizeof(uint64_t) * keys.size()))
        return fail(GH_ERR_NOMEM, "hipMalloc failed");
    if (hipMemcpy(d_q.p, q, sizeof(float) * (size_t)nq * D, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_ref.p, ref, sizeof(float) * (size_t)nref * D, hipMemcpyHostToDevice) != hipSuccess)
        return fail(GH_ERR_HIP, "upload failed");
    st = gh_knn_points_device(nullptr, d_q.p, nq, d_ref.p, nref, D, k, d_keys.p, &err);
    if (st == GH_OK && hipMemcpy(keys.data(), d_keys.p, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost) != hipSuccess) {
        st = GH_ERR_HIP;
        err = "download failed";
    }
    if (st != GH_OK) return fail(st, err);
    for (size_t i = 0; i < keys.size(); ++i) out[i] = (int64_t)(keys[i] & 0xFFFFFFFFu);
    return GH_OK;
}

extern "C" int32_t gh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" const char *gh_version(void) { return "graphem_hip 0.1 (gfx950)"; }

extern "C" void gh_debug_live_allocations(int64_t *count, int64_t *bytes) {
    if (count) *count = gh_live_count.load();
    if (bytes) *bytes = gh_live_bytes.load();
}
