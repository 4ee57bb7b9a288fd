// Which launches make up an iteration of the float32 engine: one pure function of the engine's sizes and of what the
// caller or the environment asked for, and the flags that say where a step stands.  Plain C++17, no HIP: it compiles with a
// host compiler alone (tools/step_plan_host_check.cpp sweeps it against the predicate chains it replaced).
// DESIGN.md "Step plan" has the table.
#pragma once
#include <cmath>
#include <stdint.h>

#include "../../include/graphem_hip.h"   // GH_KNN_*, GH_FILTER_*, GH_COARSE_*
#include "exchange_layout.h"             // GH_LAYOUT_*: how a partitioned engine finishes a step

// ---- sizes the choice depends on (the device headers take them from here) ----------------------------------------------
#define GH_SCAN_MIN_EDGES 16384   /* below this many searched edges the per-query block kernel scans everything itself */
#define GH_EXTRACT_MAX_K 128      /* keys the register extraction of the selection kernels takes (select_core.h) */
#define GH_QC_SMAX 256            /* queries of the query-cell table: one staged group, one uint8 index (qcell_core.h) */
#define GH_CT_KMAX 32             /* keys a coarse threshold may stand for (registers of the selecting thread, qcell_core.h gh_ct_tau) */
#define GH_THR_TILE 128           /* subset edges per set-up workgroup (setup_core.h) */
#define GH_THR_GSIZE 64           /* subset edges per group */
#define GH_IVF_TILE 512           /* members per scan workgroup of the inverted-file search (ivf.hip) */
#define GH_IVF_MAX_LISTS 2048
// Fused-kernel geometry (fused.hip): workgroups of 256 threads, 2 references per thread = tiles of 512 owned edges.
#define GH_FUSED_NT 256
#define GH_FUSED_R 2
#define GH_FUSED_TILE (GH_FUSED_NT * GH_FUSED_R)
// A fused launch of at most this many workgroups is a single round or little more: thresholds inside it (gh_tau_place)
#define GH_TAU_EMBED_MAX_VBLOCKS 2048
// The sector-packed gather table (common.h gh_cg_slot): most vertices it is built for, and where GH_COMPACT_AUTO takes it
#define GH_CG_MAX_N ((int64_t)1 << 27)
#define GH_CG_AUTO_MIN_N 400000
#define GH_CG_AUTO_MAX_N 2000000

// ---- input: what the engine is ---------------------------------------------------------------------------------------
struct gh_plan_input {
    int64_t n = 0, rows = 0, E = 0, own_count = 0, S = 0;   // vertices, own rows, edges, edges this rank searches, queries
    int D = 0, LD = 0, k = 0, K = 0, Ksel = 0;              // components, row stride, neighbours, k + 1, keys the selection extracts
    int knn_method = GH_KNN_SCAN;                           // after GH_KNN_AUTO is resolved
    bool cdist = false, cd_part = false;
    bool fused_scan = false;                                // the fused spring+scan kernel can serve this graph / partition
    int n_vblocks = 0;                                      // its workgroups
    int layout = GH_LAYOUT_NONE;
    bool whole() const { return rows == n; }                // the engine holds every row
};

// ---- requests: what the caller or the environment asked for ------------------------------------------------------------
enum gh_tau_place { GH_TAU_BY_SIZE = 0, GH_TAU_SEPARATE, GH_TAU_EMBEDDED };   // GRAPHEM_HIP_TAU_SEPARATE unset | 1 | 0
struct gh_plan_requests {
    int scan_filter = GH_FILTER_AUTO;      // gh_set_scan_filter
    int coarse_mode = GH_COARSE_AUTO;      // gh_set_coarse_tau / GRAPHEM_HIP_COARSE_TAU
    gh_tau_place tau_place = GH_TAU_BY_SIZE;
    bool no_presetup = false;              // GRAPHEM_HIP_NO_PRESETUP
    int compact_gather = GH_COMPACT_OFF;   // gh_set_compact_gather / GRAPHEM_HIP_COMPACT_GATHER (gh_create asks for GH_COMPACT_AUTO)
};

// ---- output ----------------------------------------------------------------------------------------------------------
enum gh_search {
    GH_SEARCH_NONE = 0,   // nothing sampled or no neighbours asked for (S * k = 0): spring forces only
    GH_SEARCH_GRID,       // grid over the midpoints (grid_core.h)
    GH_SEARCH_IVF,        // inverted file (ivf.hip)
    GH_SEARCH_FUSED,      // filtered scan inside the fused spring+scan launch (fused.hip)
    GH_SEARCH_SCAN,       // filtered scan over materialised midpoints, in launches of its own (knn.hip)
    GH_SEARCH_BLOCK       // exhaustive search, one workgroup per query
};
enum gh_prefilter { GH_PRE_NONE = 0, GH_PRE_SPLIT_F16, GH_PRE_WIDE_F16, GH_PRE_CELLS };
enum gh_tau_form {
    GH_TAUF_NONE = 0,     // the search takes no thresholds from the subset (none, grid, IVF, exhaustive)
    GH_TAUF_LAUNCH,       // knn_tau_kernel, a launch of its own
    GH_TAUF_EMBEDDED,     // the first workgroups of the fused launch (tau_core.h)
    GH_TAUF_COARSE        // the first workgroup of the query-cell launch, from coarse group minima (setup_core.h)
};
struct gh_step_plan {
    gh_search built = GH_SEARCH_BLOCK;     // the search the engine's buffers are made for: `search` with queries assumed (never NONE)
    gh_search search = GH_SEARCH_NONE;     // the search an iteration runs
    int64_t thr_stride = 1, thr_M1 = 0;    // the threshold subset: every thr_stride-th searched edge, thr_M1 of them (FUSED / SCAN only)
    gh_prefilter prefilter = GH_PRE_NONE;  // of the engine's fused kernel (at work when search == GH_SEARCH_FUSED; gh_get_scan_filter reports it regardless)
    gh_tau_form tau = GH_TAUF_NONE;
    bool cells_ok = false;                 // capability: the query-cell pre-filter can serve this engine
    bool coarse_ok = false;                // ... and its first workgroup can compute the thresholds (the coarse table is allocated)
    bool presetup = false;                 // a single-rank / form-C-free finish may run the next iteration's KNN set-up in its normalise launch
    bool presetup_gathered = false;        // the same for the gathered finishes (forms B and D)
    bool stage_rows = false;               // the stats_fix launch may stage that set-up's rows (d_setup_rows)
    bool ride_along = false;               // the final selection can reduce the fused kernel's column sums (gh_sums_ride_along)
    bool compact_gather = false;           // the fused kernel reads position rows from the sector-packed 12-byte table (common.h
                                           // gh_cg_slot) whenever that table is up to date (gh_step_state::compact_valid)
    bool lists() const { return built != GH_SEARCH_BLOCK; }   // candidate lists exist (a filtered search)
};

// ---- where a step stands -----------------------------------------------------------------------------------------------
// Written through the functions of engine.h only; the table there (and DESIGN.md) says who sets, reads and clears each.
struct gh_step_state {
    bool new0_ready = false;
    bool intersect_done = false;
    bool stats_reduced = false;
    bool tcount_reset_pending = false;
    bool rows_early = false;
    bool own_ids = false;
    bool compact_valid = false;
    bool pos_shared = false;
};

// The pre-filter of the fused kernels runs on the matrix pipe for every row stride they are built for: split-f16
// operands for D <= 3, single-piece f16 operands for 4 <= D <= 16 (scan_core.h).
inline bool gh_plan_mfma(int LD, int D) { return D <= 16 && (LD == 4 || LD == 8 || LD == 16); }

// Stage 1: the search.  Candidate lists (64 KiB per query) exist for 2..16 components from GH_SCAN_MIN_EDGES searched edges on.
inline gh_search gh_plan_built(const gh_plan_input &in) {
    const bool lists = in.own_count >= GH_SCAN_MIN_EDGES && in.LD <= 16 && in.D >= 2 && in.Ksel <= GH_EXTRACT_MAX_K && in.S <= 0x7FFFFFFF;
    if (!lists) return GH_SEARCH_BLOCK;
    // the grid: 2 or 3 components only (a three-coordinate shadow of a wider ball holds more midpoints than a list takes)
    if (in.knn_method == GH_KNN_GRID && in.D <= 3) return GH_SEARCH_GRID;
    if (in.knn_method == GH_KNN_IVF && !in.cdist && in.own_count >= 64 * 64 &&
        in.own_count < ((int64_t)1 << 31) - (int64_t)GH_IVF_MAX_LISTS * GH_IVF_TILE)
        return GH_SEARCH_IVF;
    return in.fused_scan ? GH_SEARCH_FUSED : GH_SEARCH_SCAN;
}

// Stage 2: stride of the threshold subset.  The set-up evaluates M/stride subset edges against every query (inside the
// normalise launch: ~0.1 us per 1000 rows at 256 queries beyond what the streaming part hides), the final pass then
// meets ~K*stride candidates per query, each a divergent exact re-check + LDS append in the scan and a key in the
// selection.  Measured optimum (rr1m, M = 4M, S*K = 2816): 64 (178 us per iteration; 40: 182, 100: 181); M = 400K: 20.
// That is sqrt(c * M / (S*K)) with c = 3 for the MFMA form of the scan (its hits cost less than half as much as the
// packed-VALU form's, whose balance sits lower).  Bounds: the list holds GH_CAND_CAP candidates (mean K*stride kept
// <= 4096), a workgroup parks its hits in LDS (mean min(S,256)*K*stride*tile/M per query group kept near 300 for a buffer of >= 512), and the
// subset must keep well over K groups of GH_THR_GSIZE rows.
inline int64_t gh_subset_stride(int64_t Mtot, int K, int64_t S, int tile, bool mfma) {
    if (S <= 0) return 2;   // no queries: the smallest stride (what the unbounded quotients below came to)
    // beyond 256 queries the threshold kernel's workgroups no longer run all at once and its cost grows
    // with S like the hits do, so the balance point stops moving
    // (the MFMA form's hits cost less than half as much -- ~0.1 us per unit of stride -- so its balance sits higher)
    int64_t r = (int64_t)std::sqrt((mfma ? 3.0 : 2.0) * (double)Mtot / ((double)(S < 256 ? S : 256) * K));
    const int64_t by_list = 4096 / K;
    if (r > by_list) r = by_list;
    if (r > 256) r = 256;
    // (per query GROUP: the fused kernels empty the buffer between groups once it is a quarter full)
    const int64_t by_hits = (int64_t)(300.0 * (double)Mtot / ((double)(S < 256 ? S : 256) * K * tile));
    if (r > by_hits) r = by_hits;
    if (r < 2) r = 2;
    while (r > 2 && Mtot / r < 8 * (int64_t)K * GH_THR_GSIZE) r /= 2;  // at least 8 K groups: tau stays close to the subset's K-th smallest
    return r;
}

// Stage 3: pre-filter, threshold form and what may be done ahead, once the subset is known.
inline gh_step_plan gh_make_step_plan(const gh_plan_input &in, const gh_plan_requests &rq) {
    gh_step_plan p;
    p.built = gh_plan_built(in);
    p.search = in.S == 0 || in.k == 0 ? GH_SEARCH_NONE : p.built;
    const bool mfma = in.fused_scan && gh_plan_mfma(in.LD, in.D);

    // the grid / IVF searches take their thresholds from their own structures
    if (p.built == GH_SEARCH_FUSED || p.built == GH_SEARCH_SCAN) {
        p.thr_stride = gh_subset_stride(in.own_count, in.Ksel, in.S, GH_FUSED_TILE, mfma);
        p.thr_M1 = (in.own_count + p.thr_stride - 1) / p.thr_stride;
    }

    // The query-cell pre-filter (spring_scan_cells_kernel) serves D <= 3 with up to GH_QC_SMAX queries.  Its first workgroup
    // can take the thresholds from coarse group minima itself on a whole-graph engine with a threshold subset and at most
    // GH_CT_KMAX keys to bound.
    p.cells_ok = mfma && in.D <= 3 && in.S >= 1 && in.S <= GH_QC_SMAX;
    p.coarse_ok = p.cells_ok && p.thr_M1 > 0 && in.whole() && in.Ksel <= GH_CT_KMAX;
    // Thresholds by the first workgroups of the fused launch where that launch is a single round of workgroups or little
    // more: there the iteration is a chain of launch latencies and this removes one (100 K vertices: 64.9 -> 60.6 us).  A
    // large graph gains nothing (1 M vertices: 175.7 -> 176.7 us) and keeps the launch of its own.
    const bool embed = rq.tau_place == GH_TAU_EMBEDDED || (rq.tau_place == GH_TAU_BY_SIZE && in.n_vblocks <= GH_TAU_EMBED_MAX_VBLOCKS);
    // AUTO takes the cells wherever the thresholds have a launch of their own anyway (the table is built from thresholds
    // already in memory, or from coarse minima); where they are computed inside the fused launch the split-f16 form stays
    const bool cells = (rq.scan_filter == GH_FILTER_CELLS || (rq.scan_filter == GH_FILTER_AUTO && !embed)) && p.cells_ok;
    p.prefilter = !mfma ? GH_PRE_NONE : in.D > 3 ? GH_PRE_WIDE_F16 : cells ? GH_PRE_CELLS : GH_PRE_SPLIT_F16;
    // Coarse thresholds: AUTO takes them where they were measured ahead -- three components, up to a dozen keys: rr1m 153.8
    // -> 149.9 us per iteration, er1m 191.2 -> 186.1, pp1m 182.6 -> 177.3 (NOTES.md "Coarse thresholds") -- and leaves the
    // two-dimensional and the 32-key kernels, whose smaller batches were not measured at scale, to a request
    const bool want_coarse = rq.coarse_mode == GH_COARSE_ON || (rq.coarse_mode == GH_COARSE_AUTO && in.D == 3 && in.Ksel <= 12);
    if (p.search == GH_SEARCH_SCAN) p.tau = GH_TAUF_LAUNCH;
    else if (p.search == GH_SEARCH_FUSED)
        p.tau = cells ? (want_coarse && p.coarse_ok ? GH_TAUF_COARSE : GH_TAUF_LAUNCH) : embed ? GH_TAUF_EMBEDDED : GH_TAUF_LAUNCH;

    // The next iteration's KNN set-up inside this one's normalise launch.  The two finishes differ: the single-rank one admits
    // the grid and IVF searches of any engine, the gathered one only those of an engine the fused kernel could serve
    // (the reason is not recorded; kept as found).
    const bool ahead = !rq.no_presetup && (p.search == GH_SEARCH_FUSED || p.search == GH_SEARCH_GRID || p.search == GH_SEARCH_IVF);
    p.presetup = ahead && in.whole() && in.layout != GH_LAYOUT_GATHERED;
    p.presetup_gathered = ahead && in.fused_scan;
    p.stage_rows = p.thr_M1 > 0 && in.whole() && in.layout == GH_LAYOUT_NONE;
    // (not with thousands of queries: there the wave-per-query selection is worth more than the ride, and stats_fix_kernel
    // adds the column sums up itself)
    p.ride_along = in.rows > 0 && in.LD <= 16 && in.S < 2048;
    // Position rows of the fused D <= 3 kernels from the sector-packed table: three components in rows of four floats, the
    // whole graph on one rank (its normalise launch writes every row of the table beside the positions), and byte offsets
    // into the table that fit 32 bits.  AUTO: GH_CG_AUTO_MIN_N .. GH_CG_AUTO_MAX_N vertices, where it was measured ahead
    // (NOTES.md "The sector-packed gather table"): below, both tables fit the L2s; above, neither does to any extent.
    const bool cg_ok = p.search == GH_SEARCH_FUSED && in.D == 3 && in.LD == 4 && in.whole() && in.layout == GH_LAYOUT_NONE &&
                       in.n <= GH_CG_MAX_N;
    p.compact_gather = cg_ok && (rq.compact_gather == GH_COMPACT_ON ||
                                 (rq.compact_gather == GH_COMPACT_AUTO && in.n >= GH_CG_AUTO_MIN_N && in.n <= GH_CG_AUTO_MAX_N));
    return p;
}

// The column sums of the fused kernel's workgroup partials ride along with the final selection launch of this step
// (stats_fix_kernel then skips them).
inline bool gh_sums_ride_along(const gh_step_plan &p, const gh_step_state &s) { return s.new0_ready && p.ride_along; }
