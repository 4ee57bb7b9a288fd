// Internal engine state shared by the translation units of libgraphem_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <string>
#include <vector>

#include "../../include/graphem_hip.h"
#include "host_util.h"   // GH_HIP, GH_TRY_ST, GH_LAUNCH_CHECK
#include "step_plan.h"   // gh_step_plan, gh_step_state and the sizes the choice of path depends on
#include "exchange_layout.h"   // gh_exchange_layout, gh_stats_rows

// Candidate-list capacity per query in the filtered KNN scan, and the LDS sort size.
#define GH_CAND_CAP 16384   /* (8192 until round 3: one query of a 16 M-vertex run reached 8777 candidates and its exhaustive fallback cost 0.5 s) */
#define GH_SEL_BUF 4096
#define GH_SEL_CHUNK 2048
// Candidate counters are padded to one per 128-byte line: adjacent counters serialise their
// returning atomics on one L2 line (~11 ns each, measured: 16 K appends per line cost 180 us).
#define GH_CNT_STRIDE 32
// Spare rows behind the n positions so equal all-gather chunks fit for any world size <= this.
#define GH_POS_PAD_ROWS 1024
// Coarse form of the threshold group minima (setup_core.h "COARSE FORM"): groups per query and the value of an empty entry
// (the most keys a threshold may stand for, GH_CT_KMAX, is in step_plan.h).
#define GH_CT_M 64
#define GH_CT_EMPTY 0xFFFFFFFFu

struct gh_timer_slot {
    std::string name;
    double total_ms = 0.0;
    int64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// Where the sample ids of an iteration come from.  The values are gh_setup_args::mode on the device (setup_core.h).
enum { GH_IDS_GIVEN = 0, GH_IDS_SAMPLER = 1, GH_IDS_ARANGE = 2 };
struct gh_ids {
    int mode;       // GH_IDS_GIVEN: the ids are at `ids`; GH_IDS_SAMPLER / GH_IDS_ARANGE: produced into `ids` (d_sampled)
    int32_t *ids;   // a view (mutable: the set-up writes the ids it draws)
};

// Parts of the engine whose types are complete only in their own translation units: each defines its gh_delete there.
struct gh_comm;   // comm.hip: collective backend of the native partitioned loop
struct gh_f64;    // f64.hip: state of a float64 engine (gh_create_f64)
struct gh_ivf;    // ivf.hip: buffers of the inverted-file search (GH_KNN_IVF)
void gh_delete(gh_comm *);
void gh_delete(gh_f64 *);
void gh_delete(gh_ivf *);
struct gh_part_delete {
    template <class T> void operator()(T *p) const { gh_delete(p); }
};

// gh_run_torch_sampled (api.hip): pinned upload slots for the rows a host thread draws (torch.randperm's prefixes), one
// event per slot (recorded behind the slot's copy: the slot is reused once it has fired)
#define GH_RING_SLOTS 8
#define GH_RING_CHUNK 32   /* rows per slot = per copy, at most */
struct gh_ring {
    int32_t *host = nullptr;
    size_t cap = 0;              // int32 words allocated in host (GH_RING_SLOTS * GH_RING_CHUNK * S)
    uint64_t uploads = 0;        // copies out of host so far, over all calls: slot = uploads % GH_RING_SLOTS
    hipEvent_t ev[GH_RING_SLOTS] = {};
    gh_ring() = default;
    gh_ring(const gh_ring &) = delete;
    gh_ring &operator=(const gh_ring &) = delete;
    ~gh_ring() {
        if (host) (void)hipHostFree(host);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The exchange of a row-partitioned step: the layout value and the buffers it sizes (exchange_layout.h describes both, and
// alone knows how a slot or a late block is laid out).  Written by the layout setter (api.hip set_layout) only;
// packed_exchange also by gh_set_packed_rows.
struct gh_exchange {
    gh_exchange_layout lay;
    gh_dev<float> d_rows, d_packed;   // lay.rows_floats, lay.packed_floats
    gh_dev<double> d_late;            // lay.late_all_doubles
    bool packed_exchange = false;     // form C: the finished blocks travel packed (default: lay.packed_default)
    bool is(int form) const { return lay.form == form; }
    float *travelling_rows() const { return d_packed.p ? d_packed.p : d_rows.p; }   // forms B, D: what the rows' all-gather fills
    // forms B, D: the buffer the ranks' statistics lie in (rank r's rows at lay.first_stats + r * lay.late_doubles)
    double *stats_buffer() const { return is(GH_LAYOUT_GATHERED) ? reinterpret_cast<double *>(d_rows.p) : d_late.p; }
};

// Ownership is stated by type: a gh_dev member owns its device memory, a raw pointer is a view into memory owned
// elsewhere, and deleting the engine releases everything it holds.
struct gh_engine {
    ~gh_engine();   // (api.hip) destroys own_stream; the members release themselves
    int device = 0;
    int64_t n = 0, E = 0;
    int D = 0, LD = 0, k = 0, K = 0;
    int64_t S = 0;
    gh_params prm{};
    gh_partition part{};
    int64_t rows = 0;       // part.row_hi - part.row_lo
    uint64_t iter = 0;      // iterations done (device sampler counter)
    std::string err;

    hipStream_t stream = nullptr;       // stream all work is enqueued on
    hipStream_t own_stream = nullptr;   // created by gh_create, destroyed by ~gh_engine
    int64_t pos_rows = 0;               // rows allocated in d_pos (n + GH_POS_PAD_ROWS)

    // graph
    gh_dev<int32_t> d_edges;      // (E, 2)
    gh_dev<int32_t> d_rowptr;     // (rows + 1) pull lists of own rows, reference summation order
    gh_dev<int32_t> d_adj;        // neighbours
    int64_t adj_len = 0;
    gh_dev<int32_t> d_first_edge;    // (rows + 1) offset of each own row's owned edges: the first owned edge id
                                     // (rule A: smaller endpoint owns) or a prefix count into d_own_eids (rule B)
    gh_dev<int32_t> d_own_eids;      // rule B (balanced ownership of partitioned engines): ids of the owned edges
                                     // in (row, list) order; null under rule A
    int64_t own_count = 0;           // edges this rank owns (midpoints in d_mid, searched by its KNN kernels)
    int64_t mid_base = 0;            // d_mid row of an owned edge = d_first_edge offset - mid_base
    bool fused_mid = false;       // own edge range == edges owned by own rows: spring kernel writes midpoints
    gh_dev<int32_t> d_long_rows;      // local ids of the own rows with more than GH_LONG_DEG neighbours (common.h)
    gh_dev<int32_t> d_long_ownptr;    // their owned (hub-hub) edges: offsets ...
    gh_dev<int32_t> d_long_ownadj;    // ... and neighbours
    gh_dev<int32_t> d_long_eptr;      // (nlong + 1) prefix of their degrees
    gh_dev<int32_t> d_long_erow;      // (long_entries) index of the long row a list entry belongs to
    gh_dev<uint8_t> d_own_long;       // (own_count) owned-edge slots whose owner row is long (common.h gh_long_midpoints)
    gh_dev<float> d_long_terms;       // (long_entries * D) force terms of their neighbours, component-major per row
    int nlong = 0;
    int long_deg = 128;               // rows with more neighbours than this are long (common.h gh_long_degree)
    int64_t long_entries = 0;
    int long_max_deg = 0;             // longest long row (forces.hip: one launch for the long rows when moderate)
    gh_dev<float> d_mid;          // (own_count, LD) midpoints of the own edges, current iteration
    gh_dev<float> d_Fs;           // (rows, LD) spring forces of the own rows
    gh_dev<float> d_gmin;         // (S, Gpad) group minima of the threshold subset (setup_core.h), float bits
    gh_dev<int32_t> d_sub_uv;     // (thr_M1, 2) endpoints of the subset edges
    gh_dev<int32_t> d_vblock;     // (n_vblocks + 1) vertex ranges of the fused spring+scan workgroups
    int n_vblocks = 0;
    bool fused_scan = false;      // fused spring+scan kernel usable for this graph / partition

    // state
    gh_dev<float> d_pos;          // (n, LD)
    gh_dev<float> d_cg;           // (gh_cg_bytes(n)) the rows of d_pos without pad columns, five to a 64-byte sector (common.h
                                  // gh_cg_slot): what the fused kernel gathers from while step.compact_valid.  Allocated only
                                  // where plan.compact_gather asks for it (gh_ensure_compact_table)
    int64_t compact_launches = 0; // fused launches so far that ran the sector-packed instantiation (gh_compact_gather_launches)
    gh_dev<float> d_new_buf;      // (rows, LD) the engine's own storage for ...
    float *d_new = nullptr;       // ... the un-normalised update of own rows.  A view: d_new_buf, or the own block of xch.d_rows (forms B, D)
    gh_dev<float> d_tmpF;         // (n, LD) scratch for the per-phase entry points
    gh_dev<float> d_tmpF2;
    gh_dev<float> d_io;           // (n, D) staging for unpadded host copies

    // intersection accumulators
    gh_dev<double> d_acc;         // (n, LD) zero between iterations
    gh_dev<int32_t> d_tflag;      // (n) zero between iterations
    gh_dev<int32_t> d_touched;    // (4 * S * k)
    gh_dev<int32_t> d_tcount;     // (1)

    // knn
    gh_dev<int32_t> d_sampled;    // (S) owned buffer
    gh_ids sample{};                  // ids of the current iteration: d_sampled or a row of d_stream_ids, GH_IDS_GIVEN once
                                      // produced (the sampler / arange run inside knn_setup_kernel or by gh_ensure_sample)
    gh_dev<int32_t> d_stream_ids;     // (iters, S) uploaded sample stream of gh_run
    size_t stream_ids_cap = 0;
    gh_ring ring;                     // gh_run_torch_sampled
    double sampler_stats[4] = {0, 0, 0, 0};   // last gh_run_torch_sampled, host ms: producer drawing, caller waiting for a pinned slot, caller waiting for ids, the call
    // The protocol of a step: which launches make it up, where it stands, and what was done ahead for the next one.
    gh_plan_requests requests;    // what the caller / the environment asked for (gh_create, gh_set_scan_filter, gh_set_coarse_tau)
    gh_step_plan plan;            // what follows from them and the sizes above: written by gh_replan only
    gh_step_state step;           // written through the gh_step_* functions below only (the table there)
    struct {
        bool valid = false;       // the last normalise launch also ran the KNN set-up of iteration `iter` from `src`
        gh_ids src{};             //   (gh_knn_prepare then skips its kernel)
        uint64_t iter = 0;
        bool rows = false;        // (not yet valid) the last stats_fix launch staged the queries' raw endpoint rows of that
                                  //   set-up in d_setup_rows, for the normalise launch right behind it
    } lookahead;                  // read and written through the gh_*lookahead* functions below only
    gh_dev<float> d_setup_rows;   // (2 S, LD) un-normalised rows of the next queries' endpoints, rows 2s, 2s + 1 for query s
                                  // (setup_core.h gh_setup_gather); whole-graph engines with threshold tiles only
    gh_dev<float> d_iscratch;     // (S * k, LD) per-pair scratch of the intersection kernel
    gh_dev<float> d_q;            // (S, QS) query records: midpoint coordinates + tau (knn.hip gh_qs)
    gh_dev<float> d_qscan;        // (S, QS) pre-filter records (-2q, t) written by the threshold kernel
    gh_dev<uint16_t> d_qA;        // (S, 16) f16 A-operand rows of the split-f16 MFMA pre-filter (D <= 3), same kernel
    gh_dev<int32_t> d_order;          // internal row of every vertex (BFS reordering), or null: identity
    std::vector<int32_t> order_host;  // the same on the host (empty: identity)
    gh_exchange xch;              // what a row partition exchanges to finish a step; d_new and d_stats may be views into it
    gh_dev<int32_t> d_qexact;     // [0] = count, [1..] = queries outside the f16 range (scanned exactly)
    gh_dev<uint64_t> d_cand;      // (S, GH_CAND_CAP)
    gh_dev<int32_t> d_cnt;        // (S * GH_CNT_STRIDE) one counter per 128-byte line
    gh_dev<int32_t> d_ovf;        // (S)
    gh_dev<int32_t> d_sel_redo;   // (S) queries knn_select_wave_kernel left to the workgroup form (zero between launches)
    gh_dev<int32_t> d_tq_count, d_tq_base, d_tq_touched;                            // (S), (S), (S, 4 k): per-query runs of the touched list (S >= 2048)
    gh_dev<int32_t> d_dbg_cnt;    // (2, S) candidate-list lengths seen by the last subset / final select
    gh_dev<uint64_t> d_partial;   // (S, K) this rank's best keys, ascending
    gh_dev<uint64_t> d_merged;    // (S, K) keys merged over the ranks (world > 1)
    const uint64_t *d_keys_cur = nullptr;  // view: the keys the intersection phase reads, d_partial or d_merged

    // GH_DIST_CDIST (cdist.hip): the reference's cdist + topk values and tie order
    bool cdist = false;
    bool cd_part = false;             // ... on a row partition: d_partial holds (S, K + 2) per-rank records, the rows are decided at the merge (cdist.hip)
    bool cd_all_ties = false;         // gh_set_cdist_replay: the loop lists every tie too (rows column for column), not only those that can change a force
    int Ksel = 0;                     // keys the candidate selection extracts: K, or K + 1 with cdist (boundary ties)
    gh_dev<int32_t> d_rare;           // [1..S] = the listed queries: partial_sort's heap is replayed for them
    gh_dev<int32_t> d_cd_rows;        // (2, S) per listed slot: prefix length P (ids below it are valued), tail length
    gh_dev<float> d_cd_vbuf;          // (cd_R, cd_nchunks * 64) cdist values of those queries against the edges below P
    gh_dev<float> d_cd_cmin;          // (cd_R, cd_nchunks) minimum of each chunk of 64 edge ids
    gh_dev<int32_t> d_cd_stat;        // two sets (used alternately) of [0] listed rows, [1] rows whose tie order ATen leaves to std::nth_element (not reproduced), [2] the longest prefix
    int cd_R = 0, cd_nchunks = 0, cd_set = 0;   // cd_set: the counter set the NEXT search uses

    // grid KNN (grid_core.h; GH_KNN_GRID)
    int grid_G = 0, grid_bits = 0;
    int64_t grid_cells = 0;
    size_t grid_temp_bytes = 0;
    gh_dev<uint32_t> d_grid_u32;      // keys, rows, sorted keys, sorted rows, cell starts, sorted edge ids
    gh_dev<float> d_grid_smid;        // (own_count) float4 midpoints in cell order
    gh_dev<unsigned char> d_grid_temp; // radix sort scratch

    // normalisation
    gh_dev<double> d_blockstats;    // (nblocks, 2, LD)
    int nblocks_update = 0;
    gh_dev<double> d_stats_buf;     // the engine's own storage for ...
    double *d_stats = nullptr;      // ... (gh_stats_rows(LD), LD): sum, sum of squares, then correction row pairs;
                                    // summed elementwise over the ranks by the caller when partitioned.  A view: d_stats_buf,
                                    // or the own statistics in xch.d_rows (form B) / xch.d_late (form D)

    // thresholds inside the fused launch (tau_core.h; plan.tau == GH_TAUF_EMBEDDED)
    gh_dev<unsigned> d_tau_flag;         // queries published so far by the current fused launch
    // the query-cell table of the D <= 3 fused kernel's phase B (qcell_core.h; plan.prefilter == GH_PRE_CELLS)
    gh_dev<uint32_t> d_qcell;            // (GH_QC_WORDS) the table of the current launch, built by its first workgroup
    gh_dev<unsigned> d_qc_flag;          // launch number whose table is complete
    unsigned qc_epoch = 0;               // number of the last launch on the query-cell path
    gh_dev<int32_t> d_wait_failed;       // a consumer gave up waiting: reported by gh_sync / gh_get_positions
    // thresholds by workgroup 0 of the query-cell launch, from coarse group minima (setup_core.h "COARSE FORM";
    // plan.tau == GH_TAUF_COARSE: no d_gmin, no knn_tau_kernel launch)
    gh_dev<uint32_t> d_cmin;             // (2, GH_CT_M, S) float bits, GH_CT_EMPTY where no set-up workgroup has written: copy
                                         // (iter & 1) is filled by the set-up of iteration iter and consumed, and reset, by its fused launch
    bool cmin_dirty[2] = {false, false}; // a set-up has written the copy and no fused launch has consumed it yet (a set-up done
                                         // ahead that turned out stale): the next set-up into it fills it with GH_CT_EMPTY first.
                                         // gh_cmin_claim / gh_cmin_release only

    // timing

#define GH_STAMP_EXTRA 8192
    gh_dev<unsigned long long> d_stamps;      // GRAPHEM_HIP_STAMPS: (n_vblocks, 8) wall-clock stamps of the last fused launch
    bool timing = false;
    std::vector<gh_timer_slot> timers;

    // (last, so that they go first, in this order: comm, f64, ivf)
    std::unique_ptr<gh_ivf, gh_part_delete> ivf;     // GH_KNN_IVF (ivf.hip)
    std::unique_ptr<gh_f64, gh_part_delete> f64;     // non-null: a float64 engine -- only this, the sizes, the parameters and the stream are in use
    std::unique_ptr<gh_comm, gh_part_delete> comm;
};

// The allocator of the engine's translation units: `count` elements (at least one) into `buf`, whose earlier allocation, if
// any, is released first; zero: filled with zeros on the engine's stream.
template <class T> gh_status gh_alloc(gh_engine *h, gh_dev<T> &buf, size_t count, bool zero) {
    if (count == 0) count = 1;
    if (!buf.alloc(count * sizeof(T))) {
        h->err = std::string("hipMalloc failed: ") + hipGetErrorString(hipGetLastError());
        return GH_ERR_NOMEM;
    }
    if (zero) GH_HIP(hipMemsetAsync(buf.p, 0, count * sizeof(T), h->stream));
    return GH_OK;
}

// The engine's own ids for an iteration: arange(E) when S >= E (pt.py:412, no randomness consumed: SURVEY Q9), else the
// device sampler.
inline gh_ids gh_own_ids(const gh_engine *h) { return gh_ids{h->S >= h->E ? GH_IDS_ARANGE : GH_IDS_SAMPLER, h->d_sampled.p}; }
// The normalise launch just enqueued also set up iteration iter + 1 from *next; null: nothing is set up ahead (any more).
// Either way the rows a stats_fix launch staged are spent: they belong to the one normalise launch behind it.
inline void gh_set_lookahead(gh_engine *h, const gh_ids *next) {
    h->lookahead.valid = next != nullptr;
    h->lookahead.rows = false;
    if (next) { h->lookahead.src = *next; h->lookahead.iter = h->iter + 1; }
}
// The stats_fix launch just enqueued also gathered, into d_setup_rows, the rows the set-up of iteration iter + 1 from
// `next` reads.
inline void gh_set_lookahead_rows(gh_engine *h, const gh_ids &next) {
    h->lookahead.valid = false;
    h->lookahead.rows = true;
    h->lookahead.src = next;
    h->lookahead.iter = h->iter + 1;
}
inline bool gh_lookahead_rows_for(const gh_engine *h, const gh_ids *next) {
    return next && h->lookahead.rows && h->lookahead.iter == h->iter + 1 && h->lookahead.src.mode == next->mode &&
           h->lookahead.src.ids == next->ids;
}
// The rows a stats_fix launch staged are spent (or no longer wanted); a set-up done ahead stays.
inline void gh_drop_lookahead_rows(gh_engine *h) { h->lookahead.rows = false; }
// The set-up of the current iteration was done ahead, from these ids (gh_knn_prepare then skips its kernel).
inline bool gh_lookahead_done_for(const gh_engine *h, const gh_ids &src) {
    return h->lookahead.valid && h->lookahead.iter == h->iter && h->lookahead.src.mode == src.mode && h->lookahead.src.ids == src.ids;
}
// A set-up done ahead is stale (another threshold form, a failed wait); rows staged for one stay.
inline void gh_drop_lookahead(gh_engine *h) { h->lookahead.valid = false; }

// gh_step_state (step_plan.h), field by field: who sets it, who reads it, where it is cleared.
//   new0_ready            set: gh_launch_spring_scan (the fused kernel wrote d_new = pos + Fs and its block sums).
//                         read: step_begin (form D: else a launch of its own), the final selection (gh_sums_ride_along),
//                         gh_launch_integrate.  cleared: gh_step_sums_spent in gh_launch_integrate, their one consumer; a search
//                         without a step (gh_knn_midpoints) leaves it to the gh_step_reset of the next step.
//   stats_reduced         set: the final selection launch (launch_select, gh_knn_finish_cdist) when the sums rode along.
//                         read: gh_launch_integrate (stats_fix_kernel skips them).  cleared: as new0_ready.
//   intersect_done        set: whatever launch ran the intersection phase of this step (the final selection, the exhaustive
//                         search, the merges; a step without queries has none to run).  read: step_merge.  cleared: gh_step_reset.
//   tcount_reset_pending  written: gh_knn_prepare, every step (the set-up was done ahead: a later launch of this step must
//                         reset d_tcount).  read: the threshold launch, the grid build, the coarse query-cell launch.
//   rows_early            set: step_begin under form D (new0 of the own rows is in its block: the rows may travel).
//                         read: gh_step_rows_early, gh_step_finish_as, which clears it; gh_step_reset.
//   own_ids               written: gh_step_begin / gh_step_begin_device_ids, every split step (called without ids: device
//                         sampler / arange).  read: the gathered finishes (they set the next draw up).
//   compact_valid         set: the two launches that write every row of d_cg beside d_pos -- pad_kernel (gh_set_positions) and
//                         the normalise launch of a whole-graph single-rank finish (gh_launch_normalise) -- when the plan
//                         asks for the table.  read: the fused launch (fused.hip fused_compact: else the padded instantiation).
//                         cleared: by everything else that can change d_pos or leave d_cg behind it -- every other normalise
//                         launch, gh_integrate_normalise, a failed device wait, gh_set_compact_gather; and it stays clear once
//                         pos_shared is set.  Not by gh_step_reset: it outlives the step.
//   pos_shared            set: gh_positions_device, for good -- a caller that holds the pointer may write the rows between any two
//                         steps, so from then on no launch of this engine trusts the copy.  read: gh_step_compact_valid,
//                         gh_get_compact_gather.  never cleared.
inline void gh_step_compact_valid(gh_engine *h, bool valid) { h->step.compact_valid = valid && !h->step.pos_shared; }
inline void gh_step_pos_shared(gh_engine *h) { h->step.pos_shared = true; h->step.compact_valid = false; }
inline void gh_step_reset(gh_engine *h) {   // the start of a step's launches
    h->step.new0_ready = h->step.stats_reduced = h->step.intersect_done = h->step.rows_early = false;
}
inline void gh_step_new0_ready(gh_engine *h) { h->step.new0_ready = true; }
inline void gh_step_stats_reduced(gh_engine *h) { h->step.stats_reduced = true; }
inline void gh_step_sums_spent(gh_engine *h) { h->step.new0_ready = h->step.stats_reduced = false; }
inline void gh_step_intersect_done(gh_engine *h) { h->step.intersect_done = true; }
inline void gh_step_tcount_reset_pending(gh_engine *h, bool pending) { h->step.tcount_reset_pending = pending; }
inline void gh_step_set_rows_early(gh_engine *h, bool early) { h->step.rows_early = early; }
inline void gh_step_own_ids(gh_engine *h, bool own) { h->step.own_ids = own; }

// What a finish normalises, and from what: the own rows from the own statistics (single-rank steps, per-phase entry
// points), the own rows from every rank's statistics (form C), all n rows from the gathered blocks (forms B and D).
enum gh_finish_kind { GH_FINISH_OWN, GH_FINISH_OWN_ALL_STATS, GH_FINISH_ALL_ROWS };

// RAII-free helper: records start/stop events around a launch when timing is on.
struct gh_scope {
    gh_engine *h;
    int slot = -1;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t stream = nullptr;
    gh_scope(gh_engine *h_, const char *name, hipStream_t on = nullptr /* null: the engine's stream */);
    ~gh_scope();
};

// graph_plan.hip: what gh_create uploads about the graph, computed on the host.  gh_plan_graph also sets the engine's graph
// scalars (part, order_host, adj_len, own_count, mid_base, fused_mid, the long-row counts, fused_scan, n_vblocks), which the
// policy functions below read.
struct gh_graph_plan {
    const int32_t *edges = nullptr;   // (E, 2) the edge list in internal vertex numbers: `internal` or the caller's
    std::vector<int32_t> internal;    // ... renumbered by the vertex order (empty: identity)
    std::vector<int32_t> rowptr, adj; // pull lists of the own rows, bit 31 of an entry: the row owns the edge
    std::vector<int32_t> first_edge, own_eids, vblock;
    std::vector<int32_t> long_rows, long_ownptr, long_ownadj, long_eptr, long_erow;
    std::vector<uint8_t> own_long;
    std::vector<int32_t> sub_uv;      // (thr_M1, 2) endpoints of the threshold subset
};
void gh_plan_graph(gh_engine *h, const int32_t *edges, bool partitioned, int reorder, gh_graph_plan *g);
void gh_auto_knn_method(gh_engine *h);   // GH_KNN_AUTO -> prm.knn_method (and the IVF parameters): needs own_count
void gh_plan_threshold_subset(const gh_engine *h, gh_graph_plan *g);   // needs thr_stride / thr_M1
// pull lists of all n rows without ownership bits (the float64 engine)
void gh_pull_lists(int64_t n, int64_t E, const int32_t *edges, std::vector<int32_t> &rowptr, std::vector<int32_t> &adj);
// api.hip
void gh_replan(gh_engine *h);   // plan from the engine's sizes and requests: the only writer of it.  Drops a set-up done ahead when the threshold form changed
// api.hip / comm.hip
// keys of all ranks -> merge, intersection forces, own rows integrated (gh_step_merge).  next: the ids the finish will set
// the next iteration up from, when the caller knows them by now
gh_status gh_step_merge_keys(gh_engine *h, const uint64_t *gathered, int world, const gh_ids *next = nullptr);
// the one finish behind gh_step_finish / _gathered / _own / _overlap.  next: GH_FINISH_OWN, the ids of the next iteration
// where known; stats_all: GH_FINISH_OWN_ALL_STATS, the (world, gh_stats_rows, LD) statistics of every rank
gh_status gh_step_finish_as(gh_engine *h, gh_finish_kind kind, const gh_ids *next = nullptr, const double *stats_all = nullptr);
gh_status gh_upload_sample_stream(gh_engine *h, int32_t iters, const int32_t *sample_stream, int32_t **d_ids);
gh_status gh_step_begin_device_ids(gh_engine *h, int32_t *dev_ids);
// f64.hip
void gh_set_create_error(const std::string &msg);   // (api.hip) message gh_last_error(NULL) returns
// (api.hip) argument and device checks of gh_create / gh_create_f64; f64_max_D > 0: the float64 engine's, with its k_attr
gh_status gh_check_create_args(int device_id, int64_t n, int32_t D, int64_t E, const int32_t *edges, const gh_params *params,
                               int f64_max_D = 0, double f64_k_attr = 0.0);
gh_status gh_f64_set_positions_f32(gh_engine *h, const float *pos);
gh_status gh_f64_get_positions_f32(gh_engine *h, float *pos);
gh_status gh_f64_step(gh_engine *h, const int32_t *sampled);
gh_status gh_f64_run(gh_engine *h, int32_t iters, const int32_t *sample_stream);
gh_status gh_f64_knn_midpoints(gh_engine *h, const int32_t *sampled, int32_t *knn);
// knn.hip
gh_status gh_knn_local(gh_engine *h, bool fuse_intersect);  // d_sampled, d_mid -> d_partial (unfused)
struct gh_setup_args;
gh_setup_args gh_make_setup_args(const gh_engine *h, gh_ids src, uint64_t iter);  // setup_core.h
unsigned gh_setup_blocks(const gh_setup_args &a);
int64_t gh_gmin_floats(const gh_engine *h);   // size of d_gmin
gh_status gh_knn_prepare(gh_engine *h);
gh_status gh_knn_thresholds(gh_engine *h, int64_t groups = 0);   // groups > 0: d_gmin holds (S, groups) minima written by the caller (ivf.hip)
struct gh_tau_args;
gh_tau_args gh_make_tau_args(gh_engine *h);  // tau_core.h
gh_status gh_knn_finish(gh_engine *h, bool have_mid, bool fuse_intersect);
gh_status gh_knn_points_device(hipStream_t stream, const float *d_q, int64_t nq, const float *d_ref, int64_t nref,
                               int D, int K, uint64_t *d_keys, std::string *err);
// cdist.hip
gh_status gh_cdist_alloc(gh_engine *h);
gh_status gh_knn_merge_cdist(gh_engine *h, const uint64_t *gathered, int world, bool with_intersect);   // row partitions: the ranks' (S, K + 2) records -> d_merged, the reference's rows
gh_status gh_knn_finish_cdist(gh_engine *h, bool all_rows, bool fuse_intersect);   // candidate lists (or nothing) -> d_partial, the reference's rows
// grid_core.h
gh_status gh_grid_alloc(gh_engine *h);
gh_status gh_grid_search(gh_engine *h);            // d_mid + tau -> candidate lists
// ivf.hip
gh_status gh_ivf_alloc(gh_engine *h);
gh_status gh_ivf_search(gh_engine *h);             // d_mid + query records -> tau and candidate lists (probed lists only)
// fused.hip
gh_status gh_radial_topk_device(gh_engine *h, int K, uint64_t *d_part, int nparts, int32_t *d_ids);
gh_status gh_cmin_claim(gh_engine *h, uint64_t iter);   // before enqueueing a coarse set-up of iteration iter: its table copy is empty
inline void gh_cmin_release(gh_engine *h, uint64_t iter) { h->cmin_dirty[iter & 1] = false; }   // its fused launch consumed the copy, and reset it entry by entry
gh_status gh_launch_spring_scan(gh_engine *h);             // d_Fs + final-level candidates in one kernel
// -> d_keys_cur; with_intersect: the merge launch (more than one rank, or a partitioned GH_DIST_CDIST engine) also runs the intersection phase
gh_status gh_knn_merge(gh_engine *h, const uint64_t *gathered, int world, bool with_intersect);
// forces.hip
gh_status gh_launch_intersect(gh_engine *h);               // d_sampled, d_keys_cur -> d_acc/d_touched
gh_status gh_launch_inter_cleanup(gh_engine *h);
gh_status gh_launch_spring_mid(gh_engine *h);              // -> d_Fs, d_mid
gh_status gh_launch_mid_only(gh_engine *h);                // -> d_mid
// d_Fs, d_acc -> d_new, d_stats.  next: the ids the normalise launch behind this one will set the next iteration up from
// (null: none, or not known yet): after a fused step the stats_fix launch then also stages that set-up's rows
gh_status gh_launch_integrate(gh_engine *h, const gh_ids *next = nullptr);
gh_status gh_launch_spring_only(gh_engine *h, float *d_F); // F (n, LD), own rows
gh_status gh_launch_inter_to_dense(gh_engine *h, float *d_F);
gh_status gh_launch_integrate_given(gh_engine *h, const float *d_Fs, const float *d_Fi);
// d_new -> d_pos (pt.py:802-804), rows and statistics from where `kind` says (gh_make_norm_src; stats_all: GH_FINISH_OWN_ALL_STATS).
// next: also the KNN set-up of the next iteration from these ids, in the same launch (null: none)
gh_status gh_launch_normalise(gh_engine *h, gh_finish_kind kind, bool with_cleanup, const gh_ids *next = nullptr,
                              const double *stats_all = nullptr);
gh_status gh_launch_unpack_rows(gh_engine *h);   // form C: the gathered packed blocks of the OTHER ranks -> their rows of d_pos
struct gh_long_args;
gh_long_args gh_make_long_args(const gh_engine *h, bool coop_mid = false);   // common.h; coop_mid: fused kernels
gh_status gh_launch_spring_long(gh_engine *h, float *outF, int64_t f_row0);  // spring forces of the hub rows
// form D: the counter this iteration's patch list is appended through (two, used by alternate iterations: patch_rows_kernel)
// and its records; null under the other forms
inline int32_t *gh_patch_count(gh_engine *h) { return h->xch.is(GH_LAYOUT_OVERLAP) ? reinterpret_cast<int32_t *>(h->d_stats + h->xch.lay.patch_counters) + (h->iter & 1) : nullptr; }
inline float *gh_patch_records(gh_engine *h) { return h->xch.is(GH_LAYOUT_OVERLAP) ? reinterpret_cast<float *>(h->d_stats + h->xch.lay.patch_records) : nullptr; }
gh_status gh_launch_new0(gh_engine *h);                            // form D without the fused kernel: d_new = pos + Fs of the own rows
gh_status gh_launch_pack_rows(gh_engine *h, hipStream_t stream);   // form D: own block of new0 -> its packed slot (on the given stream)
gh_status gh_launch_patch_rows(gh_engine *h);                      // form D: touched rows of the gathered array += Fi; accumulators zeroed
// cg: also the sector-packed copy of the same rows (d_cg; null: none)
gh_status gh_launch_pad(gh_engine *h, const float *d_src_nD, float *d_dst_nLD, float *cg = nullptr);
gh_status gh_ensure_compact_table(gh_engine *h);   // (api.hip) d_cg exists, zeroed, where the plan asks for it; a new one is not valid
gh_status gh_launch_unpad(gh_engine *h, const float *d_src_nLD, float *d_dst_nD);
gh_status gh_launch_sample(gh_engine *h);                  // device sampler -> d_sampled
gh_status gh_launch_arange(gh_engine *h);
gh_status gh_ensure_sample(gh_engine *h);                  // run a pending stand-alone sampler launch
