/*
 * graphem_hip.h -- C ABI of the MI355X (gfx950) force-directed layout engine.
 *
 * This is the drop-in boundary for ONE path of sashakolpakov/graphem-rapids: the
 * per-iteration loop behind GraphEmbedderPyTorch.run_layout().  The reference
 * has no FFI of its own (it is 100 % Python); each entry point
 * below cites the reference method (graphem_rapids/backends/embedder_pytorch.py,
 * "pt.py") whose work it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; host pointers unless a name says "device";
 *   - every function returns a gh_status; gh_last_error() gives the message;
 *   - all work is enqueued on the handle's HIP streams; only the functions
 *     documented as blocking (copies to host, gh_sync) wait for the GPU;
 *   - a handle is not thread-safe; distinct handles are independent;
 *   - positions cross the boundary as (n, D) row-major float32, edges as
 *     (E, 2) row-major int32 with u < v in the reference's edge order
 *     (pt.py:220-245), edge ids are positions in that list.
 */
#ifndef GRAPHEM_HIP_H
#define GRAPHEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gh_engine *gh_handle;

typedef enum {
    GH_OK = 0,
    GH_ERR_INVALID = 1,     /* bad argument            -> ValueError in the Python mirror   */
    GH_ERR_RUNTIME = 2,     /* runtime failure         -> RuntimeError                      */
    GH_ERR_K_TOO_LARGE = 3, /* n_neighbors + 1 > E     -> RuntimeError (torch.topk, pt.py:583) */
    GH_ERR_HIP = 4,         /* HIP API / kernel error  -> RuntimeError                      */
    GH_ERR_NOMEM = 5        /* allocation failure      -> MemoryError                       */
} gh_status;

/* Constructor arguments of the reference that the loop reads (pt.py:51-67, 130-156). */
typedef struct {
    float L_min;          /* pt.py:57  */
    float k_attr;         /* pt.py:58  */
    float k_inter;        /* pt.py:59  */
    int32_t n_neighbors;  /* pt.py:60, k */
    int32_t sample_size;  /* pt.py:61, already min(sample_size, E) as pt.py:156 */
    uint64_t seed;        /* seed of the on-device sampler (used when no sample ids are passed) */
    int32_t reorder;      /* internal vertex order: GH_REORDER_AUTO / _OFF / _BFS (no reference counterpart) */
    int32_t knn_method;   /* GH_KNN_AUTO / _SCAN / _GRID / _IVF: how the KNN of the sampled midpoints is searched */
    int32_t knn_distance; /* GH_DIST_EXACT / GH_DIST_CDIST: which distance ranks the neighbours (below) */
    int32_t ivf_lists;    /* GH_KNN_IVF: inverted lists (0: about sqrt(own edges) / 2, at most 512 up to 4 components and 1024 above;
                             always a multiple of 64 in 64 ... 2048) */
    int32_t ivf_probes;   /* GH_KNN_IVF: lists a query searches (0: lists / 16 for more than 8 components, / 32 for 5 - 8, / 64 below;
                             < 0: exact mode, every list that can hold a neighbour) */
} gh_params;

/* Distance the KNN ranks on (pt.py:543-593).
 *   GH_DIST_EXACT  squared Euclidean distance in exact-difference form, sum_d (q_d - m_d)^2 as an fma chain in
 *                  coordinate order, ties on the smaller edge id: what the reference's KeOps path computes
 *                  (pt.py:527-534) and the fp64-correct ranking.  The speed mode; 0, so a zeroed struct selects it.
 *   GH_DIST_CDIST  the value and order the reference's PyTorch-CPU backend gets from torch.cdist + torch.topk
 *                  (pt.py:580-583): ATen's matmul form  acc = fma(-2 q_d, m_d, acc) ...; acc += |q|^2; acc += |m|^2;
 *                  sqrt(max(acc, 0))  with |x|^2 = sum of rounded squares, left to right, and equal values in the
 *                  order std::partial_sort leaves them (ATen/native/TopKImpl.h; K * 64 <= E).  The sampled edge is not
 *                  special-cased: column 0 is whatever ranks first (pt.py:417-421).  Neighbour ids then equal the
 *                  reference's row by row at every size.  The candidates of the filtered scan are re-valued with that
 *                  formula; for the rows whose K + 1 smallest values hold a tie (about 1 in 100 at a million vertices)
 *                  partial_sort's heap is replayed over the ids below a prefix bound (about E / stride of them) and the
 *                  id-sorted rest of the candidate list (csrc/cdist.hip): two more launches per iteration, 220 against
 *                  165 us at a million vertices.  Works on the candidates of GH_KNN_SCAN only: knn_method = GH_KNN_AUTO
 *                  takes the scan whatever the sample size, an explicit GH_KNN_GRID / GH_KNN_IVF is refused
 *                  (GH_ERR_INVALID).  On a row partition (gh_partition given) a rank sends, instead of its K best keys, a
 *                  record of K + 2 words per query (gh_knn_partial_cols): its K + 1 best cdist keys and 1 where it could
 *                  prove them its K + 1 best; gh_step_merge decides the queries whose merged K + 1 smallest values are
 *                  pairwise different and replays partial_sort's heap for the others -- every rank holds all positions
 *                  and the whole edge list, so every rank gets the same rows and no further collective is needed; the
 *                  replay covers the ids below a bound taken from the gathered keys (about E / world) and the gathered
 *                  keys behind it, or all edges where a rank could not prove its keys. */
#define GH_DIST_EXACT 0
#define GH_DIST_CDIST 1

/* KNN search (the reference's cdist + topk, pt.py:543-593; its cuVS backend reaches for IVF indexes,
 * embedder_cuvs.py:255-313).  SCAN and GRID return the EXACT k+1 nearest midpoints, identical ids; IVF is approximate.
 *   GH_KNN_SCAN  filtered brute-force scan fused with the spring phase: S * E pre-filter evaluations on the matrix
 *                pipe, hidden under the spring phase's gathers up to a few thousand queries;
 *   GH_KNN_GRID  n_components <= 3: a grid over the midpoints rebuilt every iteration (O(E)), then per query only the
 *                cells its threshold ball touches: sub-quadratic, pays from several thousand queries on.  (With more
 *                components the engine searches with GH_KNN_SCAN instead: a grid over the first three coordinates stays
 *                exact but was measured 50-80x slower than the scan at a million vertices; removed in round 4.)
 *   GH_KNN_IVF   2 <= n_components <= 16, GH_DIST_EXACT (a partitioned engine indexes the edges it owns): an inverted-file index rebuilt every iteration,
 *                the counterpart of the cuVS backend's IVF-Flat (embedder_cuvs.py:255-313, 384-430).  ivf_lists centroids
 *                (midpoints of evenly spaced edges), every midpoint filed under its nearest one (f16 scores on the matrix
 *                pipe), a query searches the ivf_probes lists whose centroids are nearest and gets the exact k+1 nearest
 *                AMONG THEIR MEMBERS (exact-difference distances, ties on the smaller id).  APPROXIMATE: a neighbour filed
 *                under an unprobed list is missed.  Measured on a million vertices / 4 M edges, 4096 queries, defaults
 *                (1024 lists; 64 / 32 probes): recall 0.992 in 16 dimensions (1.7 ms per iteration against 2.6 for SCAN), 1.0000
 *                in 6 (1.0 against 1.5); pays from a few thousand queries on; AUTO never takes the approximate mode.
 *                ivf_probes < 0 selects its EXACT mode: a query probes every list that can hold one of its k+1 nearest -- with
 *                tau >= the (k+1)-th smallest distance, the lists whose centroid lies within sqrt(tau) + min(list radius,
 *                sqrt(tau) + distance to the query's nearest centroid) -- and the rows are those of SCAN, id for id.  A few
 *                lists per query up to 4 components, a few dozen at 6, most of them beyond 8 (then it costs a scan plus the
 *                index).  rr1m, SCAN / exact IVF us per iteration: D = 3 S = 4096 1063 / 591, 16384 3691 / 766 (GRID 1926);
 *                D = 6 S = 4096 1507 / 915, 16384 5059 / 1401; D = 8 S = 16384 5264 / 2135; D = 16 S = 16384 8827 / 6677.
 *   GH_KNN_AUTO  exact methods only: engines with 2-8 components, GH_DIST_EXACT, >= 262144 (own) edges and thousands of
 *                queries (sample_size >= 4096 up to 4 components, >= 8192 for 5-8) take IVF in its exact mode; else GRID when
 *                n_components <= 3 and sample_size >= 12288; else SCAN. */
#define GH_KNN_AUTO 0
#define GH_KNN_SCAN 1
#define GH_KNN_GRID 2
#define GH_KNN_IVF 3

/* Internal vertex order.  The spring phase gathers the position row of every neighbour; with
 * breadth-first vertex numbers a vertex sits next to its BFS siblings and close to its parent and
 * children, so more of those gathers hit the L2; within blocks of 16384 such numbers the rows are put in
 * order of falling degree (the lanes of a wave walk their lists in lock-step).  Purely internal: vertex arrays cross the API in
 * the caller's order, edge ids are unchanged and every summation keeps the reference's order, so
 * results do not depend on it.  AUTO = BFS when the position array outgrows an L2 (n * row bytes >
 * 3 MB) and the partition (if any) uses GH_EDGES_HASHED.  gh_positions_device() exposes the
 * INTERNAL order; gh_vertex_order() returns the internal row of every vertex. */
#define GH_REORDER_AUTO 0
#define GH_REORDER_OFF 1
#define GH_REORDER_BFS 2

/* Row partition for multi-GPU runs (no reference counterpart).
 * A rank integrates vertices [row_lo, row_hi) and searches the edges it OWNS in the
 * KNN phase; it still holds all n positions and all E edges.  Every edge must be owned
 * by exactly one rank of the job:
 *   GH_EDGES_RANGE   the rank owns edges [edge_lo, edge_hi) (the caller cuts the ranges);
 *   GH_EDGES_HASHED  each edge belongs to one of its endpoints, chosen by a fixed hash of
 *                    the edge id, and so to the rank whose rows hold that endpoint: every
 *                    rank owns ~E/world edges whatever the vertex numbering.  The row
 *                    ranges of the ranks must tile [0, n); edge_lo/edge_hi are ignored.
 * Single GPU: row_lo = 0, row_hi = n, edge_lo = 0, edge_hi = E, GH_EDGES_RANGE. */
#define GH_EDGES_RANGE 0
#define GH_EDGES_HASHED 1
typedef struct {
    int64_t row_lo, row_hi;
    int64_t edge_lo, edge_hi;
    int32_t edge_rule;
} gh_partition;

/* ---- lifetime -------------------------------------------------------------- */

/* Replaces the device-side part of GraphEmbedderPyTorch.__init__ (pt.py:150-159):
 * uploads the edge list, builds the pull lists for the spring phase, allocates all
 * state.  part may be NULL (whole graph).  Positions start at zero. */
gh_status gh_create(gh_handle *out, int device_id, int64_t n, int32_t n_components, int64_t n_edges,
                    const int32_t *edges, const gh_params *params, const gh_partition *part);
void gh_destroy(gh_handle h);
/* Message of the last failure on h (h may be NULL for a failed gh_create). */
const char *gh_last_error(gh_handle h);

/* ---- float64 engine (pt.py:56: the reference computes in the dtype it is created with; tests/test_pytorch_backend.py:
 *      169-181) --------------------------------------------------------------------------------------------------
 * gh_create_f64 makes an engine whose every phase runs in double: positions (n, D) doubles, spring forces, the exact
 * KNN ranked on double distances (ties on the smaller id), intersection forces, means and unbiased std in double.
 * Plain kernels, one per phase (csrc/f64.hip): what this mode is for is the reference's fp64 numbers, not speed.
 * On such a handle: gh_set_positions / gh_get_positions convert from / to float32, the *_f64 accessors below move
 * doubles; gh_step, gh_run, gh_sync, gh_knn_midpoints, gh_destroy, gh_last_error work as on a float32 engine; every
 * other entry point (partitions, collectives, float32 per-phase calls, instrumentation of the fused kernels) returns
 * GH_ERR_INVALID.  gh_params.reorder / knn_method / knn_distance are ignored.  Up to 32 components, 255 neighbours. */
gh_status gh_create_f64(gh_handle *out, int device_id, int64_t n, int32_t n_components, int64_t n_edges,
                        const int32_t *edges, const gh_params *params /* its three float constants are NOT used: */,
                        double L_min, double k_attr, double k_inter /* pt.py:57-59 as the doubles Python holds */);
gh_status gh_set_positions_f64(gh_handle h, const double *pos /* (n, D) host */);
gh_status gh_get_positions_f64(gh_handle h, double *pos /* (n, D) host, blocking */);
double *gh_positions_device_f64(gh_handle h);                 /* (n, D) doubles, caller's vertex order, no padding */
gh_status gh_spring_forces_f64(gh_handle h, double *F);      /* _compute_spring_forces (pt.py:595-636) in double */
gh_status gh_intersection_forces_f64(gh_handle h, const int32_t *sampled, const int32_t *knn, double *F);   /* pt.py:638-774 */

/* ---- positions accessors: `positions` property / setter, get_positions
 *      (pt.py:324-335, 835-844) ------------------------------------------------ */
gh_status gh_set_positions(gh_handle h, const float *pos /* (n, D) host */);
gh_status gh_get_positions(gh_handle h, float *pos /* (n, D) host, blocking */);
/* Device view for callers that keep data on the GPU (RCCL all-gather, torch tensors):
 * (n, ld) float32 rows, ld = gh_row_stride(h) >= D floats, columns >= D are zero.
 * The caller may write the rows between steps; from this call on the engine reads no copy it keeps of them
 * (gh_set_compact_gather). */
float *gh_positions_device(gh_handle h);
/* order[v] = row of vertex v in the device position array (identity without reordering). */
gh_status gh_vertex_order(gh_handle h, int32_t *order);
/* Device copy of the positions in the CALLER's vertex order, (n, n_components) floats without
 * padding; valid until the next call on this handle. */
const float *gh_positions_unpadded_device(gh_handle h);
int32_t gh_row_stride(gh_handle h);

/* ---- the loop: update_positions / run_layout (pt.py:776-806, 808-833) ------- */

/* One iteration.  sampled: the S edge ids of this iteration (what
 * torch.randperm(E)[:S] returned, pt.py:409), host pointer; NULL = draw them on the
 * device (ignored when S >= E, where the reference uses arange(E), pt.py:412). */
gh_status gh_step(gh_handle h, const int32_t *sampled);
/* iters iterations without host synchronisation.  sample_stream: (iters, S) host ids
 * or NULL for the device sampler. */
gh_status gh_run(gh_handle h, int32_t iters, const int32_t *sample_stream);
/* The reference's own sampler beside the loop (pt.py:403-413: `torch.randperm(n_edges)[:sample_size]` on the global CPU
 * generator, once per iteration).  ATen's CPU randperm is a forward Fisher-Yates over an mt19937 (z = random() % (n - i);
 * swap(r[i], r[i + z])): entries [:S] are final after S draws, the other n - 1 - S draws only move the generator on.
 *   gh_torch_randperm_prefix  pure host code, no GPU: rng_state = the 5056 bytes of torch.get_rng_state() (in / out);
 *                             writes `iters` rows of S ids = what `iters` calls of torch.randperm(n)[:S] return, and
 *                             leaves in rng_state the state those calls leave (hand it to torch.set_rng_state).
 *                             O(S) swaps per row in a small table + an AVX2 / AVX-512 twist over the skipped words
 *                             (gh_torch_randperm_isa names the one chosen on this host).
 *   gh_run_torch_sampled      gh_run with those ids: a host thread draws them (up to 256 iterations ahead) while the calling
 *                             thread uploads what is drawn and enqueues; rng_state in / out as above (written on success only).
 *                             S >= E consumes nothing, like pt.py:412.  Whole-graph engines (float32 or float64). */
gh_status gh_torch_randperm_prefix(uint8_t *rng_state, int64_t state_bytes, int64_t n, int64_t sample_size, int32_t iters,
                                   int32_t *ids /* (iters, sample_size) host */);
const char *gh_torch_randperm_isa(void);
gh_status gh_run_torch_sampled(gh_handle h, int32_t iters, uint8_t *rng_state, int64_t state_bytes);
/* Host milliseconds of the last gh_run_torch_sampled on h: [0] the producer thread drawing, [1] the calling thread
 * waiting for a pinned upload slot to come back from the GPU, [2] the calling thread waiting for ids, [3] the whole call
 * (enqueue only). */
gh_status gh_sampler_stats(gh_handle h, double *out4);
/* Blocks until everything enqueued on h has finished. */
gh_status gh_sync(gh_handle h);

/* ---- per-phase entry points (tests, profiling).  Each runs on the CURRENT
 *      positions, leaves them unchanged, blocks, and writes host buffers. -------- */

/* _compute_spring_forces (pt.py:595-636): F (n, D). */
gh_status gh_spring_forces(gh_handle h, float *F);
/* _locate_knn_midpoints + _compute_knn_chunked/_compute_knn_torch (pt.py:381-424,
 * 426-483, 543-593): knn (S, k) edge ids, column 0 already dropped (pt.py:421). */
gh_status gh_knn_midpoints(gh_handle h, const int32_t *sampled, int32_t *knn);
/* _compute_intersection_forces + _check_line_intersections (pt.py:638-774): F (n, D). */
gh_status gh_intersection_forces(gh_handle h, const int32_t *sampled, const int32_t *knn, float *F);
/* combine + normalise (pt.py:796-804): out = normalise(pos + (Fs + Fi)); (n, D) each. */
gh_status gh_integrate_normalise(gh_handle h, const float *Fs, const float *Fi, float *out);

/* ---- multi-GPU hooks.  With a gh_partition a step is split so the
 *      caller can run its collectives (RCCL through torch.distributed) between the
 *      parts; all buffers are device pointers owned by the handle. ---------------- */

/* Run all later work of h on the caller's HIP stream (e.g. torch's current stream, so the
 * engine's kernels are stream-ordered with RCCL collectives).  hip_stream may be NULL, which
 * is HIP's default (null) stream -- torch's default stream.  use_own != 0 switches back to the
 * stream gh_create made and ignores hip_stream. */
gh_status gh_set_stream(gh_handle h, void *hip_stream, int32_t use_own);
/* Rows allocated in the device position array: >= n, padded so that world equal chunks of
 * ceil(n / world) rows fit for an in-place all-gather (rows >= n are zero and never read). */
int64_t gh_positions_rows_allocated(gh_handle h);

/* Part 1: spring pull for own rows, KNN scan of own edges.  Afterwards
 * gh_knn_partial_device() holds this rank's S x (k+1) best (dist2, id) keys. */
gh_status gh_step_begin(gh_handle h, const int32_t *sampled);
uint64_t *gh_knn_partial_device(gh_handle h);      /* (S, gh_knn_partial_cols) uint64: k+1 keys, ascending */
/* 64-bit words per query of that record: k + 1; a GH_DIST_CDIST engine on a partition: k + 3 (its k + 2 best cdist keys,
 * then 1 where they are provably its k + 2 best).  gathered of gh_step_merge is (world, S, gh_knn_partial_cols). */
int32_t gh_knn_partial_cols(gh_handle h);
/* After gh_step_merge: the (S, k+1) keys of the global KNN the intersection phase read (column 0 included; the id of a
 * neighbour is the low 32 bits of its key).  Device pointer owned by the handle; NULL before the first merge. */
const uint64_t *gh_knn_merged_device(gh_handle h);
/* Part 2: gathered = (world, S, k+1) keys from all ranks (device pointer; may alias a
 * caller buffer).  Merges them, computes intersection forces, integrates own rows and
 * leaves this rank's column sums in gh_stats_partial_device(). */
gh_status gh_step_merge(gh_handle h, const uint64_t *gathered, int32_t world);
double *gh_stats_partial_device(gh_handle h);      /* (gh_stats_rows, ld) doubles, to be summed elementwise over ranks */
int32_t gh_stats_rows(gh_handle h);
/* Part 3, form A: after the caller all-reduced (SUM) the whole statistics buffer: normalise own rows in place in the
 * full position array; the caller then all-gathers the row blocks (two collectives). */
gh_status gh_step_finish(gh_handle h);

/* Part 3, form B (ONE collective): the rank's un-normalised new rows and its statistics live side by side in
 * one slot of a gather buffer; the caller all-gathers the slots in place and every rank then normalises ALL n
 * rows from the gathered slots, summing the per-rank statistics in rank order (identical on every rank).
 *   gh_gather_layout(h, world, rank, chunk)  once after gh_create: this rank is `rank` of `world`, rank r owns
 *                                             rows [r*chunk, min(n, (r+1)*chunk)); allocates the buffer
 *   gh_gather_buffer_device(h)               world * gh_gather_slot_bytes(h) bytes; slot r belongs to rank r
 *   gh_step_finish_gathered(h)               after the all-gather: d_pos <- normalised rows of every rank */
gh_status gh_gather_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk);
void *gh_gather_buffer_device(gh_handle h);
int64_t gh_gather_slot_bytes(gh_handle h);
gh_status gh_step_finish_gathered(gh_handle h);

/* Part 3, form C (the default of the drivers; no pass over all n rows): the rank keeps its un-normalised rows to itself,
 * the caller all-gathers only the ranks' STATISTICS (gh_stats_rows * ld doubles each, rank order), every rank
 * normalises ITS rows into its block of the position array -- per-rank sums added in rank order, so all ranks use the
 * same mean / std bits -- and the caller then all-gathers the finished blocks IN PLACE in gh_positions_device():
 * block r = rows [r*chunk, (r+1)*chunk), chunk * ld floats (gh_positions_rows_allocated() >= world * chunk).
 *   gh_rank_layout(h, world, rank, chunk)   once after gh_create (instead of gh_gather_layout)
 *   gh_step_finish_own(h, stats_all, world) stats_all: (world, gh_stats_rows, ld) doubles, device
 * The position array is complete again only after the caller's all-gather.
 * With fewer components than the row stride (3 of 4, 5..7 of 8, 9..15 of 16) and world > 1 the blocks can travel WITHOUT
 * their pad columns (12 instead of 16 bytes per row at 3 components: a quarter off the largest collective of the iteration):
 * gh_step_finish_own also writes the own block into slot `rank` of gh_rows_packed_device(), a (world, chunk, D) float
 * array; the caller all-gathers THAT in place instead of the position blocks and calls gh_step_unpack_rows, which expands
 * the other ranks' blocks into the position array.  The expansion is a kernel over all n rows (30 us at 4 M vertices, 14 at
 * 1 M, measured), so the packed exchange is in use by default from 2 M vertices on; gh_set_packed_rows switches it on or
 * off after gh_rank_layout.  gh_rows_packed_device() is NULL while it is not in use (D == ld, world == 1, switched off):
 * the caller then all-gathers the position blocks in place. */
gh_status gh_rank_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk);
/* Part 3, form D (round 5; the default of bench.py --gpus N and of distributed.PartitionedLayout): form B's finish -- every
 * rank normalises ALL n rows from the ranks' gathered un-normalised rows, no collective after the normalisation -- with the
 * big collective moved to the FRONT of the KNN tail.  Part 1 leaves new0 = pos + Fs of the own rows in block `rank` of a
 * (world, chunk, ld) array (the fused spring+scan kernel writes it; a rank too small for that kernel makes it with a launch
 * of its own, so every rank sends at the same point: gh_step_rows_early() is 1 after every gh_step_begin); the caller
 * starts the all-gather of those blocks at once, on a second stream / communicator, and runs select -> all-gather of the
 * keys -> gh_step_merge -> all-gather of the statistics beside it.  Only the <= 4 S k rows the intersection phase touches
 * differ from new0 afterwards: gh_step_merge puts the finished value of every OWN touched row -- pos + (Fs + Fi), the single
 * engine's expression -- into the rank's PATCH LIST, which sits behind its statistics and travels with them.
 * gh_step_finish_overlap (enqueued behind BOTH collectives) writes every rank's patch list over those rows of the gathered
 * array and normalises all n rows into the position array (the next iteration's KNN set-up rides in that launch).  Results:
 * what forms B / C give (the single engine's up to the order in which the ranks' statistics are added).  What travels:
 *   gh_rows_all_device()      (world, chunk, gh_rows_all_row_floats()) floats, block r = rank r's rows: WITHOUT pad columns
 *                             when n_components < ld and world > 1 (row_floats = n_components; the own block is put there
 *                             by gh_step_pack_rows on the stream given -- call it on the side stream before the all-gather;
 *                             a no-op otherwise), else the (world, chunk, ld) array itself;
 *   gh_stats_all_device()     (world, gh_stats_all_block_doubles()) doubles, block r = rank r's statistics rows
 *                             (= gh_stats_partial_device(), gh_stats_rows * ld doubles), then 16 bytes holding its two patch
 *                             counters (int32; iteration t uses counter t & 1, the other is zeroed meanwhile) and
 *                             min(4 S k, chunk) records of (row as int32, ld floats).
 * Up to 16 components. */
gh_status gh_overlap_layout(gh_handle h, int32_t world, int32_t rank, int64_t chunk);
float *gh_rows_all_device(gh_handle h);
int32_t gh_rows_all_row_floats(gh_handle h);
double *gh_stats_all_device(gh_handle h);
int64_t gh_stats_all_block_doubles(gh_handle h);
int32_t gh_step_rows_early(gh_handle h);
gh_status gh_step_pack_rows(gh_handle h, void *hip_stream, int32_t use_engine_stream);
gh_status gh_step_finish_overlap(gh_handle h);
gh_status gh_step_finish_own(gh_handle h, const double *stats_all, int32_t world);
gh_status gh_set_packed_rows(gh_handle h, int32_t on);
float *gh_rows_packed_device(gh_handle h);
gh_status gh_step_unpack_rows(gh_handle h);

/* ---- the whole partitioned run as ONE call (no host language in the loop) ----------------------
 * After gh_create(partition) + gh_rank_layout(world, rank, chunk) (form C: all-gathers of the keys, of the statistics
 * and, in place, of the finished position blocks) or gh_gather_layout (form B: keys, slots) + one of the communicator
 * calls, gh_run_partitioned enqueues `iters` iterations on the handle's stream; only the collective backend may block.
 * Every rank must call it with the same iters and the same sample_stream ((iters, S) host ids, or NULL:
 * each rank's engine then draws identical ids from (seed, iteration)).
 *   gh_comm_unique_id        rank 0: 128 bytes to hand to every rank (ncclGetUniqueId)
 *   gh_comm_init_rccl        RCCL communicator on the engine's device; collectives = ncclAllGather on the engine's
 *                            stream over xGMI.  librccl.so is opened here, not at load time.
 *   gh_loopback_group_create / gh_comm_init_loopback
 *                            `world` engines of one process, one host thread each, exchange by device copies:
 *                            the same loop on a single GPU (where RCCL refuses two ranks on one device)
 * After gh_overlap_layout (form D) the communicator call also makes the side stream and, with RCCL, a second communicator
 * (ncclCommSplit) for the early all-gather of the rows; without one the rows go out after the merge (form B's order).
 * Kernel and collective times appear under gh_timing_get as "allgather_keys" / "allgather_slots" / "allgather_rows" (form
 * D: measured on the side stream) / "allgather_rows_exposed" (form D: how long the engine's stream then still waited). */
typedef struct gh_loop_group gh_loop_group;
int32_t gh_comm_available(void);         /* 1 when librccl.so opens and has every entry point used here (no communicator made) */
gh_status gh_comm_unique_id(void *out128);
gh_status gh_comm_init_rccl(gh_handle h, int32_t world, int32_t rank, const void *unique_id128);
gh_loop_group *gh_loopback_group_create(int32_t world);
void gh_loopback_group_destroy(gh_loop_group *group);
gh_status gh_comm_init_loopback(gh_handle h, gh_loop_group *group, int32_t rank);
gh_status gh_comm_destroy(gh_handle h);
gh_status gh_run_partitioned(gh_handle h, int32_t iters, const int32_t *sample_stream);
const char *gh_comm_last_error(void);   /* message of a failed gh_comm_unique_id */

/* ---- instrumentation --------------------------------------------------------- */

/* Names and accumulated GPU milliseconds of the kernels launched since the last
 * reset, measured with HIP events on the launching stream when timing is enabled. */
gh_status gh_timing_enable(gh_handle h, int32_t on);
gh_status gh_timing_reset(gh_handle h);
int32_t gh_timing_count(gh_handle h);
gh_status gh_timing_get(gh_handle h, int32_t i, const char **name, double *total_ms, int64_t *launches);

/* Environment variables the library reads -- diagnostics only, all of them at gh_create, none needed in production:
 *   GRAPHEM_HIP_TAU_SEPARATE=1|0  thresholds always in a launch of their own / always by the first workgroups of the fused
 *                                 launch (default: inside for <= 2048 fused workgroups);
 *   GRAPHEM_HIP_COARSE_TAU=1|0    GH_COARSE_ON | GH_COARSE_OFF instead of GH_COARSE_AUTO (gh_set_coarse_tau);
 *   GRAPHEM_HIP_COMPACT_GATHER=1|0  GH_COMPACT_ON | GH_COMPACT_OFF instead of GH_COMPACT_AUTO (gh_set_compact_gather);
 *   GRAPHEM_HIP_NO_PRESETUP=1     the next iteration's KNN set-up as a launch of its own instead of inside the normalise
 *                                 launch (the per-query flags of gh_knn_last_counts then survive a step);
 *   GRAPHEM_HIP_REORDER=1|2       overrides gh_params.reorder (1 off, 2 breadth-first);
 *   GRAPHEM_HIP_STAMPS=1          allocates the stamp buffer gh_debug_stamps reads. */

/* Diagnostic runs only (environment GRAPHEM_HIP_STAMPS set at gh_create): 8 wall-clock stamps (100 MHz) per workgroup
 * of the last fused spring+scan launch (tools/stamp_probe.py).  Blocking. */
gh_status gh_debug_stamps(gh_handle h, unsigned long long *out, int64_t count);

/* Diagnostics of the last KNN search: per query, the candidate-list length the last subset
 * level and the final level saw, and whether the exact fallback had to redo the query
 * (any of the three (S,) host pointers may be NULL).  Blocking. */
gh_status gh_knn_last_counts(gh_handle h, int32_t *subset_counts, int32_t *final_counts, int32_t *overflow);
/* GH_DIST_CDIST engines, last KNN search: rows whose partial_sort heap was replayed (a tie among their K + 1 smallest
 * cdist values, or a candidate list that could not be proven complete), and rows NOT reproduced.  Tiny graphs
 * (K * 64 > E), where ATen ranks with std::nth_element + std::sort, get libstdc++'s introselect and introsort replayed on
 * single-engine runs (a row partition's merge replays the heap for them: equal values in (value, id) order, counted)
 * (E <= 8000: tie order reproduced; the second count then only holds rows whose introselect depth limit ran out, which
 * adversarial inputs alone do); with K * 64 > E > 8000 (more than 125 neighbours on a graph of a few thousand edges)
 * equal values come out in (value, id) order and a row with a tie is counted.  Either pointer may be NULL.  Blocking. */
gh_status gh_knn_cdist_stats(gh_handle h, int32_t *full_pass_rows, int32_t *unresolved_tie_rows);
/* GH_DIST_CDIST engines: which ties the LOOP (gh_step / gh_run / gh_run_torch_sampled) replays.  The intersection phase
 * reads a neighbour row as a set of pairs (column 0 dropped, pt.py:417-421; the other k ids paired with the sampled edge,
 * pt.py:668-699), so only a tie between values 0 and 1 (which id is dropped) or between values k and k + 1 (which id is a
 * member) can change a force; a tie strictly inside permutes columns of the same set.  all_ties = 0 (default): the loop
 * replays partial_sort's heap for those two kinds of tie only -- same positions, bit for bit, as with all_ties = 1 (every
 * tie, rows column for column: what gh_knn_midpoints always does, and what row-partitioned engines always do). */
gh_status gh_set_cdist_replay(gh_handle h, int32_t all_ties);
/* The pre-filter of the fused spring+scan kernel for n_components <= 3 -- which (query, midpoint) pairs reach the exact
 * fp32 test d2 <= tau; the candidates, and so the neighbour rows and positions, are the same bit for bit either way.
 *   GH_FILTER_CELLS  a table of the sampled midpoints' query balls over a quantile grid of 8 cells per axis, built once
 *                    per iteration on the device; a midpoint tests the queries listed in its cell (and those whose ball
 *                    spans many cells).  Needs a fused engine with 1 <= sample_size <= 256; the thresholds then have
 *                    a launch of their own.
 *   GH_FILTER_MFMA   every pair through the split-f16 matrix-pipe screen.
 *   GH_FILTER_AUTO   (default) CELLS where the engine would compute the thresholds in a launch of their own anyway
 *                    (graphs of more than 2048 fused workgroups of 512 owned edges), else MFMA.
 * Forcing CELLS where it cannot serve is refused.  gh_get_scan_filter reports the filter in use: GH_FILTER_CELLS or
 * GH_FILTER_MFMA, or GH_FILTER_AUTO when the engine runs neither (another dimension, an unfused or a float64 engine). */
#define GH_FILTER_AUTO 0
#define GH_FILTER_MFMA 1
#define GH_FILTER_CELLS 2
gh_status gh_set_scan_filter(gh_handle h, int32_t mode);
gh_status gh_get_scan_filter(gh_handle h, int32_t *mode);
/* Where the thresholds of a GH_FILTER_CELLS engine come from (whole-graph engines, n_neighbors + 1 -- + 2 with
 * GH_DIST_CDIST -- up to 32; results are the same bit for bit either way):
 *   GH_COARSE_ON    the set-up reduces each query's subset distances to 64 coarse group minima and the first workgroup
 *                   of the fused launch takes their K-th smallest itself: no threshold launch.  Also on graphs that AUTO
 *                   would give embedded thresholds, once gh_set_scan_filter(GH_FILTER_CELLS) is in force.
 *   GH_COARSE_OFF   group minima of 64 subset edges and a threshold launch of their own.
 *   GH_COARSE_AUTO  (default; GRAPHEM_HIP_COARSE_TAU=1|0 at creation sets ON | OFF) ON for three components and up to 12 keys,
 *                   where it was measured ahead (1 M vertices: 153.8 -> 149.9 us per iteration), else OFF.
 * Forcing ON where it cannot serve is not an error: gh_get_coarse_tau reports what is in use, 1 or 0. */
#define GH_COARSE_AUTO 0
#define GH_COARSE_OFF 1
#define GH_COARSE_ON 2
gh_status gh_set_coarse_tau(gh_handle h, int32_t mode);
gh_status gh_get_coarse_tau(gh_handle h, int32_t *in_use);
/* Both copies of the coarse table, (2, 64, sample_size) float bits, 0xFFFFFFFF = empty (diagnostic; count words).  Blocking. */
gh_status gh_debug_coarse_table(gh_handle h, uint32_t *out, int64_t count);
/* Where the fused spring+scan kernel of a three-component engine takes position rows from (its own rows and the rows it
 * gathers; same values, so the same results bit for bit either way):
 *   GH_COMPACT_ON    a second table of 12-byte rows, five to a 64-byte sector (no row crosses a sector), written beside the
 *                    positions by the launches that write them.  Whole-graph single-rank fused engines with n_components
 *                    = 3 only; a step that finds the table out of date (the positions were changed by another entry
 *                    point) reads the padded positions and the next finish brings it up to date.  Once
 *                    gh_positions_device has handed the rows out the table is not read again: the caller may write them
 *                    between any two steps.
 *   GH_COMPACT_OFF   the padded 16-byte rows of gh_positions_device.
 *   GH_COMPACT_AUTO  (default; GRAPHEM_HIP_COMPACT_GATHER=1|0 at creation sets ON | OFF) ON where it was measured ahead.
 * Forcing ON where it cannot serve is not an error: gh_get_compact_gather reports what is in use, 1 or 0 (0 also once the
 * rows were handed out), and gh_compact_gather_launches how many fused launches of this engine have read the table so far
 * (a step that found it out of date does not count). */
#define GH_COMPACT_OFF 0
#define GH_COMPACT_ON 1
#define GH_COMPACT_AUTO 2
gh_status gh_set_compact_gather(gh_handle h, int32_t mode);
gh_status gh_get_compact_gather(gh_handle h, int32_t *in_use);
gh_status gh_compact_gather_launches(gh_handle h, int64_t *packed);
/* The layout of that table on the host (test support): the dword offset of vertex v's row -- of the count vertices from v0
 * on into out[] -- and the bytes a table for n vertices takes. */
int64_t gh_compact_slot(int64_t v);
gh_status gh_compact_slots(int64_t v0, int64_t count, int64_t *out);
int64_t gh_compact_bytes(int64_t n);
/* Host copy of the query-cell box (test support): for each of n (q, tau, m) triples of D <= 3 coordinates -- boundaries
 * (D, 7) per axis -- writes the fp32 chain d2(q, m) of the exact test to d2[i], and per axis the cell of m and q's box
 * [lo, hi] to cells[(i * D + d) * 3 + {0, 1, 2}]. */
gh_status gh_qcell_probe(const float *bounds, int32_t D, const float *q, const float *tau, const float *m, int64_t n,
                         float *d2, int32_t *cells);
/* GH_KNN_IVF engines: the number of inverted lists and of lists probed per query the engine settled on (0, 0 when the
 * engine searches another way).  Either pointer may be NULL. */
gh_status gh_knn_ivf_config(gh_handle h, int32_t *lists, int32_t *probes);
/* Members of every inverted list after the last search (diagnostic; count must equal the number of lists).  Blocking. */
gh_status gh_knn_ivf_list_sizes(gh_handle h, int32_t *sizes, int32_t count);

/* Plain point-set KNN without a handle: the reference's _compute_knn_chunked /
 * _compute_knn_torch (pt.py:426-483, 543-593).  q (nq, D), ref (nref, D) host float32 row-major;
 * out (nq, k) int64: ids of the k nearest reference rows, ascending distance (exact squared
 * Euclidean distance, ties on the smaller id).  k > nref -> GH_ERR_K_TOO_LARGE like torch.topk.
 * On failure gh_last_error(NULL) has the message.  Blocking. */
gh_status gh_knn_points(int device_id, const float *q, int64_t nq, const float *ref, int64_t nref,
                        int32_t n_components, int32_t k, int64_t *out);

/* ---- caller-side reduction on the device (influence.py:28-37) ----
 * The k vertices farthest from the origin, farthest first: np.argsort(-np.linalg.norm(positions,
 * axis=1))[:k] of the reference's graphem_seed_selection without the (n, D) device-to-host copy.
 * Radial distance = sqrtf of the sum of squares accumulated in coordinate order with separate
 * multiply and add: numpy's own order for rows shorter than 8 (longer rows it sums pairwise, so the
 * last bit -- and with it only the order of near-ties -- may differ); equal distances -> smaller
 * vertex id first (numpy's unstable sort leaves that order open).  ids: k host int32.  1 <= k <= min(n, 64).
 * Blocking. */
gh_status gh_radial_topk(gh_handle h, int32_t k, int32_t *ids);

/* ---- spectral initialisation (_compute_laplacian_embedding, pt.py:337-379) ----
 * y = (2I - L) x for the normalised Laplacian L of a symmetric, unweighted graph in CSR form:
 * y_i = x_i + s_i * sum_j s_j x_j over the neighbours j of i (s = degree^-1/2), y_i = 2 x_i for an
 * isolated vertex.  The operator of the Lanczos iteration in graphem-rapids_amd/spectral.py.
 * All pointers are DEVICE pointers; fp64; asynchronous on hip_stream (NULL = default stream).
 * gh_spectral_last_error() has the message of a failed call. */
gh_status gh_spmv_symnorm(void *hip_stream, int64_t n, const int64_t *indptr, const int32_t *indices,
                          const double *inv_sqrt_deg, const double *x, double *y);
/* Steps k .. m-1 of a Lanczos sweep on B (thick-restart form: the first k columns of the projected matrix are given):
 * matvec, classical Gram-Schmidt twice against the nl locked vectors and the basis so far, coefficients into column j of
 * Td, beta[j] = |w|, hmax[j] = max |coefficient|, next basis vector -- seven launches per step on hip_stream, no host
 * synchronisation.  V (nl + m + 1, n), Td (m, m) row-major, work: n + 2 (nl + m + 1) + ceil(n / 512) (nl + m + 1)
 * doubles, beta / hmax (m); all DEVICE pointers; nl + m + 1 <= 256.
 * Layout of work, with R = nl + j + 1 and as the LAST step j of the call left it: w at 0 (n doubles: B V[nl + j] after
 * both passes, before the division by beta[j]); h1 at n (the R coefficients of the first pass, row by row of V); h2 at
 * n + (nl + m + 1) (those of the second pass, taken on w after the first); the chunk partials from n + 2 (nl + m + 1)
 * on.  Td[r - nl][j] = h1[r] + h2[r] for nl <= r < R; no other entry of Td, beta or hmax is written, nor any row of V
 * but nl + j + 1.  k == m is an empty sweep: GH_OK, nothing written. */
gh_status gh_trlan_sweep(void *hip_stream, int64_t n, const int64_t *indptr, const int32_t *indices,
                         const double *inv_sqrt_deg, double *V, int32_t nl, int32_t m, int32_t k, double *Td,
                         double *work, double *beta, double *hmax);
const char *gh_spectral_last_error(void);

/* Self-test (no reference counterpart): the spring phase computes sqrt and its D divisions by one distance with leaner
 * instruction sequences than the compiler's general ones; this compares them bit for bit with sqrtf and '/' on `samples`
 * pseudo-random operand sets over and beyond their fast domain.  Both counts must come back 0.  Blocking. */
gh_status gh_selftest_arith(int device_id, uint64_t seed, int64_t samples, int64_t *bad_sqrt, int64_t *bad_div);

/* ---- influence: Monte Carlo Independent Cascade (reference influence.py: ndlib_estimated_influence,
 * greedy_seed_selection; graphem-rapids_amd/influence.py) -------------------------------------------------
 * A handle over one graph, independent of the layout engine.
 *
 * Independent Cascade: round 0 activates the seed set; in round r every vertex activated in round r-1 tries each
 * inactive neighbour once and succeeds with probability p.  A vertex's hop distance is the round it was activated in.
 * spread = number of vertices with hop distance <= max_hops (max_hops = -1: no limit).
 *
 * Coins are counter-based, so every result can be recomputed bit for bit on the host.  In trial t (0 <= t < n_trials)
 * the arc pair (a, b) is live iff  coin(seed, t, a, b) < thr,  with uint64 wrapping arithmetic:
 *     mix(z):  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
 *     coin   = mix( mix(seed + t * 0x9E3779B97F4A7C15) ^ ((uint64)a << 32 | b) ) >> 40             (24 bits)
 *     thr    = min(2^24, floor(p * 2^24 + 0.5))                                                      (double, once)
 * (a, b) = (min(u, v), max(u, v)) for an undirected graph -- both directions share one coin; a cascade tries an
 * undirected edge at most once, so by deferred decisions the reached set and every hop distance have the distribution
 * of a separate coin per direction -- and (u, v) per arc u -> v for a directed graph.  The reached set of trial t is
 * exactly the breadth-first search over the live arcs from the seeds, cut at max_hops.  Results therefore depend only on
 * (arc set, seed set, p, max_hops, n_trials, seed): not on arc order, duplicate arcs, self-loops, how trials are packed,
 * how seed sets are batched or chunked.
 *
 * Per-arc probabilities (gh_ic_set_arc_probabilities, gh_ic_spread_arcs, gh_ic_rr_sample_arcs): arc u -> v has its own
 * probability p_uv in [0, 1] and its own threshold, computed once on the host in double:
 *     thr_uv = min(2^24, floor(p_uv * 2^24 + 0.5))
 * In trial t the arc u -> v is live iff  coin(seed, t, a, b) < thr_uv.  coin, mix and the key (a, b) are unchanged: (u, v)
 * for a directed graph, (min, max) for an undirected one, whose two directions therefore share a coin but may have
 * different thresholds.  Trial t so defines ONE live digraph; a cascade is the breadth-first search over it from the
 * seeds, cut at max_hops, and an RR set is the search over it backwards from the root.  Two consequences:
 *   1. One forward (or one backward) search looks at an undirected edge in at most one direction -- from the endpoint it
 *      reaches first -- so by deferred decisions its result has the distribution of independent coins per direction, as
 *      argued above for the uniform p.
 *   2. The identity  sum over all roots r of [S meets RR(t, r)] = |R_t(S)|  (RIS section) holds exactly, because both
 *      searches walk the same live digraph.
 * Results depend only on (arc set, probability table, seed set or samples, max_hops, n_trials, seed).  The table is graph
 * state on the device, 4 bytes per CSR slot in each of two arrays (a slot per arc and array for a directed graph, two
 * slots per edge and array for an undirected one); gh_ic_set_memory_budget does not count it.
 *
 * Linear Threshold (gh_ic_set_lt_weights, gh_ic_spread_lt, gh_ic_rr_sample_lt; Kempe, Kleinberg, Tardos 2003), in its
 * live-edge form.  Every vertex v has weights w_uv >= 0 on its in-arcs with  sum over u of w_uv <= 1.  In one trial v
 * selects AT MOST ONE in-arc: arc u -> v with probability w_uv, none with probability 1 - sum w_uv, independently across
 * vertices.  The selected arcs are the live digraph of the trial; a cascade is the breadth-first search over it from the
 * seeds, cut at max_hops, and an RR set is the search over it backwards from the root.  By Kempe et al., Claim 2.6 (an
 * induction over rounds), the active set after every round of the threshold process -- theta_v uniform on [0, 1], v
 * becomes active once the weights of its active in-neighbours reach theta_v -- has the distribution of the set reached
 * within that many hops over the live arcs: max_hops counts rounds, as for Independent Cascade.
 *     pick(seed, t, v) = mix( mix(seed + t * 0x9E3779B97F4A7C15) ^ ((uint64)v << 32 | v) ) >> 32           (32 bits)
 * The key (v, v) is a self-loop key: no arc coin has it (self-loops are dropped), and it is not the all-ones root key.
 * Intervals, computed once on the host in double: the in-arcs of v in ascending source id, after self-loops and
 * duplicates went; an arc that is not listed has weight 0;
 *     S_k = the sequential double sum of the first k weights,  c_0 = 0,  c_k = min(2^32 - 1, floor(S_k * 2^32 + 0.5))
 * as uint32.  The k-th in-arc of v is live in trial t iff  c_{k-1} <= pick(seed, t, v) < c_k.  S is monotone, so c is: the
 * intervals are disjoint, and a zero-weight arc has an empty one.  Because of the clamp a vertex whose weights sum to 1
 * selects nobody with probability 2^-32.
 * A row may sum to at most 1 + 2^-20.  The margin is derived: a sequential sum of d <= 2^31 doubles has a relative error
 * of at most d * 2^-53 <= 2^-22, so a row whose exact sum is 1 (d copies of fl(1 / d)) always passes, and the clamp
 * absorbs the excess.
 * Undirected graphs: the edge {a, b} is the two arcs a -> b and b -> a, each in its own target's row with its own weight
 * and selected by its own target's pick.  Nothing is shared between the two -- unlike the Independent Cascade coin, which
 * the two directions of an edge share.
 * The identity  sum over all roots r of [S meets RR(t, r)] = |R_t(S)|  holds exactly (one digraph, two searches), and
 * under fixed picks the spread is reachability in a fixed digraph, so it is monotone and submodular.
 * Results depend only on (arc set, weight table, seed set or samples, max_hops, n_trials, seed): not on arc order,
 * duplicates, loops, batching, chunking or either memory budget.  The table is graph state of its own beside the per-arc
 * table -- a handle may hold both, and setting one never touches the other or the scalar p: the pair (c_{k-1}, c_k) of
 * every CSR slot in each of two arrays, 8 bytes per slot and array (16 bytes per arc of a directed graph, 32 per edge of
 * an undirected one), so that no launch looks into another vertex's row; gh_ic_set_memory_budget does not count it. */
typedef struct gh_ic *gh_ic_handle;

/* arcs: (n_arcs, 2) int32 host array, vertex ids in [0, n).  directed = 0: each row is an undirected edge.  Self-loops
 * are dropped and duplicates merged; the CSR of arcs by target (and, for a directed graph, by source) is uploaded.
 * On failure *out = NULL and gh_ic_last_error(NULL) has the message. */
gh_status gh_ic_create(gh_ic_handle *out, int device_id, int64_t n, int64_t n_arcs, const int32_t *arcs, int32_t directed);
void gh_ic_destroy(gh_ic_handle h);
const char *gh_ic_last_error(gh_ic_handle h);
/* Arcs after self-loops and duplicates went (an undirected edge counts once). */
int64_t gh_ic_arc_count(gh_ic_handle h);
/* Device bytes of chunk state gh_ic_spread may hold: n * (24 * ceil(n_trials / 64) + 17) bytes per seed set evaluated
 * at once, at least one set.  0 restores the default, 1 GiB.  Results do not depend on it. */
gh_status gh_ic_set_memory_budget(gh_ic_handle h, int64_t bytes);
/* Evaluates n_sets seed sets with the same coins: set s = set_vertices[set_offsets[s] .. set_offsets[s + 1]) (duplicates
 * allowed, may be empty).  totals[s] = sum over the n_trials trials of the spread (host int64, n_sets); per_trial (NULL
 * or host int32 (n_sets, n_trials)) = the spread of every trial.  With n_base > 0 both hold the MARGINAL spread
 * |R(base + set)| - |R(base)| of each trial instead.  GH_ERR_INVALID for p outside [0, 1], n_trials < 1,
 * max_hops < -1, a vertex id outside [0, n), decreasing offsets.  Blocking. */
gh_status gh_ic_spread(gh_ic_handle h, double p, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                       const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base, int64_t n_base,
                       int64_t *totals, int32_t *per_trial);
/* The handle's per-arc table: arcs is an (m, 2) int32 host array of DIRECTED pairs u -> v, prob[i] the probability of
 * pair i.  For an undirected graph (u, v) and (v, u) are the two directions of one edge; each may be listed once.  An arc
 * of the graph that is not listed gets threshold 0.  GH_ERR_INVALID, with the pair in gh_ic_last_error(h), for a pair
 * that is not an arc of the graph, a pair listed twice, a probability that is NaN or outside [0, 1].  A call replaces
 * the previous table; a failed call leaves it in place.  Calls with a scalar p are not affected by it.  Blocking. */
gh_status gh_ic_set_arc_probabilities(gh_ic_handle h, int64_t m, const int32_t *arcs, const double *prob);
/* gh_ic_spread with the table in place of p: the same arguments, checks, chunking and budget.  GH_ERR_INVALID when no
 * table has been set. */
gh_status gh_ic_spread_arcs(gh_ic_handle h, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                            const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base, int64_t n_base,
                            int64_t *totals, int32_t *per_trial);
/* The handle's Linear Threshold table: arcs is an (m, 2) int32 host array of DIRECTED pairs u -> v, weight[i] = w_uv of
 * pair i.  For an undirected graph (u, v) and (v, u) are two arcs; each may be listed once.  An arc of the graph that is
 * not listed gets weight 0.  GH_ERR_INVALID, with the target vertex in gh_ic_last_error(h), for a pair that is not an arc
 * of the graph, a pair listed twice, a weight that is NaN or outside [0, 1], a row whose sequential sum is above
 * 1 + 2^-20.  A call replaces the previous Linear Threshold table; a failed call leaves it in place.  The per-arc
 * probability table and calls with a scalar p are not affected.  Blocking. */
gh_status gh_ic_set_lt_weights(gh_ic_handle h, int64_t m, const int32_t *arcs, const double *weight);
/* gh_ic_spread under Linear Threshold with the table above: the same arguments, checks, chunking, marginal mode and
 * budget.  GH_ERR_INVALID when no Linear Threshold table has been set. */
gh_status gh_ic_spread_lt(gh_ic_handle h, int32_t max_hops, int32_t n_trials, uint64_t seed, int64_t n_sets,
                          const int64_t *set_offsets, const int32_t *set_vertices, const int32_t *base, int64_t n_base,
                          int64_t *totals, int32_t *per_trial);

/* ---- reverse influence sampling (RIS; Borgs et al. 2014, TIM/IMM, OPIM-C; graphem-rapids_amd/influence.py) --------------
 * A collection of reverse-reachable (RR) sets on the device behind its own handle, drawn by a gh_ic handle with the coins
 * above.  Sample j of a collection is the pair (trial t_j, root r_j).
 *
 * RR set: RR(t, r) is the set of vertices u from which r is reached over the live arcs of trial t within max_hops hops
 * (-1: no limit): a breadth-first search from r that walks every arc u -> v backwards, with the unchanged
 * coin(seed, t, a, b) of that arc -- (a, b) = (u, v) for a directed arc u -> v, (min, max) for an undirected edge.  r
 * always belongs to its set; members are reported in ascending id.
 * Default root: from the trial's own word with a key no arc can have (all ones would be a self-loop on vertex 2^32 - 1,
 * and self-loops are dropped):
 *     w = mix( mix(seed + t * 0x9E3779B97F4A7C15) ^ 0xFFFFFFFFFFFFFFFF ),   r = ((w >> 32) * n) >> 32
 * Default trials: the trial of a sample is its index in the collection, so an empty collection gets 0 .. theta - 1 and
 * appending continues the sequence.  A caller may pass explicit trials (uint64) and / or roots (int32) instead.
 * Maximum coverage: each of min(k, n) rounds takes the not yet chosen vertex contained in the most UNCOVERED sets, ties to
 * the smallest id; the sets it hits become covered; a round with gain 0 still chooses (the smallest unchosen id).
 * Estimate: the spread of S is estimated as n * (sets hit by S) / theta, one double division.
 * Identity: for a fixed trial t and any seed set S,
 *     sum over all roots r of [S meets RR(t, r)]  =  |R_t(S)|,
 * the per-trial count gh_ic_spread returns for the same p, seed and max_hops (u reaches r forwards iff r reaches u
 * backwards, and both searches cut at the same number of hops).
 * Results depend only on (arc set, p, max_hops, seed, the samples): not on chunking or either memory budget. */
typedef struct gh_rr *gh_rr_handle;

/* An empty collection over vertex ids [0, n) on a device.  On failure *out = NULL, gh_rr_last_error(NULL) has the message. */
gh_status gh_rr_create(gh_rr_handle *out, int device_id, int64_t n);
void gh_rr_destroy(gh_rr_handle h);
const char *gh_rr_last_error(gh_rr_handle h);
/* Device bytes a collection may hold: 8 * (sets + 1) + 4 * sets + 4 * members.  0 restores the default, 4 GiB. */
gh_status gh_rr_set_memory_budget(gh_rr_handle h, int64_t bytes);
/* Appends n_samples RR sets drawn with ic's graph and coins; trials / roots: host arrays of n_samples, or NULL for the
 * defaults above.  Samples are chunked to ic's memory budget as gh_ic_spread chunks seed sets (n * (24 * W + 17) bytes for
 * 64 * W samples at once, W at most 128 and at most max(16, n / 2048)).  GH_ERR_INVALID for p outside [0, 1], max_hops < -1, a root outside [0, n), a collection of
 * another n or device.  GH_ERR_NOMEM, with the mean set size so far in gh_ic_last_error(ic), when the collection would
 * outgrow ITS budget: RIS is for sets that are small against n.  A failed call leaves the collection as it was.  Blocking. */
gh_status gh_ic_rr_sample(gh_ic_handle ic, gh_rr_handle rr, double p, int32_t max_hops, uint64_t seed, int64_t n_samples,
                          const uint64_t *trials, const int32_t *roots);
/* gh_ic_rr_sample with ic's per-arc table (gh_ic_set_arc_probabilities) in place of p: the same arguments, checks,
 * chunking and budgets.  GH_ERR_INVALID when no table has been set. */
gh_status gh_ic_rr_sample_arcs(gh_ic_handle ic, gh_rr_handle rr, int32_t max_hops, uint64_t seed, int64_t n_samples,
                               const uint64_t *trials, const int32_t *roots);
/* gh_ic_rr_sample under Linear Threshold with ic's table (gh_ic_set_lt_weights): the same arguments, checks, chunking,
 * default trials and roots, and budgets; an RR set is then a simple path backwards from the root.  GH_ERR_INVALID when no
 * Linear Threshold table has been set. */
gh_status gh_ic_rr_sample_lt(gh_ic_handle ic, gh_rr_handle rr, int32_t max_hops, uint64_t seed, int64_t n_samples,
                             const uint64_t *trials, const int32_t *roots);
gh_status gh_rr_counts(gh_rr_handle h, int64_t *n_sets, int64_t *n_members);
/* Host arrays (each may be NULL): indptr int64 (sets + 1), members int32, roots int32 (sets; -1 for an uploaded set
 * without one).  Blocking. */
gh_status gh_rr_download(gh_rr_handle h, int64_t *indptr, int32_t *members, int32_t *roots);
/* Replaces the contents by a host CSR, so maximum coverage serves any set system: indptr[0] = 0, not decreasing; the
 * members of a set in [0, n), strictly ascending; roots NULL or n_sets ids (-1: none).  Blocking. */
gh_status gh_rr_upload(gh_rr_handle h, int64_t n_sets, const int64_t *indptr, const int32_t *members, const int32_t *roots);
/* Greedy maximum coverage as above: seeds int32 and gains int64, host arrays of min(k, n).  Blocking. */
gh_status gh_rr_cover(gh_rr_handle h, int64_t k, int32_t *seeds, int64_t *gains);
/* *count = sets that contain at least one of the m vertices (duplicates allowed).  Blocking. */
gh_status gh_rr_count_hit(gh_rr_handle h, const int32_t *vertices, int64_t m, int64_t *count);

/* ---- centrality (reference benchmark.py: run_benchmark, benchmark_correlations; graphem-rapids_amd/centrality.py) ----
 * A handle over one undirected, unweighted graph, independent of the layout engine.  Self-loops are dropped and
 * duplicate edges merged.  Everything is fp64.
 *
 * Shortest paths from a source s (breadth-first levels): d(s, v) the hop distance, sigma_s(v) the number of shortest
 * s-v paths (a double, as networkx counts), pred_s(v) the neighbours u of v with d(s, u) = d(s, v) - 1.  Over the
 * successors w of v (v in pred_s(w)):
 *     delta_s(v)  = sum_w sigma_s(v) * ((1 + delta_s(w)) / sigma_s(w))     Brandes dependency (betweenness)
 *     lambda_s(v) = sum_w (1 + lambda_s(w)) / |pred_s(w)|                   Newman load dependency (load centrality)
 * Sources are taken in list order, 64 to a group (source j: group j / 64).  The per-vertex sums are formed as: for each
 * group in order, a fixed lane-tree sum over its 64 sources, added to the output with one fp64 add.  Results therefore
 * depend only on the graph and the ordered source list, bit for bit: not on the memory budget, edge order, duplicate
 * edges, self-loops, nor run-to-run scheduling. */
typedef struct gh_cent *gh_cent_handle;

/* edges: (n_edges, 2) int32 host array, vertex ids in [0, n).  On failure *out = NULL and gh_cent_last_error(NULL) has
 * the message. */
gh_status gh_cent_create(gh_cent_handle *out, int device_id, int64_t n, int64_t n_edges, const int32_t *edges);
void gh_cent_destroy(gh_cent_handle h);
const char *gh_cent_last_error(gh_cent_handle h);
/* Edges after self-loops and duplicates went. */
int64_t gh_cent_edge_count(gh_cent_handle h);
/* The handle's symmetric CSR on the device (neighbours ascending): indptr (n + 1) int64, indices int32.  Valid until
 * gh_cent_destroy; for gh_spmv_adj_shift. */
gh_status gh_cent_csr_device(gh_cent_handle h, const int64_t **indptr, const int32_t **indices);
/* Device bytes of path state gh_cent_paths may hold: n * (32 * 64 + 32) bytes per 64-source group processed at once, at
 * least one group.  0 restores the default, 1 GiB.  GH_ERR_INVALID for a negative value.  Results do not depend on it. */
gh_status gh_cent_set_memory_budget(gh_cent_handle h, int64_t bytes);
/* One all-sources pass over sources[0 .. n_sources) (ids in [0, n); duplicates allowed).
 * betweenness (NULL or host double[n]) = sum over the sources s != v of delta_s(v); load (NULL or host double[n]) =
 * sum over the sources s != v of lambda_s(v): raw sums, unnormalised (networkx _rescale / newman_betweenness_centrality
 * scale on the host).  reached, dist_sum (both NULL or both host int64[n_sources]): vertices reached from source j (the
 * source included) and the sum of their distances -- closeness on the host.  GH_ERR_INVALID for an id outside [0, n).
 * Blocking. */
gh_status gh_cent_paths(gh_cent_handle h, int64_t n_sources, const int32_t *sources, double *betweenness, double *load,
                        int64_t *reached, int64_t *dist_sum);
/* networkx _pagerank_scipy, uniform personalisation: x0 = 1 / N;  x <- alpha (x A_rownorm + (sum of x over the vertices of
 * degree 0) / N) + (1 - alpha) / N;  stops at the first iteration whose L1 change is < N * tol.  x: host double[n], the
 * result; *iterations = that iteration, or -1 when max_iter iterations did not converge (x then holds the last
 * iterate).  The convergence test runs on the device; the host reads its flag every 8 iterations.  GH_ERR_INVALID for
 * alpha outside [0, 1], max_iter < 1, tol < 0.  Blocking. */
gh_status gh_cent_pagerank(gh_cent_handle h, double alpha, int32_t max_iter, double tol, double *x, int32_t *iterations);
/* y = A x + c x for the 0/1 adjacency A in CSR form (e.g. gh_cent_csr_device): the operator of the eigenvector
 * centrality solve (the shift c > 0 separates the Perron root from -lambda_max on a bipartite graph).  All pointers are
 * DEVICE pointers; fp64; asynchronous on hip_stream (NULL = default stream).  gh_cent_last_error(NULL) has the message
 * of a failed call. */
gh_status gh_spmv_adj_shift(void *hip_stream, int64_t n, const int64_t *indptr, const int32_t *indices, double c,
                            const double *x, double *y);

/* ---- graph statistics (reference examples: real_world_datasets_example.py:111-175; graphem-rapids_amd/graphstats.py) --
 * Connected components, hop distances and triangles over a gh_cent handle's graph: undirected, unweighted, self-loops
 * dropped and duplicate edges merged.  Every output is an integer and every device sum is an integer atomic, so each
 * result is a pure function of the graph (and, for distances, of the source list), bit for bit: not of the memory
 * budget, edge order, duplicate edges, self-loops, nor run-to-run scheduling.  The calls are blocking and report through
 * gh_cent_last_error(h); a NULL handle gives GH_ERR_INVALID. */

/* labels (host int32[n]): labels[v] = the smallest vertex id in v's component; an isolated vertex is its own component.
 * *n_components (may be NULL) = the number of distinct labels.  Hook and shortcut: every vertex takes the smallest label
 * among its neighbours and hooks its tree's root under it, then pointer jumping flattens every tree, until a round
 * changes nothing; the host reads the device's change flags every 4 rounds. */
gh_status gh_cent_components(gh_cent_handle h, int32_t *labels, int64_t *n_components);
/* Breadth-first levels from sources[0 .. n_sources) (ids in [0, n); duplicates allowed; n_sources = 0 is a no-op), 64
 * sources to a machine word.  Each of reached, dist_sum (host int64[n_sources]) and eccentricity (host
 * int32[n_sources]) may be NULL: reached[j] = vertices source j reaches, itself included; dist_sum[j] = the sum of
 * their hop distances; eccentricity[j] = the greatest of them -- the greatest FINITE distance when source j does not
 * reach every vertex (reached[j] < n says so).  Device state: 24 n bytes per 64-source group (three 64-bit words per
 * vertex: visited, frontier, next frontier), as many groups at once as gh_cent_set_memory_budget allows, at least one;
 * results do not depend on it.  GH_ERR_INVALID for an id outside [0, n). */
gh_status gh_cent_distances(gh_cent_handle h, int64_t n_sources, const int32_t *sources, int64_t *reached,
                            int64_t *dist_sum, int32_t *eccentricity);
/* triangles (host int64[n]): triangles[v] = the number of triangles through v.  Per edge the shorter neighbour row is
 * searched in the longer one, so an edge costs min(deg) log(max deg); counts are 64-bit throughout. */
gh_status gh_cent_triangles(gh_cent_handle h, int64_t *triangles);

/* ---- cores and trusses (graphem-rapids_amd/cores.py) ----------------------------------------------------------------
 * The k-core and k-truss decompositions of a gh_cent handle's graph, under the preamble of "graph statistics":
 * undirected, unweighted, self-loops dropped, duplicate edges merged, every output an integer, blocking calls that
 * report through gh_cent_last_error(h), GH_ERR_INVALID for a NULL handle.  Each result is a pure function of the edge
 * set: not of edge order, duplicate edges, scheduling, nor of earlier calls on the handle.  Both are synchronous peels.
 *
 * Vertex peel (core number and onion layer).  State: deg[v], alive[v], threshold k = 0, round r = 0.  While a vertex is
 * alive:
 *     r += 1;  k = max(k, min over alive v of deg[v]);  S = {alive v : deg[v] <= k};
 *     every v in S gets core[v] = k and layer[v] = r and dies;
 *     every surviving vertex loses one degree per neighbour in S.
 * Isolated vertices leave in round 1 with core 0.  core is networkx.core_number, layer is networkx.onion_layers.
 *
 * Edge peel (truss number).  Edge ids are the positions in the canonical edge list: u < v, sorted by (u, v) -- the order
 * of the CSR's upper arcs.  sup[e] = the triangles through e whose three edges are alive.  State: j = 0, r = 0.  While an
 * edge is alive:
 *     r += 1;  j = max(j, min over alive e of sup[e]);  S = {alive e : sup[e] <= j};
 *     every e in S gets truss[e] = j + 2 and dies;
 *     every triangle that was alive at the start of the round and has an edge in S is destroyed, and each of its edges
 *     outside S loses exactly one support (on the device the triangle is charged to its smallest-id edge in S).
 * {e : truss[e] >= k} is the edge set of networkx.k_truss(G, k) for every k >= 2.
 *
 * A round is a fixed sequence of launches: select S, let S take what it owes from the survivors with integer atomicSub,
 * and a one-thread step that moves k (or j), r and the alive count on.  A selection that finds S empty only raises the
 * threshold to the minimum it saw and has no round number.  The host reads the device's "nobody alive" flag every 4
 * steps.  *n_rounds (may be NULL) = r at the end: the largest onion layer for the vertex peel.  More than 2^31 - 1 arcs
 * (twice the edges) give GH_ERR_INVALID; a peel that outlives its bound (items + 1 rounds) GH_ERR_RUNTIME. */

/* core, layer: host int32[n] each; either may be NULL.  n = 0: GH_OK with *n_rounds = 0.  Device state: 8 n bytes. */
gh_status gh_cent_cores(gh_cent_handle h, int32_t *core, int32_t *layer, int32_t *n_rounds);
/* truss: host int32[edges] in canonical edge order (gh_cent_edge_count).  No edges: GH_OK with *n_rounds = 0.  Device
 * state: 12 bytes per arc (edge id per arc; endpoint, arc position, support and removal round per edge), and 16 n bytes
 * plus a scan's work space while the edge ids are built. */
gh_status gh_cent_truss(gh_cent_handle h, int32_t *truss, int32_t *n_rounds);

/* ---- communities: Louvain levels and exact modularity (graphem-rapids_amd/communities.py) -------------------------------
 * Over a gh_cent handle's graph: undirected, unweighted, self-loops dropped and duplicate edges merged.  Every quantity
 * is an exact integer and no floating-point number is ever compared, so the result is a pure function of (edge set, n,
 * seed, max_levels, max_rounds), id for id: not of edge order, duplicate edges, self-loops, the memory budget, nor
 * run-to-run scheduling.  M = the sum of the degrees = 2 * edges.  Both calls give GH_ERR_INVALID for a handle of more
 * than 2^30 edges; up to there every product below fits int64 (M W <= M^2, k T <= M^2, sum T^2 <= M^2 <= 2^62).  A
 * handle of exactly 2^30 edges is refused as well: its 2^31 arcs are one more than the aggregation sort can count.
 *
 * Level graph: vertices 0 .. n_l - 1, symmetric integer weights w(u, v) >= 1 for u != v, a self weight s(u) >= 0, and
 * k(u) = s(u) + sum over v != u of w(u, v).  Level 0 has s = 0 and w = 1; sum k = M on every level.
 *
 * Numerator of a labelling c:  I(c) = sum over u in c of s(u) + sum over the ORDERED pairs u != v in c of w(u, v);
 * T(c) = sum over u in c of k(u);  N = M * sum_c I(c) - sum_c T(c)^2.  Modularity is N / M^2: one division of two exact
 * integers, left to the caller.
 *
 * One level starts from singletons, c(u) = u.  Round r = 0, 1, ... computes everything from the labels at its start:
 *   1. For every u and every community d != c(u) that holds a neighbour of u:
 *          W(u, d) = sum over v in d, v != u, of w(u, v);      val(d) = M W(u, d) - k(u) T(d);
 *          stay(u) = M W(u, c(u)) - k(u) (T(c(u)) - k(u)).
 *      target(u) = the d of largest val, the smallest d among equals, if val(d) > stay(u) strictly; else target(u) = c(u).
 *   2. If no vertex has target != c, the level ends.
 *   3. prio(u) = mix( mix(seed + level * 0x9E3779B97F4A7C15) ^ ((uint64)r << 32 | u) ), mix() as in the influence section,
 *      wrapping uint64 arithmetic.  u moves iff target(u) != c(u) and (prio(u), u) > (prio(v), v) for every neighbour
 *      v != u with target(v) != c(v): the movers of a round are pairwise non-adjacent.
 *   4. The moves are applied and N' computed.  N' > N keeps them and resets the failure count; otherwise the round is
 *      discarded and counts as one failure.  The level ends at two failures in a row, or after max_rounds rounds; the
 *      labels are then the last accepted ones.
 * rounds[level] = the rounds whose step 1 ran, the one that found no target included.
 *
 * Aggregation: a community's id is the level vertex it started from; coarse vertex ids are the ranks of the ids in use,
 * ascending; coarse w(a, b) = sum of w(u, v) over u in a, v in b; coarse s(a) = I(a).  The run ends when a level merges
 * nothing, or after max_levels levels.
 *
 * Device work per round: the best-move pass (rows up to 32 entries by groups of 8 lanes that combine the row's
 * (community, weight) pairs from a staged copy in LDS; longer rows by a workgroup with an LDS hash table keyed by
 * community; a row whose communities do not fit it goes on to a third pass over hash tables in global memory, as many at
 * once as gh_cent_set_memory_budget allows, at least one), the mover test, and the integer sums of N'.  The host reads
 * {any target, sum I', sum T'^2} once per round.  Aggregation sorts the arcs by their 64-bit (c(u), c(v)) keys and
 * reduces equal keys into the next level's CSR; that storage is proportional to the arcs and not divided by the budget. */

/* labels: host int32[n], any values in [0, n) (GH_ERR_INVALID otherwise).  out = {sum_c I(c), sum_c T(c)^2, M}. */
gh_status gh_cent_modularity(gh_cent_handle h, const int32_t *labels, int64_t out[3]);
/* labels: host int32 (max_levels, n); row l, for l < *n_levels, is the labelling after level l: labels[l][v] = the
 * smallest ORIGINAL vertex id in v's community (the convention of gh_cent_components).  One row per level that merged
 * something; when level 0 merges nothing, *n_levels = 1 and row 0 holds the singletons.  numerators (host
 * int64[max_levels]), n_communities (host int64[max_levels]) and rounds (host int32[max_levels]) give N, the community
 * count and the rounds run per row.  GH_ERR_INVALID for max_levels < 1 or max_rounds < 1.  Blocking. */
gh_status gh_cent_louvain(gh_cent_handle h, uint64_t seed, int32_t max_levels, int32_t max_rounds, int32_t *labels,
                          int32_t *n_levels, int64_t *numerators, int64_t *n_communities, int32_t *rounds);

/* ---- label propagation: synchronous, with clamped seeds (graphem-rapids_amd/classify.py: label_propagation) ---------------
 * The graph-side baseline of node classification, over a gh_cent handle's graph (undirected, self-loops dropped, duplicate
 * edges merged).  Every quantity is an integer; the result is a pure function of (graph, seed_labels, max_rounds).
 *
 * Input.  seed_labels: host int32[n]; -1 = unlabelled, any other value a class in [0, n_classes).  A labelled vertex is a
 * seed and never changes.  L_0 = seed_labels.
 * Round.  L_{i+1} is computed from L_i alone (two buffers).  For every non-seed v: count the classes of its neighbours w
 * with L_i[w] >= 0.  With no such neighbour v keeps L_i[v].  Otherwise best = the greatest count; v keeps L_i[v] if that is
 * >= 0 and its count equals best; else v takes the least class id whose count equals best.
 * Loop.  it = 0.  (1) if it == max_rounds: stop, converged = 0; (2) run a round, it += 1; (3) if no label changed in it:
 * stop, converged = 1; (4) repeat.  rounds = it.  max_rounds = 0 returns the input.
 *
 * 1 <= n_classes <= 1024.  labels: host int32[n], -1 where no label arrived; rounds and converged may be NULL.
 * GH_ERR_INVALID for an n_classes outside that range, for max_rounds < 0 and for "seed label <v> is outside [-1, n_classes)".
 * Device state: 12 n bytes of labels.  The host reads one flag per round.  Blocking. */
gh_status gh_cent_label_propagation(gh_cent_handle h, int32_t n_classes, const int32_t *seed_labels, int32_t max_rounds,
                                    int32_t *labels, int32_t *rounds, int32_t *converged);

/* ---- graph generators (reference generators.py: generate_sbm / generate_bipartite_graph, generate_geometric,
 * generate_ba; graphem-rapids_amd/generators.py) ------------------------------------------------------------------
 * Three random graph families whose every random decision is a counter-based word, so an edge list is a pure function
 * of the parameters and the seed -- not of launch geometry, memory budget, scheduling, nor of whether the device or
 * the host path ran -- and can be recomputed bit for bit in integer arithmetic.  With mix() of the influence section
 * and G = 0x9E3779B97F4A7C15, uint64 wrapping arithmetic:
 *     word(seed, i, j) = mix( mix(seed + (i + 1) * G) ^ j )          (i + 1: mix(0) = 0, and seed 0 is the default)
 * No transcendental function sits between a word and a decision: doubles appear only in tables and thresholds that are
 * computed once on the host with IEEE +, -, * alone (no fused multiply-add).
 * Every result is the edge list with u < v, no duplicates, sorted by (u, v).
 *
 * Block model.  Blocks a = 0 .. B-1 of sizes[a] vertices, numbered block after block (block a starts at off[a]);
 * P (B, B) row-major, symmetric, entries in [0, 1].  Block pairs are numbered q = 0, 1, .. in the order (0,0), (0,1), ..,
 * (0,B-1), (1,1), .. (a <= b).  The pair space of block pair (a, b) has N vertex pairs, index i in [0, N):
 *     a < b:   N = s_a * s_b;            i -> (off[a] + i / s_b,  off[b] + i % s_b)
 *     a == b:  N = s (s - 1) / 2, h = (s - 1) / 2 (integer division);
 *              i <  s * h:  r = i / h, c = i % h  -> { off + r, off + (r + 1 + c) % s }     (circulant layout)
 *              i >= s * h:  r = i - s * h         -> { off + r, off + r + s / 2 }           (s even: the diameters)
 * Each pair space is cut into segments of GH_GEN_SBM_SEGMENT indices (the last one shorter); segments are numbered
 * g = 0, 1, .. through the block pairs in order (a block pair with N = 0 has none).  Gap table of a probability p, with
 * q = 1 - p and pw[0] = 1, pw[k + 1] = pw[k] * q (doubles, one rounding per operation):
 *     cdf[k] = (uint64) floor( (1 - pw[k + 1]) * 2^52 ),   k = 0 .. GH_GEN_SBM_TABLE - 1
 * Segment g covering [lo, hi) of its pair space is walked with pos = lo, j = 0:
 *     r = word(seed, g, j) >> 12; j += 1;  k = the number of table entries with cdf[k] <= r;
 *     k == GH_GEN_SBM_TABLE (the tail):  pos += GH_GEN_SBM_TABLE          -- redraw; the geometric gap is memoryless
 *     else:  pos += k;  if pos < hi: pair(pos) is an edge;  pos += 1
 * until pos >= hi.  p = 0 gives no edge and p = 1 every pair, exactly.
 *
 * Random geometric graph.  Vertex i has the integer coordinates k_d(i) = word(seed, i, d) >> 40 (24 bits), d = 0 ..
 * dim - 1, 1 <= dim <= 8; its position is k_d * 2^-24 (exact in float32).  (u, v) is an edge iff
 *     sum over d of (k_d(u) - k_d(v))^2  <=  R2 = (uint64) floor( min(radius * radius, 16.0) * 2^48 ).
 *
 * Preferential attachment (networkx barabasi_albert_graph as a process), 1 <= m < n.  The endpoint list: slots
 * 0 .. 2m-1 hold the star on vertices 0 .. m (slot 2i: vertex 0, slot 2i + 1: vertex i + 1); vertex v > m owns slots
 * 2m(v - m) + 2t (holding v) and 2m(v - m) + 2t + 1 (holding its t-th accepted target), t = 0 .. m-1.  Vertex v draws
 *     slot(v, a) = floor( word(seed, v, a) * 2m(v - m) / 2^64 ),   a = 0, 1, 2, ..
 * and accepts the vertex in that slot as its next target unless it already holds it, until it holds m targets.  Edges:
 * (0, i) for i = 1 .. m and (target, v); E = m (n - m).  On the device a vertex is finished in the first round in which
 * every slot it draws belongs to the star, is an even slot, or belongs to a vertex finished in an EARLIER round (one
 * launch per round; nothing waits on another workgroup); more than GH_GEN_BA_MAX_ROUNDS rounds is an error. */
#define GH_GEN_SBM_SEGMENT 16384
#define GH_GEN_SBM_TABLE 1024
#define GH_GEN_BA_MAX_ROUNDS 4096
typedef struct gh_gen *gh_gen_handle;

/* device_id >= 0: kernels on that device.  device_id < 0: the host path (no device is touched), same edges bit for
 * bit.  On failure *out = NULL and gh_gen_last_error(NULL) has the message. */
gh_status gh_gen_create(gh_gen_handle *out, int device_id);
void gh_gen_destroy(gh_gen_handle h);
const char *gh_gen_last_error(gh_gen_handle h);
/* Bytes a generator call may allocate for segment counts and edges (16 bytes per edge: the 64-bit keys u << 32 | v and
 * the radix sort's second buffer).  0 restores the default, 4 GiB.  A graph that needs more returns GH_ERR_NOMEM with
 * the figures in the message, decided from the count pass before any edge is written; nothing is truncated.  Results
 * do not depend on it. */
gh_status gh_gen_set_memory_budget(gh_gen_handle h, int64_t bytes);
/* Each call replaces the handle's result and reports its edge count; vertex ids must fit int32 (n < 2^31).  Blocking.
 * sizes: host int64[n_blocks], each >= 0; P: host double (n_blocks, n_blocks), symmetric. */
gh_status gh_gen_sbm(gh_gen_handle h, int32_t n_blocks, const int64_t *sizes, const double *P, uint64_t seed,
                     int64_t *n_edges);
gh_status gh_gen_geometric(gh_gen_handle h, int64_t n, double radius, int32_t dim, uint64_t seed, int64_t *n_edges);
/* rounds (may be NULL): launches the dependency resolution took (0 on the host path, which runs the process in order). */
gh_status gh_gen_ba(gh_gen_handle h, int64_t n, int64_t m, uint64_t seed, int64_t *n_edges, int32_t *rounds);
/* The last result: edges host int32 (E, 2); positions host float32 (n, dim) of the last gh_gen_geometric. */
gh_status gh_gen_edges(gh_gen_handle h, int32_t *edges);
gh_status gh_gen_positions(gh_gen_handle h, float *positions);

/* ---- rank correlation (reference visualization.py: report_corr, report_full_correlation_matrix;
 * graphem-rapids_amd/visualization.py) ------------------------------------------------------------------------------
 * Spearman's rho between columns of one table, plain and over bootstrap resamples, in exact integer arithmetic.
 *
 * Columns: m >= 1 columns of n doubles, 2 <= n <= GH_CORR_MAX_N (so that n^3 < 2^63), all finite.  Values compare as
 * IEEE doubles: -0.0 and 0.0 tie.  A tie group of a column is a maximal set of points with equal value.
 *
 * Resample b (0 <= b < reps), with word() of the generator section:
 *     idx(b, j) = floor( word(seed, b, j) * n / 2^64 ),  j = 0 .. n-1          (128-bit product, high word)
 *     c_i       = the number of j with idx(b, j) = i                            (the sum of c is n)
 * The plain statistic is the case c_i = 1 for all i.
 *
 * For a column and a weight vector c, with the groups in ascending value order, C_g = the sum of c over group g and
 * B_g = the sum of C over the groups before g:
 *     u_i = 2 * B_g(i) + C_g(i) - n          (an integer; = 2 * midrank - (n + 1); the weighted mean of u is exactly 0)
 * For a pair of columns (x, y) with u from x and v from y:
 *     Sxy = sum c_i u_i v_i,   Sxx = sum c_i u_i^2,   Syy = sum c_i v_i^2                      (exact in int64)
 *     rho = NaN if Sxx = 0 or Syy = 0, else (double)Sxy / sqrt((double)Sxx * (double)Syy)      (gh_corr_rho)
 * The device computes the three integers; the conversion to double is gh_corr_rho on the host for both paths, so
 * device and host agree bit for bit.  Results depend only on (columns, pairs, reps, seed): not on batch size, memory
 * budget, sort stability, launch geometry, nor on whether the device or the host path ran. */
#define GH_CORR_MAX_N 2097151
typedef struct gh_corr *gh_corr_handle;

/* columns: host double (m, n) row-major.  device_id >= 0: kernels on that device; device_id < 0: the host path (no
 * device is touched).  Each column is prepared once: an order-preserving 64-bit key per value, a sort, and for every
 * sorted position the start and end of its tie group.  GH_ERR_INVALID for a NaN or an infinity, for n < 2 and for
 * n > GH_CORR_MAX_N (larger tables need 128-bit sums).  On failure *out = NULL and gh_corr_last_error(NULL) has the
 * message. */
gh_status gh_corr_create(gh_corr_handle *out, int device_id, int64_t n, int32_t m, const double *columns);
void gh_corr_destroy(gh_corr_handle h);
const char *gh_corr_last_error(gh_corr_handle h);
/* Device bytes of replicate state gh_corr_bootstrap may hold: about 4 n + 8 n per column in use + 24 per pair, per
 * replicate processed at once, at least one replicate.  0 restores the default, 4 GiB.  GH_ERR_INVALID for a negative value.
 * Results do not depend on it; the host path ignores it. */
gh_status gh_corr_set_memory_budget(gh_corr_handle h, int64_t bytes);
/* The conversion both paths use. */
double gh_corr_rho(int64_t sxy, int64_t sxx, int64_t syy);
/* The m x m matrix of the plain statistic: out host double (m, m), symmetric, diagonal 1 (NaN for a constant column).
 * sums: NULL or host int64 (m, m, 3), the triple (Sxy, Sxx, Syy) of every entry (row = x, column = y).  Blocking. */
gh_status gh_corr_matrix(gh_corr_handle h, double *out, int64_t *sums);
/* pairs: host int32 (n_pairs, 2) of column ids; out: host double (n_pairs, reps), rho of every pair in every resample.
 * Replicate b uses one c for all pairs.  sums: NULL or host int64 (n_pairs, reps, 3).  Replicates are processed in
 * batches sized by the memory budget; only columns that occur in `pairs` are ranked.  GH_ERR_INVALID for reps < 1,
 * n_pairs < 1, a column id outside [0, m).  Blocking. */
gh_status gh_corr_bootstrap(gh_corr_handle h, int32_t n_pairs, const int32_t *pairs, int32_t reps, uint64_t seed,
                            double *out, int64_t *sums);

/* ---- layout quality: edge crossings and edge lengths (graphem-rapids_amd/quality.py) -------------------------------
 * The one measure of the loop's own product: how many pairs of edges of a layout cross, under the test the engine
 * itself uses, as an exact integer.
 *
 * pos: (n, D) float32.  edges: (E, 2) int32, taken as given: ids are kept, nothing is merged or dropped, and an edge's
 * index is its id.  Edges i != j CROSS iff D >= 2, they share no vertex (the four-way id comparison of gh_intersect_pair),
 * and with a = pos[u_i], b = pos[v_i], c = pos[u_j], d = pos[v_j] on coordinates 0 and 1 only and
 *     orient(p, q, r) = (q0 - p0) * (r1 - p1) - (q1 - p1) * (r0 - p0)
 * (every operation a separate IEEE float32 operation, no contraction, gradual underflow)
 *     orient(a, b, c) * orient(a, b, d) < 0   and   orient(c, d, a) * orient(c, d, b) < 0,     both products in float32.
 * That is gh_orient2d and the test of csrc/intersect_core.h (reference pt.py:760-772) without its i < j filter.  The
 * relation is symmetric in (i, j): the two products are exchanged.  Self-loops and duplicate edges never cross anything.
 * Swapping an edge's endpoints changes the point the differences are taken from, so orient(b, a, c) is -orient(a, b, c)
 * only up to rounding: counts of nearly collinear quadruples can depend on the direction an edge is stored in, exactly as
 * the engine's own forces do.
 *     counts[r] = the number of edges j in [0, E) that cross edge rows[r]
 * and with all edges as rows the layout's crossing number is sum(counts) / 2.
 * It is a float32 rule: the same formula in double gives other counts wherever the four points are nearly collinear,
 * and two segments with disjoint bounding boxes can cross under it (csrc/quality.hip has a case), so every pair is tested.
 *
 * Edge lengths use all D coordinates: L_e = sqrt(sum_d ((double)x_u,d - (double)x_v,d)^2), the sum in order
 * d = 0 .. D-1, in double, no contraction.
 *
 * Results depend only on (edges, positions, rows / pairs): not on launch geometry, nor on whether the device or the
 * host path ran -- except the two length sums, whose order of summation is the path's own. */
typedef struct gh_qual *gh_qual_handle;

/* edges: host int32 (n_edges, 2).  device_id >= 0: kernels on that device; device_id < 0: the host path (no device is
 * touched).  GH_ERR_INVALID for a vertex id outside [0, n) ("edge <i> has a vertex id outside [0, n)").  On failure
 * *out = NULL and gh_qual_last_error(NULL) has the message. */
gh_status gh_qual_create(gh_qual_handle *out, int device_id, int64_t n, int64_t n_edges, const int32_t *edges);
void gh_qual_destroy(gh_qual_handle h);
const char *gh_qual_last_error(gh_qual_handle h);
/* Takes a snapshot of (n, D) float32 rows; ld >= D is the row stride in floats.  on_device = 0: pos is a host pointer.
 * on_device = 1: pos is a device pointer on the handle's device (gh_positions_unpadded_device(engine) with ld = D, for
 * one); it is copied on the handle's stream before the call returns, and the engine may go on afterwards.  Later
 * queries see the snapshot until positions are set again.  GH_ERR_INVALID for D < 1, ld < D, on_device on a host-path
 * handle.  D = 1 is valid: every count is 0. */
gh_status gh_qual_set_positions(gh_qual_handle h, const float *pos, int32_t D, int64_t ld, int32_t on_device);
/* rows: host int32, n_rows edge ids in any order and with repeats; NULL = all E edges in order (n_rows is ignored).
 * counts: host int32, one per row.  sum (may be NULL): the sum of counts.  GH_ERR_INVALID for an id outside [0, E)
 * and for a query before any positions were set.  Blocking. */
gh_status gh_qual_crossings(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int32_t *counts, int64_t *sum);
/* The test for explicit pairs: pairs host int32 (n_pairs, 2) of edge ids; cross[p] = 0 or 1.  Blocking. */
gh_status gh_qual_pairs(gh_qual_handle h, int64_t n_pairs, const int32_t *pairs, uint8_t *cross);
/* out = {min L, max L, sum L, sum L^2} over all edges; {+inf, -inf, 0, 0} for an empty edge list.  Blocking. */
gh_status gh_qual_edge_lengths(gh_qual_handle h, double out[4]);

/* ---- embedding quality: exact neighbour ranks (graphem-rapids_amd/quality.py: neighbor_ranks, link_auc,
 * neighborhood_preservation, embedding_quality) -- the same gh_qual handle ------------------------------------------------
 * Are a vertex's neighbours nearer to it than the vertices it is not joined to?  Under every such measure lies one exact
 * pair of integers per (vertex, neighbour): how many other vertices lie strictly nearer, and how many exactly as near.
 *
 * Graph.  The simple undirected graph of the handle's edge list: self-loops dropped, repeats and both directions merged
 * (graphstats.py's convention).  N(u) = u's distinct neighbours, ids ascending; k_u = |N(u)|; m_u = n - 1 - k_u.  The
 * crossing functions above keep taking the edge list as given.  The graph is built on the host by the first query.
 * Distance.  For float32 rows x,
 *     d2(u, w) = (((0 + t_0 * t_0) + t_1 * t_1) + ... + t_{D-1} * t_{D-1}),   t_d = x[u][d] - x[w][d],
 * every subtraction, product and sum a separate IEEE float32 operation in the order d = 0 .. D-1, nothing contracted, all
 * D coordinates used.  (a - b)^2 and (b - a)^2 are the same float, so d2 is symmetric in (u, w) bit for bit.  It is a
 * float32 rule: a float64 embedder's positions are rounded to float32 first.  Comparisons are IEEE: a NaN distance is
 * neither below nor equal to anything, +inf equals +inf.  A NaN threshold is returned as the quiet NaN 0x7FC00000: the
 * sign and payload an operation gives a NaN are the hardware's, not IEEE's.
 * Counts.  For a source u and each v in N(u), with t = d2(u, v):
 *     below(u -> v) = #{ w in [0, n), w != u, w != v : d2(u, w) <  t }
 *     equal(u -> v) = #{ w in [0, n), w != u, w != v : d2(u, w) == t }
 * over neighbours and non-neighbours alike.  Results depend only on (edges, positions, rows): not on launch geometry, on
 * how a long row is cut into pieces, or on whether the device or the host path ran.  No float is ever summed.
 *
 * rows: host int32, n_rows source vertex ids in any order, repeats allowed; NULL = all n vertices in order (n_rows is
 * ignored).  The result is in CSR form over rows: row r owns the slots [indptr[r], indptr[r + 1]), one per neighbour of
 * rows[r], ids ascending.  GH_ERR_INVALID for a row id outside [0, n) ("row <r> has a vertex id outside [0, n)"). */
/* indptr: host int64, n_rows + 1 (n + 1 for rows == NULL).  Needs no positions. */
gh_status gh_qual_neighbor_sizes(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int64_t *indptr);
/* The fill: host arrays of indptr[n_rows] slots each (they may be NULL when that is 0): the neighbour's id, the
 * threshold d2(u, v) (its bits), below and equal.  GH_ERR_INVALID for a query before any positions were set.  D = 1 is
 * valid.  Blocking. */
gh_status gh_qual_neighbor_ranks(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2,
                                 int32_t *below, int32_t *equal);

/* ---- distance preservation: hop profile, stress, Shepard curve (graphem-rapids_amd/quality.py: hop_profile, layout_stress,
 * hop_distance_correlation, distance_quality) -- the same gh_qual handle -----------------------------------------------------
 * Does the embedding preserve graph distance as a whole?  Under stress, the Shepard curve and the correlation of embedding
 * distance with hop distance lie the same sums: per hop and per source, over every (source, vertex) pair the graph joins.
 *
 * Graph.  The simple undirected graph of the handle's edge list, exactly as for the neighbour ranks: self-loops dropped,
 * repeats and both directions merged.  hop(s, v) = the breadth-first distance.
 * Distance.  d2(s, v) is the float32 chain above over all D coordinates.  A pair contributes d = sqrt((double)d2), an IEEE
 * double square root, and q = (double)d2.
 * Sources.  sources[0 .. S), ids in [0, n) in any order; a repeat is a source of its own.  NULL = all n vertices in order
 * (n_sources is ignored).
 * Pairs.  P = {(j, v) : v != sources[j], v reachable from sources[j]}.  With all vertices as sources every unordered pair
 * appears twice -- d2 is symmetric bit for bit.
 * Per hop h = 1 .. H, H = the greatest hop in P (0 when P is empty), at entry h - 1 of each array:
 *     pairs   (int64)   the number of pairs at hop h
 *     sum_d, sum_d2     (double)  sum of d, sum of q over them
 *     min_d2, max_d2    (float32) the exact least and greatest d2 among them
 * Per source j:
 *     reach[j]          (int64)   the number of pairs (j, v) in P: the source itself is not counted
 *     eccentricity[j]   (int32)   the greatest finite hop; 0 when nothing is reached
 *     sum_d_over_h[j]   (double)  sum over v of d / hop
 *     sum_d2_over_h2[j] (double)  sum over v of q / hop^2
 * Exactness.  The integers and the bits of min_d2 / max_d2 are pure functions of (edges, positions, sources): they do not
 * depend on launch geometry, on how sources are batched into 64-bit groups, on edge order or duplicates, or on whether the
 * device or the host path ran.  The four kinds of double sums are sums of non-negative, individually well-defined terms;
 * only the order of summation, and where the division by h or h^2 is applied (both paths divide a source's sum over one hop),
 * is the path's own -- as for the two length sums of gh_qual_edge_lengths.  A sum of N terms is within (N + 2) 2^-53 of the
 * true sum, relatively.  On the device the order within a workgroup is that of its LDS adds, so two runs can differ there.
 * Non-finite positions.  Rows with a NaN or an infinity leave the integer outputs exact; the float outputs are then
 * unspecified.
 *
 * hop_cap: the length of the per-hop arrays; n always suffices.  *n_hops (may be NULL) = H.  Every output array may be NULL.
 * GH_ERR_INVALID for a source id outside [0, n) ("source <j> has a vertex id outside [0, n)"), for a query before any
 * positions were set, and for hop_cap < H with a per-hop array given (*n_hops is set, so the call can be repeated).
 * S = 0 is a no-op with H = 0.  The device path keeps as many 64-source groups in flight as 1 GiB of search state allows
 * (24 n bytes a group), at least one.  Blocking. */
gh_status gh_qual_hop_profile(gh_qual_handle h, int64_t n_sources, const int32_t *sources, int64_t hop_cap, int64_t *n_hops,
                              int64_t *pairs, double *sum_d, double *sum_d2, float *min_d2, float *max_d2, int64_t *reach,
                              int32_t *eccentricity, double *sum_d_over_h, double *sum_d2_over_h2);

/* ---- embedding clusters: exact k-means, k-means++ minima, silhouette sums (graphem-rapids_amd/clusters.py: kmeans,
 * kmeans_plusplus, nearest_center, silhouette_samples, silhouette_score, cluster_recovery) -- the same gh_qual handle ------
 * Do the clusters of the embedding equal the communities of the graph?  k-means on the position snapshot, with integer
 * results that are a pure function of the input, and the sums the silhouette is a few divisions of.
 *
 * Distance.  d2(x, c) is the float32 chain of "embedding quality" over all D coordinates, between a snapshot row x and a
 * centre row c: t_d = x[d] - c[d].
 * Assignment.  label(v) = the least c in [0, k) that minimises d2(x_v, centre_c): with best = +inf and label = 0, c is walked
 * upwards and taken when d2 < best, strictly.  A +inf or NaN distance is never taken: a row whose distances all overflow
 * keeps label 0 and best = +inf.  The returned d2[v] is best.
 * Centre update, exact.  M = the greatest |x| of the snapshot; s = 38 - ilogb(M), or 0 when M = 0;
 *     q(x) = llrint(ldexp((double)x, s)), ties to even      (|q| <= 2^39)
 *     S[c][d] = sum of q(x_v[d]) over the members v of c, in int64; count[c] = the number of members
 *     centre[c][d] = (float) ldexp((double)S[c][d] / (double)count[c], -s)
 * and a cluster without members keeps its centre.  n <= 2^24 cannot overflow S; a larger n is refused.  Integer adds commute,
 * so labels, d2, counts and the centres' bits depend only on (positions, start centres, max_iter): not on launch geometry,
 * the order of atomic adds, or whether the device or the host path ran; and a permuted vertex order gives the same centres.
 * Lloyd loop.  it = 0, no prev.  (1) assign; (2) if it > 0 and the labels equal prev: converged, stop; (3) if it == max_iter:
 * not converged, stop; (4) update the centres, prev = labels, it += 1; (5) repeat.  The returned labels and d2 always belong
 * to the returned centres; n_iter = the number of updates; max_iter = 0 is a plain assignment.
 * Seeding.  The handle keeps min_d2[w] = min(min_d2[w], d2(x_w, x_vertex)) over the seed steps since the last one with
 * `first` set, which starts it at d2(x_w, x_vertex); the draw itself is the caller's.
 * Distance sums.  sums[r][c] = the sum over w with labels[w] == c, w != rows[r], of sqrt((double)d2(rows[r], w)): non-negative
 * double terms whose order of summation is the path's own, within (N + 2) 2^-53 of the true sum relatively, as for the hop
 * profile's sums.
 *
 * 1 <= k <= min(n, 4096).  centres: host float32 (k, D), packed.  GH_ERR_INVALID for a k outside that range, for a query
 * before any positions were set, for a snapshot row that holds a NaN or an infinity ("position row <v> is not finite"), for
 * such a centre ("centre <c> is not finite"), for a label outside [0, k) ("label <w> is outside [0, k)") and for a row id
 * outside [0, n) ("row <r> has a vertex id outside [0, n)").  All calls are blocking. */
/* out: host float32 (n_rows, D): the snapshot's rows rows[0 .. n_rows), ids in any order, repeats allowed -- the start
 * centres of a run that begins at chosen vertices, without a download of the layout. */
gh_status gh_qual_position_rows(gh_qual_handle h, int64_t n_rows, const int32_t *rows, float *out);
/* labels: host int32, n; d2: host float32, n. */
gh_status gh_qual_kmeans_assign(gh_qual_handle h, int32_t k, const float *centres, int32_t *labels, float *d2);
/* centres: the start centres in, the last centres out.  counts: host int64, k members per cluster of the returned labels;
 * counts, n_iter and converged may be NULL.  GH_ERR_INVALID for max_iter < 0 and for n > 2^24. */
gh_status gh_qual_kmeans(gh_qual_handle h, int32_t k, float *centres, int32_t max_iter, int32_t *labels, float *d2, int64_t *counts,
                         int32_t *n_iter, int32_t *converged);
/* min_d2: host float32, n: the handle's running minimum after this step.  GH_ERR_INVALID for a vertex outside [0, n) and
 * for a step without `first` when none with it came before on these positions. */
gh_status gh_qual_kmeans_seed_step(gh_qual_handle h, int64_t vertex, int32_t first, float *min_d2);
/* labels: host int32, n, every one in [0, k).  rows: host int32, n_rows vertex ids in any order, repeats allowed; NULL = all
 * n vertices in order (n_rows is ignored).  sums: host float64 (n_rows, k).  The device path takes the rows in batches, so
 * its working memory is bounded: 4 n D bytes of sorted columns and at most 256 MiB of partial sums. */
gh_status gh_qual_cluster_distance_sums(gh_qual_handle h, int32_t k, const int32_t *labels, int64_t n_rows, const int32_t *rows,
                                        double *sums);

/* ---- node classification: exact k nearest labelled vertices and their vote (graphem-rapids_amd/classify.py: knn_neighbors,
 * knn_classify, node_classification_benchmark) -- the same gh_qual handle ----------------------------------------------------
 * Given the classes of a few vertices, which class does the embedding give the others?  The k nearest of a SUBSET of the
 * snapshot's rows under a total order, and the vote of their classes: integers and float32 bits that are a pure function of
 * the input.
 *
 * Training set.  train[0 .. n_train) are distinct vertex ids in [0, n), in any order; train_labels[i] >= 0 is the class of
 * train[i].  A class id has no bound and there is no class count: ids may be sparse (0 and 1 000 000).  train_labels == NULL
 * is allowed; pred and votes must then be NULL too.
 * Queries.  rows[0 .. n_rows) are vertex ids in any order, repeats allowed; NULL = all n vertices in order (n_rows is ignored).
 * Distance.  d2(u, t) is the float32 chain of "embedding quality" over all D coordinates between the snapshot rows u and t.
 * Candidates of a query u: every training vertex t != u.  A query that is itself a training vertex never votes for itself, so
 * train = rows = all vertices is leave-one-out in one call.
 * Order.  (d2(u, t), t) ascending: the float distance by IEEE comparison, then the smaller vertex id.  A snapshot with a row
 * that is not finite is refused, so no NaN arises; +inf distances (an overflowing difference) are legal, tie, and are ordered
 * by id.
 * Taken.  The first m = min(k, number of candidates) candidates in that order: neighbors[r][j] and d2[r][j] hold the j-th;
 * the slots j >= m hold -1 and +inf.
 * Vote.  votes[r] = the greatest number of taken neighbours that share one class; pred[r] = the least class id that reaches
 * it.  m = 0 gives pred = -1 and votes = 0.
 * Results depend only on (positions, train, train_labels, rows, k): not on the order of train, on launch geometry, on how the
 * training set is cut into tiles and pieces, or on whether the device or the host path ran.
 *
 * 1 <= k <= 128.  neighbors (int32) and d2 (float32) are host arrays of shape (n_rows, k); pred and votes host int32,
 * n_rows; each of the four may be NULL.  n_train = 0 is valid.  GH_ERR_INVALID for a k outside that range, for a query before
 * any positions were set, for "training row <i> has a vertex id outside [0, n)", "training row <i> repeats vertex <v>" (i walks
 * upwards, the id is tested first), "label <i> is negative", "row <r> has a vertex id outside [0, n)" and "position row <v> is
 * not finite".  Blocking.  The device path takes the rows in batches of at most 2^22 list entries, so its working memory is
 * bounded: 4 T (D + 2) bytes of gathered training rows, 4 n bytes of training ranks, 4 n_rows of row ids, at most 128 MiB of
 * per-piece lists and 48 MiB of results. */
gh_status gh_qual_knn_vote(gh_qual_handle h, int32_t k, int64_t n_train, const int32_t *train, const int32_t *train_labels,
                           int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2, int32_t *pred, int32_t *votes);

/* ---- edge-list ingestion: text -> (vertices, edges) (reference datasets.py: SNAPDataset.load, _load_mtx_file,
 * _load_edges_file; graphem-rapids_amd/datasets.py) ------------------------------------------------------------------
 * The reference reads a file in text mode line by line, tests line.startswith(c), takes line.strip().split() and calls
 * int() on the first two fields.  The rule below is that, restated on bytes; every result is an exact integer.
 *
 * Lines.  A terminator is CR LF, LF or CR, longest match first (Python's universal newlines).  A line is the bytes
 * between two terminators; the last line needs none.  CR LF counts once, for line numbers and for the mtx header.
 * Blanks are the bytes 0x09, 0x0B, 0x0C, 0x1C .. 0x1F and 0x20.  A byte >= 0x80 is never a blank (a declared deviation:
 * Python also splits on U+0085 and U+00A0).
 * Fields.  A field is a maximal run of non-blank bytes of a line.  A line with fewer than two fields is skipped without
 * a look at its content; fields after the second are never read.
 * Integers.  The first two fields must match [+-]?[0-9]+ and fit int64 (leading zeros are fine); anything else -- a
 * letter, an underscore, a non-ASCII digit, a lone sign, overflow -- is an error (a declared deviation: Python takes
 * 1_0 and non-ASCII digits).  Labels may be negative; their order is the signed one.
 * Formats.  GH_INGEST_SNAP and GH_INGEST_EDGES: a line whose FIRST BYTE is '#' is skipped whole (" # x y" is no comment
 * and so an error).  GH_INGEST_MTX: the leading run of lines whose first byte is '%' and the one line after it, whatever
 * it holds, are skipped; after that nothing is a comment; both labels are decremented by one, and a label of INT64_MIN
 * is an error.
 * Errors.  GH_ERR_INVALID with the FIRST offending line in file order, 1-based, and the field's text, as
 *     "line <N>: invalid integer '<field>'"      or      "line <N>: integer outside int64 '<field>'".
 * Results.  R = the number of data rows.  Directed: the R rows in file order as they are (self-loops and repeats stay).
 * Undirected: the sorted unique pairs (min, max) with min < max, in signed order (numpy's unique(axis=0)).  vertices =
 * the sorted distinct labels of the returned edges (GH_INGEST_FROM_EDGES, SNAPDataset.load: a vertex that has only a
 * self-loop drops out of an undirected result) or of all R rows (GH_INGEST_FROM_ROWS, _load_mtx_file and
 * _load_edges_file).  relabel replaces every label by its rank in vertices.  R = 0 gives empty arrays.
 * Limits.  More than 2^31 - 1 distinct labels, 2^30 or more rows, or a single line of 2^31 bytes or more: an error status.
 *
 * The device path takes the text in chunks of chunk_bytes = budget / GH_INGEST_BUDGET_PER_BYTE bytes, cut only after a
 * whole terminator (never between CR and LF; a line longer than a chunk makes that chunk longer).  Results depend only
 * on (bytes, format, directed, vertices_from): not on chunking, budget, launch geometry or atomic order, nor on whether
 * the device or the host path ran. */
#define GH_INGEST_SNAP 0
#define GH_INGEST_EDGES 1
#define GH_INGEST_MTX 2
#define GH_INGEST_FROM_EDGES 0
#define GH_INGEST_FROM_ROWS 1
#define GH_INGEST_BUDGET_PER_BYTE 40   /* device bytes a chunk may need per byte of text (every byte a line: 29) */
#define GH_INGEST_MIN_BUDGET 4096
typedef struct gh_ingest *gh_ingest_handle;

/* device_id >= 0: kernels on that device.  device_id < 0: the host path (no device is touched), same arrays bit for
 * bit.  On failure *out = NULL and gh_ingest_last_error(NULL) has the message. */
gh_status gh_ingest_create(gh_ingest_handle *out, int device_id);
void gh_ingest_destroy(gh_ingest_handle h);
const char *gh_ingest_last_error(gh_ingest_handle h);
/* Device bytes of working state one chunk may hold (text, line starts, parsed lines); the rows themselves and the
 * sorts' buffers (48 bytes per row) come on top.  0 restores the default, 4 GiB; GH_ERR_INVALID below
 * GH_INGEST_MIN_BUDGET.  Results do not depend on it; the host path ignores it. */
gh_status gh_ingest_set_memory_budget(gh_ingest_handle h, int64_t bytes);
/* bytes: host, nbytes >= 0.  Each call replaces the handle's result.  Blocking. */
gh_status gh_ingest_parse(gh_ingest_handle h, const uint8_t *bytes, int64_t nbytes, int32_t format, int32_t directed,
                          int32_t vertices_from);
/* The same with the text already on the handle's device as well: d_bytes, 16-byte aligned, holds the same nbytes.  The
 * host copy is still read for the cuts, the mtx header and an error's line number; nothing is uploaded. */
gh_status gh_ingest_parse_uploaded(gh_ingest_handle h, const uint8_t *bytes, const uint8_t *d_bytes, int64_t nbytes,
                                   int32_t format, int32_t directed, int32_t vertices_from);
/* Of the last parse: data rows R, returned edges, vertices (each pointer may be NULL). */
gh_status gh_ingest_counts(gh_ingest_handle h, int64_t *rows, int64_t *edges, int64_t *vertices);
/* chunk_bytes under the current budget and the number of chunks the last parse took (0 on the host path). */
gh_status gh_ingest_chunking(gh_ingest_handle h, int64_t *chunk_bytes, int64_t *chunks);
/* vertices: host int64[vertices].  edges: host int64 (edges, 2); relabel != 0: ranks in vertices instead of labels. */
gh_status gh_ingest_copy_vertices(gh_ingest_handle h, int64_t *vertices);
gh_status gh_ingest_copy_edges(gh_ingest_handle h, int32_t relabel, int64_t *edges);

/* ---- link scores (graphem-rapids_amd/links.py) --------------------------------------------------------------------------
 * The classical neighbourhood predictors of link prediction over a gh_cent handle's graph: undirected, unweighted,
 * self-loops dropped, duplicate edges merged.  N(v) is row v of the handle's CSR and deg(v) its length.  Every device
 * quantity is an integer, so every result is a pure function of the edge set and the arguments: not of the memory
 * budget, edge order, duplicate edges, scheduling, nor of earlier calls on the handle.  Both calls are blocking and
 * report through gh_cent_last_error(h); a NULL handle gives GH_ERR_INVALID.
 *
 * Fixed-point weights, scale 2^32:
 *     W_ra(d) = (2^33 + d) / (2 d) in integer division: 2^32 / d rounded half up;  W_ra(0) = 0
 *     W_aa(d) = nearbyint(2^32 / log(d)) for d >= 2, else 0: computed on the host in double, once per handle, as a table
 *               over 0 .. the largest degree, and uploaded -- the device never evaluates a logarithm.
 * For a pair (u, v), over the common neighbours w in N(u) & N(v):
 *     cn = |N(u) & N(v)|     aa = sum W_aa(deg w)     ra = sum W_ra(deg w)     uni = deg u + deg v - cn     pa = deg u * deg v
 * all int64.  u = v is allowed and gives cn = deg u.  A graph whose largest degree is >= 2^30 gives GH_ERR_INVALID (the
 * sums would leave int64).
 *
 * A score kind ranks by the rational key num / den:
 *     GH_LINK_CN cn / 1     GH_LINK_JACCARD cn / uni     GH_LINK_AA aa / 1     GH_LINK_RA ra / 1     GH_LINK_PA pa / 1
 * Two keys are compared by cross-multiplication in integers (both products fit in 64 bits); the larger key ranks first,
 * equal keys rank the smaller vertex id first: a strict total order, so a top-k is unique.
 * The candidates of a source u are C(u) = {v : v != u, v not in N(u), N(u) & N(v) not empty}: the vertices at hop distance
 * exactly two. */
enum { GH_LINK_CN = 0, GH_LINK_JACCARD = 1, GH_LINK_AA = 2, GH_LINK_RA = 3, GH_LINK_PA = 4 };

/* The weight a common neighbour of that degree adds to the sum of `kind`: W_aa for GH_LINK_AA, W_ra for GH_LINK_RA, 1 for
 * the three kinds that count; -1 for another kind or a degree outside [0, 2^30).  Host only, no device. */
int64_t gh_link_weight(int32_t kind, int64_t degree);
/* pairs: host int32 (n_pairs, 2), ids in [0, n) (GH_ERR_INVALID otherwise: "pair <i> has a vertex id outside [0, n)"), in
 * any order, repeats allowed; n_pairs = 0 is a no-op.  cn, aa, ra: host int64[n_pairs], each may be NULL.  A group of
 * lanes takes one pair: its lanes stride over the shorter row, each bisects the longer one, and the group adds up its
 * three integer sums with shuffles.  The group is 4 .. 64 lanes wide, the power of two at or above the mean degree.
 * Device state: 32 bytes per pair, as many pairs at once as gh_cent_set_memory_budget allows, at least one. */
gh_status gh_cent_link_scores(gh_cent_handle h, int64_t n_pairs, const int32_t *pairs, int64_t *cn, int64_t *aa,
                              int64_t *ra);
/* For each of rows[0 .. n_rows) (ids in [0, n), any order, repeats allowed; GH_ERR_INVALID otherwise: "row <r> has a
 * vertex id outside [0, n)") the k best members of C(rows[r]) under the order of `kind`, best first: ids int32, num and
 * den int64, (n_rows, k) each, host.  Unused slots hold id -1, num 0, den 1.  1 <= k <= 128 (GH_ERR_INVALID otherwise,
 * and for another kind).  Persistent workgroups take the rows off a counter; each owns a slab of n int64 sums, zero
 * between two rows, and a candidate buffer, 20 n bytes together, as many workgroups as gh_cent_set_memory_budget allows,
 * at least one and at most 1024.  Per row: (a) every wedge u-w-v adds the weight of deg w to slab[v] with integer
 * atomics; (b) the wedges are walked again and slab[v] is exchanged for 0 -- the one lane that gets a non-zero value
 * owns v, drops it when v = u or v is in row u, and appends it to the buffer otherwise; (c) k passes over the buffer take
 * the best entry below the one before.  The outputs of up to 2^22 / k rows at once (20 k bytes a row) come on top. */
gh_status gh_cent_link_candidates(gh_cent_handle h, int32_t kind, int32_t k, int64_t n_rows, const int32_t *rows,
                                  int32_t *ids, int64_t *num, int64_t *den);

/* Device / build facts for the host mirror's get_backend_info(). */
int32_t gh_device_count(void);
const char *gh_version(void);

/* Debugging aid for tests of the handles' life cycles: the device allocations that handles and calls of this library hold
 * in this process right now, and their bytes (either pointer may be NULL).  Closing a handle gives back all of its own. */
void gh_debug_live_allocations(int64_t *count, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHEM_HIP_H */
