// Layout quality (include/graphem_hip.h "layout quality"): how many pairs of edges of a layout cross under the engine's own
// float32 test on coordinates 0 and 1, and the edge-length statistics, behind gh_qual_*.
//
// The pair test is gh_orient2d and the condition of gh_intersect_pair (intersect_core.h), compiled for both sides: the
// kernels and the host path (device_id < 0) run the same function, so they give the same integers.
//
//   qual_segments_kernel   one gather per snapshot: (a0, a1, b0, b1) of every edge; with the edge list itself that is the
//                          24-byte segment table, and the pair loop never touches the position array
//   qual_cross_kernel      all pairs (row, column): a thread keeps one row segment in registers, the workgroup walks the
//                          column tiles of the table through LDS (every lane reads the same column: a broadcast, no bank
//                          conflict) and counts in a register; one int32 store per row, no atomics
//   qual_sum_kernel        adds the partial counts when the columns of a few rows were split over several workgroups
//   qual_pairs_kernel      the test for listed pairs
//   qual_length_kernel     per-edge length in double; min / max / sum / sum of squares by wave shuffles and one LDS step,
//                          one partial per workgroup, combined on the host in workgroup order (deterministic, no atomics)
//
//   qual_rank_kernel       neighbour ranks ("embedding quality" in the header): a wave owns up to 64 (source, neighbour) slots
//                          of one source, lane i keeps threshold i and its two counts in registers, the workgroup walks the
//                          position tiles through LDS, and per 64 columns each threshold costs two compares, two ballots and
//                          two popcounts; no atomics.  qual_rank_sum_kernel adds the partial counts of split columns.
//
// The crossing kernel runs the full square: row i meets every column j, and nothing is credited to a column.  There is no pruning
// by bounding boxes: it would not be exact.  Two segments whose closed bounding boxes are disjoint CAN cross under the
// float32 test, because for four nearly collinear points all four orientation values are rounding noise of either sign:
//     a = (0.06998461484909058, 0.06998474150896072)   b = (2.662574529647827, 2.662574291229248)
//     c = (4.330337047576904, 4.330337047576904)       d = (6.195383548736572, 6.195383548736572)
// gives o1 = -9.536743e-07, o2 = 9.536743e-07, o3 = 9.536743e-07, o4 = -4.7683716e-07: a crossing, with every x of the
// first segment below every x of the second (tests/test_quality_cpu.py keeps this case).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"
#include "intersect_core.h"

#define QUAL_BLOCK 256
#define QUAL_TILE 1024                      // column segments staged at once: 24 KiB of LDS
#define QUAL_LAUNCH_PAIRS (1ll << 36)       // pair tests per launch: rows are taken in batches of about a second
#define QUAL_LAUNCH_ROWS (1ll << 22)
#define QUAL_MIN_BLOCKS 2048                // fewer row blocks than this: the column tiles are split over gridDim.y
#define QUAL_LEN_BLOCKS 1024
#define QUAL_HOST_THREADS 16
#define QUAL_RANK_PIECE 64                  // slots of one source that one wave owns: lane i keeps threshold i (at most 64)
#define QUAL_RANK_WAVES (QUAL_BLOCK / 64)   // pieces per workgroup: they share the staged position tile
#define QUAL_RANK_LDS 8192                  // floats of the position tile, D rows of tile_cols columns: 32 KiB
#define QUAL_RANK_TILE 1024                 // columns of a tile at most; fewer when D * 1024 floats do not fit
#define QUAL_RANK_LAUNCH_PAIRS (1ll << 40)  // (piece, column) pairs per launch: pieces are taken in batches of about a second
#define QUAL_RANK_LAUNCH_ITEMS (1ll << 22)

namespace {

// The rule for one pair: no shared vertex, and both float32 products strictly negative.  Branch-free on purpose.
__host__ __device__ __forceinline__ int qual_cross(const float4 &p, const int2 &e, const float4 &q, const int2 &f) {
    const bool shared = (e.x == f.x) | (e.x == f.y) | (e.y == f.x) | (e.y == f.y);
    const float a[2] = {p.x, p.y}, b[2] = {p.z, p.w}, c[2] = {q.x, q.y}, d[2] = {q.z, q.w};
    const float o1 = gh_orient2d(a, b, c), o2 = gh_orient2d(a, b, d);
    const float o3 = gh_orient2d(c, d, a), o4 = gh_orient2d(c, d, b);
    return (int)(!shared & (o1 * o2 < 0.0f) & (o3 * o4 < 0.0f));
}

__host__ __device__ __forceinline__ float4 qual_segment(const float *pos, int64_t ld, int D, const int2 &uv) {
    const float *a = pos + (int64_t)uv.x * ld, *b = pos + (int64_t)uv.y * ld;
    return make_float4(a[0], D >= 2 ? a[1] : 0.0f, b[0], D >= 2 ? b[1] : 0.0f);
}

__host__ __device__ __forceinline__ double qual_length(const float *pos, int64_t ld, int D, const int2 &uv) {
    const float *a = pos + (int64_t)uv.x * ld, *b = pos + (int64_t)uv.y * ld;
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
        const double t = (double)a[d] - (double)b[d];
        s += t * t;
    }
    return sqrt(s);
}

// (n, D) rows of stride ld -> packed rows
__global__ __launch_bounds__(QUAL_BLOCK) void qual_pack_kernel(int64_t total, int D, int64_t ld, const float *__restrict__ src,
                                                               float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (i < total) dst[i] = src[(i / D) * ld + i % D];
}

__global__ __launch_bounds__(QUAL_BLOCK) void qual_segments_kernel(int64_t E, const int2 *__restrict__ edges,
                                                                   const float *__restrict__ pos, int D, float4 *__restrict__ seg) {
    const int64_t e = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (e < E) seg[e] = qual_segment(pos, D, D, edges[e]);
}

// Rows [row0, row0 + nr) of `rows` (NULL: row r is edge r) against the column tiles [blockIdx.y * tiles_per_chunk, ...).
// out[blockIdx.y * nr + (r - row0)] = the number of crossing columns among them.  E >= 1.
__global__ __launch_bounds__(QUAL_BLOCK) void qual_cross_kernel(int64_t E, const float4 *__restrict__ seg, const int2 *__restrict__ edges,
                                                                int64_t row0, int64_t nr, const int32_t *__restrict__ rows,
                                                                int64_t tiles_per_chunk, int32_t *__restrict__ out) {
    __shared__ float4 s_p[QUAL_TILE];
    __shared__ int2 s_e[QUAL_TILE];
    const int64_t local = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    const bool live = local < nr;
    const int64_t i = live ? (rows ? (int64_t)rows[row0 + local] : row0 + local) : 0;   // an idle thread tests edge 0 and stores nothing
    const float4 p = seg[i];
    const int2 e = edges[i];
    const int64_t n_tiles = (E + QUAL_TILE - 1) / QUAL_TILE;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_chunk, t1 = min(n_tiles, t0 + tiles_per_chunk);
    int32_t cnt = 0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * QUAL_TILE;
        const int m = (int)min((int64_t)QUAL_TILE, E - base);   // the last tile is partial
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += QUAL_BLOCK) {
            s_p[k] = seg[base + k];
            s_e[k] = edges[base + k];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) cnt += qual_cross(p, e, s_p[j], s_e[j]);
    }
    if (live) out[(int64_t)blockIdx.y * nr + local] = cnt;
}

__global__ __launch_bounds__(QUAL_BLOCK) void qual_sum_kernel(int64_t nr, int chunks, const int32_t *__restrict__ part, int32_t *__restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (r >= nr) return;
    int32_t s = 0;
    for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * nr + r];
    out[r] = s;
}

__global__ __launch_bounds__(QUAL_BLOCK) void qual_pairs_kernel(int64_t n_pairs, const int2 *__restrict__ pairs, const float4 *__restrict__ seg,
                                                                const int2 *__restrict__ edges, int D, uint8_t *__restrict__ cross) {
    const int64_t p = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    const int2 ij = pairs[p];
    cross[p] = (uint8_t)(D >= 2 && ij.x != ij.y ? qual_cross(seg[ij.x], edges[ij.x], seg[ij.y], edges[ij.y]) : 0);
}

struct qual_len {
    double mn, mx, s, ss;
};

__host__ __device__ __forceinline__ void qual_len_join(qual_len &a, const qual_len &b) {
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.s += b.s;
    a.ss += b.ss;
}

// part[4 * blockIdx.x ..] = {min, max, sum, sum of squares} of the lengths of the edges this workgroup strides over
__global__ __launch_bounds__(QUAL_BLOCK) void qual_length_kernel(int64_t E, const int2 *__restrict__ edges, const float *__restrict__ pos,
                                                                 int D, double *__restrict__ part) {
    __shared__ qual_len s_w[QUAL_BLOCK / 64];
    qual_len v = {INFINITY, -INFINITY, 0.0, 0.0};
    for (int64_t e = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * QUAL_BLOCK) {
        const double L = qual_length(pos, D, D, edges[e]);
        const qual_len one = {L, L, L, L * L};
        qual_len_join(v, one);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const qual_len o = {__shfl_down(v.mn, off, 64), __shfl_down(v.mx, off, 64), __shfl_down(v.s, off, 64), __shfl_down(v.ss, off, 64)};
        qual_len_join(v, o);
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < QUAL_BLOCK / 64; ++w) qual_len_join(v, s_w[w]);
        double *o = part + 4 * (int64_t)blockIdx.x;
        o[0] = v.mn; o[1] = v.mx; o[2] = v.s; o[3] = v.ss;
    }
}

// ---- neighbour ranks -------------------------------------------------------------------------------------------------
// The exact-difference chain of the header: (((0 + t_0 t_0) + t_1 t_1) + ...), t_d = a[d] - b[d * sb], every operation a
// separate float32 operation (the Makefile's -ffp-contract=off keeps the product and the sum apart).  a is a packed row; b
// has stride sb, which is 1 for a packed row and the tile's column count for a column of the staged tile.
__host__ __device__ __forceinline__ float qual_d2(const float *a, const float *b, int64_t sb, int D) {
    float s = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float t = a[d] - b[d * sb];
        s = s + t * t;
    }
    return s;
}

// What one column at distance d adds to the two counts of a threshold t: IEEE comparisons, so a NaN on either side adds
// nothing and +inf equals +inf.
__host__ __device__ __forceinline__ int qual_is_below(float d, float t) { return (int)(d < t); }
__host__ __device__ __forceinline__ int qual_is_equal(float d, float t) { return (int)(d == t); }
// Column v itself is at distance t exactly -- d2(u, v) is the very chain the threshold came from -- so the walk over all
// columns counts it in `equal` once unless t is NaN.  This is the w != v exclusion, made once per slot, not once per column.
__host__ __device__ __forceinline__ int qual_own_column(float t) { return (int)(t == t); }

// lane i's x, for an i that is the same in every lane
__device__ __forceinline__ float qual_lane_value(float x, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), i)); }

// The threshold as it is returned: the sign and payload of a NaN are whatever the hardware and the compiler's choice of
// instructions made of them (a negated operand flips the sign), so a NaN is returned as the one quiet NaN 0x7FC00000.
__host__ __device__ __forceinline__ float qual_returned_d2(float t) {
    union { uint32_t u; float f; } nan = {0x7FC00000u};
    return t == t ? t : nan.f;
}

// A piece: up to QUAL_RANK_PIECE consecutive output slots [slot0, slot0 + len) of source u.  A row longer than a piece is
// cut into several; the counts of a slot do not depend on the cut.
struct qual_item {
    int64_t slot0;
    int32_t u, len;
};

// Wave w of workgroup blockIdx.x owns piece item0 + 4 * blockIdx.x + w and meets the columns of the tiles
// [blockIdx.y * tiles_per_chunk, ...).  out[blockIdx.y * batch_slots + (slot - slot_base)] = (below, equal) among them;
// d2out[slot] = the threshold (written by chunk 0).  STAGED: the tile goes through LDS as D rows of tile_cols columns, so
// consecutive lanes read consecutive words; otherwise (D too large for one 64-column tile) columns are read from memory.
template <bool STAGED>
__global__ __launch_bounds__(QUAL_BLOCK) void qual_rank_kernel(int64_t n, int D, const float *__restrict__ pos, int tile_cols,
                                                               const qual_item *__restrict__ items, int64_t item0, int64_t n_items,
                                                               const int32_t *__restrict__ nbr, int64_t tiles_per_chunk, int64_t slot_base,
                                                               int64_t batch_slots, float *__restrict__ d2out, int2 *__restrict__ out) {
    __shared__ float s_tile[STAGED ? QUAL_RANK_LDS : 1];
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * QUAL_RANK_WAVES + (threadIdx.x >> 6);
    const bool live = it < n_items;   // the same in every lane; an idle wave stages its share of the tile and counts nothing
    const int64_t slot0 = live ? items[item0 + it].slot0 : 0;
    // one value per wave, said so to the compiler: the loops over a piece's thresholds are scalar loops
    const int u = __builtin_amdgcn_readfirstlane(live ? items[item0 + it].u : 0);
    const int len = __builtin_amdgcn_readfirstlane(live ? items[item0 + it].len : 0);
    const float *xu = pos + (int64_t)u * D;
    const bool mine = lane < len;
    const int v = mine ? nbr[slot0 + lane] : 0;
    const float tv = mine ? qual_d2(xu, pos + (int64_t)v * D, 1, D) : NAN;
    float tmax = -INFINITY;   // the largest threshold that is no NaN: a column beyond it adds nothing to any count of the piece
    for (int i = 0; i < len; ++i) tmax = fmaxf(tmax, qual_lane_value(tv, i));
    const int64_t n_tiles = (n + tile_cols - 1) / tile_cols;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_chunk, t1 = min(n_tiles, t0 + tiles_per_chunk);
    int32_t below = 0, equal = 0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * tile_cols;
        const int m = (int)min((int64_t)tile_cols, n - base);   // the last tile is partial
        if (STAGED) {
            __syncthreads();
            for (int d = 0; d < D; ++d)
                for (int c = threadIdx.x; c < m; c += QUAL_BLOCK) s_tile[d * tile_cols + c] = pos[(base + c) * D + d];
            __syncthreads();
        }
        if (!live) continue;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int c = c0 + lane;
            const int64_t w = base + c;
            float d = NAN;   // a lane past the tile's end and the column w == u add nothing
            if (c < m && w != u) d = STAGED ? qual_d2(xu, s_tile + c, tile_cols, D) : qual_d2(xu, pos + w * D, 1, D);
            if (__ballot(d <= tmax) == 0) continue;
            for (int i = 0; i < len; ++i) {
                const float ti = qual_lane_value(tv, i);
                const int nb = __popcll(__ballot(qual_is_below(d, ti))), ne = __popcll(__ballot(qual_is_equal(d, ti)));
                if (lane == i) { below += nb; equal += ne; }
            }
        }
    }
    if (mine) {
        if (v >= t0 * tile_cols && v < t1 * tile_cols) equal -= qual_own_column(tv);   // v < n: t1 * tile_cols may pass n, v cannot
        out[(int64_t)blockIdx.y * batch_slots + (slot0 - slot_base) + lane] = make_int2(below, equal);
        if (blockIdx.y == 0) d2out[slot0 + lane] = qual_returned_d2(tv);
    }
}

__global__ __launch_bounds__(QUAL_BLOCK) void qual_rank_sum_kernel(int64_t slots, int chunks, const int2 *__restrict__ part, int2 *__restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (s >= slots) return;
    int2 a = make_int2(0, 0);
    for (int c = 0; c < chunks; ++c) {
        const int2 p = part[(int64_t)c * slots + s];
        a.x += p.x;
        a.y += p.y;
    }
    out[s] = a;
}

unsigned qual_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + QUAL_BLOCK - 1) / QUAL_BLOCK); }

}  // namespace

struct gh_qual : gh_host {          // device < 0: host path
    int64_t n = 0, E = 0;
    int32_t D = 0;                  // 0: no positions yet
    size_t pos_bytes = 0;
    gh_dev<int2> d_edges;
    gh_dev<float> d_pos;            // the snapshot, packed (n, D)
    gh_dev<float4> d_seg;
    std::vector<int2> h_edges;
    std::vector<float> h_pos;
    std::vector<float4> h_seg;
    // the simple graph of the edge list (self-loops dropped, repeats and both directions merged), built by the first
    // neighbour query: neighbours of u = g_idx[g_ptr[u] .. g_ptr[u + 1]), ids ascending
    bool g_built = false;
    std::vector<int64_t> g_ptr;
    std::vector<int32_t> g_idx;
};

static thread_local std::string g_qual_error;

namespace {

gh_status qual_invalid(gh_qual *h, const std::string &msg) {
    h->err = msg;
    return GH_ERR_INVALID;
}

// fn(first, last) over [0, count) on up to QUAL_HOST_THREADS threads
template <class Fn> void qual_host_parallel(int64_t count, int64_t grain, Fn fn) {
    const int64_t want = std::min<int64_t>(QUAL_HOST_THREADS, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    const int64_t nt = std::max<int64_t>(1, std::min(want, count / std::max<int64_t>(1, grain)));
    if (nt == 1) { fn(0, count); return; }
    std::vector<std::thread> pool;
    for (int64_t t = 0; t < nt; ++t) pool.emplace_back(fn, count * t / nt, count * (t + 1) / nt);
    for (auto &th : pool) th.join();
}

gh_status qual_crossings_device(gh_qual *h, int64_t n_rows, const int32_t *rows, int32_t *counts) {
    GH_HIP(hipSetDevice(h->device));
    gh_dev<int32_t> d_rows, d_counts, d_part;
    if (!d_counts.alloc(4 * n_rows) || (rows && !d_rows.alloc(4 * n_rows))) {
        h->err = "hipMalloc failed for " + std::to_string(8 * n_rows) + " bytes of rows and counts";
        return GH_ERR_NOMEM;
    }
    if (rows) GH_HIP(hipMemcpyAsync(d_rows.p, rows, 4 * n_rows, hipMemcpyHostToDevice, h->stream));
    const int64_t n_tiles = (h->E + QUAL_TILE - 1) / QUAL_TILE;
    const int64_t batch = std::max<int64_t>(QUAL_BLOCK, std::min<int64_t>(QUAL_LAUNCH_ROWS, QUAL_LAUNCH_PAIRS / h->E / QUAL_BLOCK * QUAL_BLOCK));
    for (int64_t row0 = 0; row0 < n_rows; row0 += batch) {
        const int64_t nr = std::min(batch, n_rows - row0);
        const int64_t row_blocks = (nr + QUAL_BLOCK - 1) / QUAL_BLOCK;
        // a few rows only (a sample, a small graph): their columns are split so that every compute unit has work
        const int64_t chunks = std::max<int64_t>(1, std::min(n_tiles, QUAL_MIN_BLOCKS / row_blocks));
        const int64_t tiles_per_chunk = (n_tiles + chunks - 1) / chunks;
        const int64_t used = (n_tiles + tiles_per_chunk - 1) / tiles_per_chunk;
        if (used > 1 && !d_part.p && !d_part.alloc(4 * (size_t)QUAL_MIN_BLOCKS * QUAL_BLOCK)) {
            h->err = "hipMalloc failed for the partial counts";
            return GH_ERR_NOMEM;
        }
        // used * nr <= (QUAL_MIN_BLOCKS / row_blocks) * row_blocks * QUAL_BLOCK: inside d_part
        int32_t *out = used > 1 ? d_part.p : d_counts.p + row0;
        qual_cross_kernel<<<dim3((unsigned)row_blocks, (unsigned)used), dim3(QUAL_BLOCK), 0, h->stream>>>(
            h->E, h->d_seg.p, h->d_edges.p, row0, nr, rows ? d_rows.p : nullptr, tiles_per_chunk, out);
        GH_LAUNCH_CHECK();
        if (used > 1) {
            qual_sum_kernel<<<dim3((unsigned)row_blocks), dim3(QUAL_BLOCK), 0, h->stream>>>(nr, (int)used, d_part.p, d_counts.p + row0);
            GH_LAUNCH_CHECK();
        }
    }
    GH_HIP(hipMemcpyAsync(counts, d_counts.p, 4 * n_rows, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

void qual_crossings_host(const gh_qual *h, int64_t n_rows, const int32_t *rows, int32_t *counts) {
    const int64_t E = h->E;
    const float4 *seg = h->h_seg.data();
    const int2 *edges = h->h_edges.data();
    qual_host_parallel(n_rows, 16, [=](int64_t first, int64_t last) {
        for (int64_t r = first; r < last; ++r) {
            const int64_t i = rows ? rows[r] : r;
            const float4 p = seg[i];
            const int2 e = edges[i];
            int32_t cnt = 0;
            for (int64_t j = 0; j < E; ++j) cnt += qual_cross(p, e, seg[j], edges[j]);
            counts[r] = cnt;
        }
    });
}

// The simple graph, once per handle.  A device handle keeps its edge list on the device only, so it is read back here.
gh_status qual_build_graph(gh_qual *h) {
    if (h->g_built) return GH_OK;
    std::vector<int2> fetched;
    const int2 *edges = h->h_edges.data();
    if (h->device >= 0 && h->E > 0) {
        GH_HIP(hipSetDevice(h->device));
        fetched.resize((size_t)h->E);
        GH_HIP(hipMemcpyAsync(fetched.data(), h->d_edges.p, 8 * (size_t)h->E, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        edges = fetched.data();
    }
    std::vector<uint64_t> keys;
    GH_TRY_ST(gh_canonical_edge_keys(h->n, h->E, (const int32_t *)edges, false, "edge", &keys, &h->err));
    h->g_ptr.assign((size_t)h->n + 1, 0);
    for (uint64_t k : keys) {
        h->g_ptr[(size_t)(k >> 32) + 1] += 1;
        h->g_ptr[(size_t)(k & 0xFFFFFFFFu) + 1] += 1;
    }
    for (int64_t u = 0; u < h->n; ++u) h->g_ptr[u + 1] += h->g_ptr[u];
    h->g_idx.resize(2 * keys.size());
    std::vector<int64_t> fill(h->g_ptr.begin(), h->g_ptr.end() - 1);
    // keys ascend by (a, b) with a < b: row b takes its smaller neighbours a in ascending order first, then row a its
    // larger neighbours b in ascending order, so every row ends up ascending
    for (uint64_t k : keys) h->g_idx[(size_t)fill[k & 0xFFFFFFFFu]++] = (int32_t)(k >> 32);
    for (uint64_t k : keys) h->g_idx[(size_t)fill[k >> 32]++] = (int32_t)(k & 0xFFFFFFFFu);
    h->g_built = true;
    return GH_OK;
}

// The checks both neighbour calls share; afterwards *n_rows is the row count (n for rows == NULL) and the graph is built.
gh_status qual_rank_rows(gh_qual *h, int64_t *n_rows, const int32_t *rows) {
    if (!rows) *n_rows = h->n;
    if (*n_rows < 0) return qual_invalid(h, "n_rows must be >= 0, got " + std::to_string(*n_rows));
    for (int64_t r = 0; rows && r < *n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= h->n) return qual_invalid(h, "row " + std::to_string(r) + " has a vertex id outside [0, n)");
    return qual_build_graph(h);
}

void qual_ranks_host(const gh_qual *h, int64_t n_rows, const int32_t *rows, const int64_t *indptr, const int32_t *nbr, float *d2,
                     int32_t *below, int32_t *equal) {
    const int64_t n = h->n;
    const int D = h->D;
    const float *pos = h->h_pos.data();
    qual_host_parallel(n_rows, 1, [=](int64_t first, int64_t last) {
        for (int64_t r = first; r < last; ++r) {
            const int64_t u = rows ? rows[r] : r, s0 = indptr[r], k = indptr[r + 1] - s0;
            const float *xu = pos + u * D;
            float tmax = -INFINITY;
            for (int64_t i = 0; i < k; ++i) {
                d2[s0 + i] = qual_returned_d2(qual_d2(xu, pos + (int64_t)nbr[s0 + i] * D, 1, D));
                tmax = fmaxf(tmax, d2[s0 + i]);
                below[s0 + i] = 0;
                equal[s0 + i] = -qual_own_column(d2[s0 + i]);
            }
            for (int64_t w = 0; k > 0 && w < n; ++w) {
                if (w == u) continue;
                const float d = qual_d2(xu, pos + w * D, 1, D);
                if (!(d <= tmax)) continue;
                for (int64_t i = 0; i < k; ++i) {
                    below[s0 + i] += qual_is_below(d, d2[s0 + i]);
                    equal[s0 + i] += qual_is_equal(d, d2[s0 + i]);
                }
            }
        }
    });
}

gh_status qual_ranks_device(gh_qual *h, int64_t n_rows, const int32_t *rows, const int64_t *indptr, const int32_t *nbr, float *d2,
                            int32_t *below, int32_t *equal) {
    const int64_t slots = indptr[n_rows], n = h->n;
    // rows are cut into pieces of at most QUAL_RANK_PIECE slots, one wave each
    std::vector<qual_item> items;
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t s = indptr[r]; s < indptr[r + 1]; s += QUAL_RANK_PIECE)
            items.push_back({s, rows ? rows[r] : (int32_t)r, (int32_t)std::min<int64_t>(QUAL_RANK_PIECE, indptr[r + 1] - s)});
    const int64_t n_items = (int64_t)items.size();
    GH_HIP(hipSetDevice(h->device));
    gh_dev<qual_item> d_items;
    gh_dev<int32_t> d_nbr;
    gh_dev<float> d_d2;
    gh_dev<int2> d_cnt, d_part;
    if (!d_items.alloc(sizeof(qual_item) * (size_t)n_items) || !d_nbr.alloc(4 * (size_t)slots) || !d_d2.alloc(4 * (size_t)slots) ||
        !d_cnt.alloc(8 * (size_t)slots)) {
        h->err = "hipMalloc failed for " + std::to_string(16 * (n_items + slots)) + " bytes of neighbour slots";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(qual_item) * (size_t)n_items, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_nbr.p, nbr, 4 * (size_t)slots, hipMemcpyHostToDevice, h->stream));
    // the tile: D rows of tile_cols columns in QUAL_RANK_LDS floats, tile_cols a multiple of 64; none fits: no staging
    const int fit = (int)std::min<int64_t>(QUAL_RANK_TILE, QUAL_RANK_LDS / h->D / 64 * 64);
    const bool staged = fit >= 64;
    const int tile_cols = staged ? fit : QUAL_RANK_TILE;
    const int64_t n_tiles = (n + tile_cols - 1) / tile_cols;
    const int64_t batch = std::max<int64_t>(QUAL_RANK_WAVES, std::min<int64_t>(QUAL_RANK_LAUNCH_ITEMS, QUAL_RANK_LAUNCH_PAIRS / n / QUAL_RANK_WAVES * QUAL_RANK_WAVES));
    for (int64_t item0 = 0; item0 < n_items; item0 += batch) {
        const int64_t ni = std::min(batch, n_items - item0);
        const int64_t slot_base = items[item0].slot0, batch_slots = items[item0 + ni - 1].slot0 + items[item0 + ni - 1].len - slot_base;
        const int64_t blocks = (ni + QUAL_RANK_WAVES - 1) / QUAL_RANK_WAVES;
        // a few pieces only (a sample, a small graph): their columns are split so that every compute unit has work
        const int64_t chunks = std::max<int64_t>(1, std::min(n_tiles, QUAL_MIN_BLOCKS / blocks));
        const int64_t tiles_per_chunk = (n_tiles + chunks - 1) / chunks;
        const int64_t used = (n_tiles + tiles_per_chunk - 1) / tiles_per_chunk;
        if (used > 1 && d_part.bytes < 8 * (size_t)(used * batch_slots) && !d_part.alloc(8 * (size_t)(used * batch_slots))) {
            h->err = "hipMalloc failed for the partial counts";
            return GH_ERR_NOMEM;
        }
        int2 *out = used > 1 ? d_part.p : d_cnt.p + slot_base;
        auto kernel = staged ? qual_rank_kernel<true> : qual_rank_kernel<false>;
        kernel<<<dim3((unsigned)blocks, (unsigned)used), dim3(QUAL_BLOCK), 0, h->stream>>>(
            n, h->D, h->d_pos.p, tile_cols, d_items.p, item0, ni, d_nbr.p, tiles_per_chunk, slot_base, batch_slots, d_d2.p, out);
        GH_LAUNCH_CHECK();
        if (used > 1) {
            qual_rank_sum_kernel<<<dim3(qual_grid(batch_slots)), dim3(QUAL_BLOCK), 0, h->stream>>>(batch_slots, (int)used, d_part.p, d_cnt.p + slot_base);
            GH_LAUNCH_CHECK();
        }
    }
    std::vector<int2> cnt((size_t)slots);
    GH_HIP(hipMemcpyAsync(d2, d_d2.p, 4 * (size_t)slots, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, 8 * (size_t)slots, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    for (int64_t s = 0; s < slots; ++s) {
        below[s] = cnt[s].x;
        equal[s] = cnt[s].y;
    }
    return GH_OK;
}

}  // namespace

extern "C" gh_status gh_qual_create(gh_qual_handle *out, int device_id, int64_t n, int64_t n_edges, const int32_t *edges) {
    if (!out) { g_qual_error = "out is NULL"; return GH_ERR_INVALID; }
    *out = nullptr;
    if (n < 0 || n_edges < 0 || n_edges > 0x7FFFFFFFll || (n_edges > 0 && !edges)) {
        g_qual_error = "n and n_edges must be >= 0, n_edges below 2^31, and edges given";
        return GH_ERR_INVALID;
    }
    for (int64_t i = 0; i < n_edges; ++i) {
        const int64_t u = edges[2 * i], v = edges[2 * i + 1];
        if (u < 0 || u >= n || v < 0 || v >= n) {
            g_qual_error = "edge " + std::to_string(i) + " has a vertex id outside [0, n)";
            return GH_ERR_INVALID;
        }
    }
    gh_qual *h = new gh_qual();
    h->n = n;
    h->E = n_edges;
    gh_status st = GH_OK;
    if (device_id < 0) {
        h->h_edges.resize((size_t)n_edges);
        for (int64_t i = 0; i < n_edges; ++i) h->h_edges[i] = make_int2(edges[2 * i], edges[2 * i + 1]);
    } else {
        st = gh_host_open(h, device_id, &g_qual_error);
        if (st == GH_OK) {
            st = [&]() -> gh_status {
                if (!h->d_edges.alloc(8 * (size_t)n_edges) || !h->d_seg.alloc(16 * (size_t)n_edges)) {
                    h->err = "hipMalloc failed for " + std::to_string(24 * n_edges) + " bytes of segment table";
                    return GH_ERR_NOMEM;
                }
                if (n_edges) GH_HIP(hipMemcpyAsync(h->d_edges.p, edges, 8 * (size_t)n_edges, hipMemcpyHostToDevice, h->stream));
                GH_HIP(hipStreamSynchronize(h->stream));
                return GH_OK;
            }();
            if (st != GH_OK) g_qual_error = h->err;
        }
    }
    if (st != GH_OK) { gh_qual_destroy(h); return st; }
    *out = h;
    return GH_OK;
}

extern "C" void gh_qual_destroy(gh_qual_handle h) {
    if (!h) return;
    gh_host_close(h);
    delete h;
}

extern "C" const char *gh_qual_last_error(gh_qual_handle h) { return h ? h->err.c_str() : g_qual_error.c_str(); }

extern "C" gh_status gh_qual_set_positions(gh_qual_handle h, const float *pos, int32_t D, int64_t ld, int32_t on_device) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (D < 1) return qual_invalid(h, "D must be at least 1, got " + std::to_string(D));
    if (ld < D) return qual_invalid(h, "ld = " + std::to_string(ld) + " is below D = " + std::to_string(D));
    if (!pos && h->n > 0) return qual_invalid(h, "pos is NULL");
    if (on_device && h->device < 0) return qual_invalid(h, "a host-path handle takes host positions only");
    const int64_t n = h->n, total = n * D;
    if (h->device < 0) {
        h->h_pos.resize((size_t)total);
        for (int64_t i = 0; i < n; ++i) std::copy(pos + i * ld, pos + i * ld + D, h->h_pos.begin() + i * D);
        h->h_seg.resize((size_t)h->E);
        for (int64_t e = 0; e < h->E; ++e) h->h_seg[e] = qual_segment(h->h_pos.data(), D, D, h->h_edges[e]);
        h->D = D;
        return GH_OK;
    }
    GH_HIP(hipSetDevice(h->device));
    h->D = 0;   // a failure below leaves no snapshot
    if (4 * (size_t)total != h->pos_bytes || !h->d_pos.p) {
        if (!h->d_pos.alloc(4 * (size_t)total)) { h->pos_bytes = 0; h->err = "hipMalloc failed for " + std::to_string(4 * total) + " bytes of positions"; return GH_ERR_NOMEM; }
        h->pos_bytes = 4 * (size_t)total;
    }
    std::vector<float> packed;
    if (total > 0) {
        if (on_device) {
            if (ld == D) GH_HIP(hipMemcpyAsync(h->d_pos.p, pos, 4 * (size_t)total, hipMemcpyDeviceToDevice, h->stream));
            else {
                qual_pack_kernel<<<dim3(qual_grid(total)), dim3(QUAL_BLOCK), 0, h->stream>>>(total, D, ld, pos, h->d_pos.p);
                GH_LAUNCH_CHECK();
            }
        } else {
            const float *src = pos;
            if (ld != D) {
                packed.resize((size_t)total);
                for (int64_t i = 0; i < n; ++i) std::copy(pos + i * ld, pos + i * ld + D, packed.begin() + i * D);
                src = packed.data();
            }
            GH_HIP(hipMemcpyAsync(h->d_pos.p, src, 4 * (size_t)total, hipMemcpyHostToDevice, h->stream));
        }
    }
    if (h->E > 0) {
        qual_segments_kernel<<<dim3(qual_grid(h->E)), dim3(QUAL_BLOCK), 0, h->stream>>>(h->E, h->d_edges.p, h->d_pos.p, D, h->d_seg.p);
        GH_LAUNCH_CHECK();
    }
    GH_HIP(hipStreamSynchronize(h->stream));   // the caller's buffer is free again: an engine may go on
    h->D = D;
    return GH_OK;
}

extern "C" gh_status gh_qual_crossings(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int32_t *counts, int64_t *sum) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (!rows) n_rows = h->E;
    if (n_rows < 0) return qual_invalid(h, "n_rows must be >= 0, got " + std::to_string(n_rows));
    if (n_rows > 0 && !counts) return qual_invalid(h, "counts is NULL");
    for (int64_t r = 0; rows && r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= h->E) return qual_invalid(h, "row " + std::to_string(r) + " has an edge id outside [0, E)");
    if (h->D < 2) std::fill(counts, counts + n_rows, 0);
    else if (n_rows > 0) {
        if (h->device < 0) qual_crossings_host(h, n_rows, rows, counts);
        else GH_TRY_ST(qual_crossings_device(h, n_rows, rows, counts));
    }
    if (sum) {
        int64_t s = 0;
        for (int64_t r = 0; r < n_rows; ++r) s += counts[r];
        *sum = s;
    }
    return GH_OK;
}

extern "C" gh_status gh_qual_pairs(gh_qual_handle h, int64_t n_pairs, const int32_t *pairs, uint8_t *cross) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (n_pairs < 0) return qual_invalid(h, "n_pairs must be >= 0, got " + std::to_string(n_pairs));
    if (n_pairs > 0 && (!pairs || !cross)) return qual_invalid(h, "pairs or cross is NULL");
    for (int64_t p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= h->E) return qual_invalid(h, "pair " + std::to_string(p / 2) + " has an edge id outside [0, E)");
    if (n_pairs == 0) return GH_OK;
    if (h->device < 0) {
        for (int64_t p = 0; p < n_pairs; ++p) {
            const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
            cross[p] = (uint8_t)(h->D >= 2 && i != j ? qual_cross(h->h_seg[i], h->h_edges[i], h->h_seg[j], h->h_edges[j]) : 0);
        }
        return GH_OK;
    }
    GH_HIP(hipSetDevice(h->device));
    gh_dev<int2> d_pairs;
    gh_dev<uint8_t> d_cross;
    if (!d_pairs.alloc(8 * (size_t)n_pairs) || !d_cross.alloc((size_t)n_pairs)) {
        h->err = "hipMalloc failed for " + std::to_string(9 * n_pairs) + " bytes of pairs";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_pairs.p, pairs, 8 * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream));
    qual_pairs_kernel<<<dim3(qual_grid(n_pairs)), dim3(QUAL_BLOCK), 0, h->stream>>>(n_pairs, d_pairs.p, h->d_seg.p, h->d_edges.p, h->D, d_cross.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(cross, d_cross.p, (size_t)n_pairs, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_qual_edge_lengths(gh_qual_handle h, double out[4]) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (!out) return qual_invalid(h, "out is NULL");
    qual_len all = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), 0.0, 0.0};
    if (h->device < 0) {
        for (int64_t e = 0; e < h->E; ++e) {
            const double L = qual_length(h->h_pos.data(), h->D, h->D, h->h_edges[e]);
            const qual_len one = {L, L, L, L * L};
            qual_len_join(all, one);
        }
    } else if (h->E > 0) {
        GH_HIP(hipSetDevice(h->device));
        const unsigned blocks = (unsigned)std::min<int64_t>(QUAL_LEN_BLOCKS, qual_grid(h->E));
        gh_dev<double> d_part;
        if (!d_part.alloc(32 * (size_t)blocks)) { h->err = "hipMalloc failed for the length partials"; return GH_ERR_NOMEM; }
        qual_length_kernel<<<dim3(blocks), dim3(QUAL_BLOCK), 0, h->stream>>>(h->E, h->d_edges.p, h->d_pos.p, h->D, d_part.p);
        GH_LAUNCH_CHECK();
        std::vector<double> part(4 * (size_t)blocks);
        GH_HIP(hipMemcpyAsync(part.data(), d_part.p, 32 * (size_t)blocks, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
        for (unsigned b = 0; b < blocks; ++b) {
            const qual_len one = {part[4 * b], part[4 * b + 1], part[4 * b + 2], part[4 * b + 3]};
            qual_len_join(all, one);
        }
    }
    out[0] = all.mn; out[1] = all.mx; out[2] = all.s; out[3] = all.ss;
    return GH_OK;
}

extern "C" gh_status gh_qual_neighbor_sizes(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int64_t *indptr) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (!indptr) return qual_invalid(h, "indptr is NULL");
    GH_TRY_ST(qual_rank_rows(h, &n_rows, rows));
    indptr[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t u = rows ? rows[r] : r;
        indptr[r + 1] = indptr[r] + (h->g_ptr[u + 1] - h->g_ptr[u]);
    }
    return GH_OK;
}

extern "C" gh_status gh_qual_neighbor_ranks(gh_qual_handle h, int64_t n_rows, const int32_t *rows, int32_t *neighbors, float *d2,
                                            int32_t *below, int32_t *equal) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    GH_TRY_ST(qual_rank_rows(h, &n_rows, rows));
    std::vector<int64_t> indptr((size_t)n_rows + 1, 0);
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t u = rows ? rows[r] : r;
        indptr[r + 1] = indptr[r] + (h->g_ptr[u + 1] - h->g_ptr[u]);
    }
    const int64_t slots = indptr[n_rows];
    if (slots == 0) return GH_OK;
    if (!neighbors || !d2 || !below || !equal) return qual_invalid(h, "neighbors, d2, below or equal is NULL");
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t u = rows ? rows[r] : r;
        std::copy(h->g_idx.begin() + h->g_ptr[u], h->g_idx.begin() + h->g_ptr[u + 1], neighbors + indptr[r]);
    }
    if (h->device < 0) qual_ranks_host(h, n_rows, rows, indptr.data(), neighbors, d2, below, equal);
    else GH_TRY_ST(qual_ranks_device(h, n_rows, rows, indptr.data(), neighbors, d2, below, equal));
    return GH_OK;
}
