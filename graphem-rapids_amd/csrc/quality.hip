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
//   qual_hop_level_kernel  distance preservation ("distance preservation" in the header): one level of a breadth-first search
//                          from 64 sources to a machine word; where a source first reaches a vertex the pair's distance goes
//                          onto lane-local sums for the hop and LDS sums for the source; one slab of partials per workgroup.
//                          qual_hop_reduce_kernel adds the slabs in a fixed order: no float atomic touches global memory.
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
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "frontier_core.h"   // with csr_core.h: gs_flag, GS_GRID_LOOP
#include "host_util.h"
#include "intersect_core.h"
#include "qual_handle.h"   // struct gh_qual, QUAL_BLOCK, qual_d2, qual_host_parallel: shared with clusters.hip

#define QUAL_TILE 1024                      // column segments staged at once: 24 KiB of LDS
#define QUAL_LAUNCH_PAIRS (1ll << 36)       // pair tests per launch: rows are taken in batches of about a second
#define QUAL_LAUNCH_ROWS (1ll << 22)
#define QUAL_MIN_BLOCKS 2048                // fewer row blocks than this: the column tiles are split over gridDim.y
#define QUAL_LEN_BLOCKS 1024
#define QUAL_RANK_PIECE 64                  // slots of one source that one wave owns: lane i keeps threshold i (at most 64)
#define QUAL_RANK_WAVES (QUAL_BLOCK / 64)   // pieces per workgroup: they share the staged position tile
#define QUAL_RANK_LDS 8192                  // floats of the position tile, D rows of tile_cols columns: 32 KiB
#define QUAL_RANK_TILE 1024                 // columns of a tile at most; fewer when D * 1024 floats do not fit
#define QUAL_RANK_LAUNCH_PAIRS (1ll << 40)  // (piece, column) pairs per launch: pieces are taken in batches of about a second
#define QUAL_RANK_LAUNCH_ITEMS (1ll << 22)
#define QUAL_HOP_SRC_LDS 8192               // floats of a group's 64 staged source rows: 32 KiB, D <= 128
#define QUAL_HOP_MAX_BLOCKS 2048            // workgroups of one level launch, over all groups of the batch
#define QUAL_HOP_STATE_BYTES (1ll << 30)    // visited, frontier and next frontier of the groups in flight: 24 n bytes a group
#define QUAL_HOP_CHECK_EVERY 4              // levels between two host reads of the flags

static_assert(QUAL_BLOCK == GS_BLOCK, "GS_GRID_LOOP and the frontier kernels stride by GS_BLOCK");

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
    GS_GRID_LOOP(e, E) {
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
// The distance is qual_d2 (qual_handle.h), the exact-difference chain of the header.

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

// ---- distance preservation ------------------------------------------------------------------------------------------
typedef unsigned long long qual_u64;

// What the pairs of one hop add up to.  mn and mx are the float's bit pattern, which orders the floats d2 can be without a
// NaN (+0 .. +inf) as the values do.
struct qual_hop {
    qual_u64 pairs;
    double sd, sq;
    uint32_t mn, mx;
};

__host__ __device__ __forceinline__ qual_hop qual_hop_empty() { return {0, 0.0, 0.0, 0xFFFFFFFFu, 0u}; }

__host__ __device__ __forceinline__ void qual_hop_join(qual_hop &a, const qual_hop &b) {
    a.pairs += b.pairs;
    a.sd += b.sd;
    a.sq += b.sq;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
}

// One pair at squared distance d2: q = (double)d2 and d = sqrt(q), an IEEE double square root; *d_out = d.
__host__ __device__ __forceinline__ void qual_hop_pair(qual_hop &a, float d2, double *d_out) {
    union { float f; uint32_t u; } bits = {d2};
    const double q = (double)d2, d = sqrt(q);
    const qual_hop one = {1, d, q, bits.u, bits.u};
    qual_hop_join(a, one);
    *d_out = d;
}

struct QualHopLevel {
    const int64_t *ptr; const int32_t *idx;   // the simple graph
    const float *pos;
    const int32_t *src;                       // the batch's source ids, 64 per group; the unused slots of the last group hold 0
    uint64_t *vis; const uint64_t *cur; uint64_t *nxt;
    int32_t *flags;                           // flags[L] = 1: level L reached something
    double *lvl_f; qual_u64 *lvl_i;           // per workgroup: (sum d, sum q) and (pairs, min bits, max bits) of this level
    double *src_f; uint32_t *src_c;           // per workgroup: 2 x 64 sums and 64 counts, one per source of the group
    int64_t n;
    int32_t D, level;
};

// One level of the bit-parallel search (frontier_core.h), grid (x, G): the waves of row g stride over the vertices, 64 at a
// time, lane = vertex; gs_frontier_pull gives the vertex's word of new bits.  A lane whose word is not empty walks them:
// bit b is the pair (source 64 g + b, v) at hop `level`, met here and
// never again.  Per hop the lane keeps the five accumulators in registers; per source the workgroup adds in LDS.  Both
// leave the workgroup as one slab of partials -- every workgroup writes its slab, zeros included -- and
// qual_hop_reduce_kernel adds the slabs in a fixed order.  STAGED: the group's 64 source rows are read from LDS.
template <bool STAGED>
__global__ __launch_bounds__(QUAL_BLOCK) void qual_hop_level_kernel(QualHopLevel a) {
    __shared__ float s_src[STAGED ? QUAL_HOP_SRC_LDS : 1];
    __shared__ double s_sum[2][64];
    __shared__ uint32_t s_cnt[64];
    __shared__ int32_t s_id[64];
    __shared__ qual_hop s_w[QUAL_BLOCK / 64];
    if (gs_flag(&a.flags[a.level - 1]) == 0) return;   // the search ended before this level: the same for every thread
    const int lane = threadIdx.x & 63, D = a.D;
    const int64_t g = blockIdx.y, off = g * a.n;
    uint64_t *vis = a.vis + off, *nxt = a.nxt + off;
    const uint64_t *cur = a.cur + off;
    if (threadIdx.x < 64) {
        s_sum[0][threadIdx.x] = 0.0;
        s_sum[1][threadIdx.x] = 0.0;
        s_cnt[threadIdx.x] = 0;
        s_id[threadIdx.x] = a.src[g * 64 + threadIdx.x];
    }
    if (STAGED)
        for (int i = threadIdx.x; i < 64 * D; i += QUAL_BLOCK) s_src[i] = a.pos[(int64_t)a.src[g * 64 + i / D] * D + i % D];
    __syncthreads();
    qual_hop acc = qual_hop_empty();
    const int64_t stride = (int64_t)gridDim.x * QUAL_BLOCK;
    for (int64_t base = (int64_t)blockIdx.x * QUAL_BLOCK + (threadIdx.x & ~63); base < a.n; base += stride) {
        const int64_t v = base + lane;
        const uint64_t w = v < a.n ? gs_frontier_pull(a.ptr, a.idx, vis, cur, nxt, v) : 0;
        if (w == 0) continue;
        const float *xv = a.pos + v * D;
        // lane l starts its walk at bit l: where the words are dense the lanes of a wave add to 64 different LDS words
        uint64_t rot = (w >> lane) | (w << ((64 - lane) & 63));
        while (rot) {
            const int b = (__ffsll((long long)rot) - 1 + lane) & 63;
            rot &= rot - 1;
            const float *xs = STAGED ? s_src + b * D : a.pos + (int64_t)s_id[b] * D;
            const float d2 = qual_d2(xs, xv, 1, D);
            double d;
            qual_hop_pair(acc, d2, &d);
            atomicAdd(&s_sum[0][b], d);
            atomicAdd(&s_sum[1][b], (double)d2);
            atomicAdd(&s_cnt[b], 1u);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const qual_hop other = {__shfl_down(acc.pairs, o, 64), __shfl_down(acc.sd, o, 64), __shfl_down(acc.sq, o, 64),
                                __shfl_down(acc.mn, o, 64), __shfl_down(acc.mx, o, 64)};
        qual_hop_join(acc, other);
    }
    if (lane == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();   // the wave partials and every wave's LDS adds
    const int64_t slab = g * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < QUAL_BLOCK / 64; ++wv) qual_hop_join(acc, s_w[wv]);
        a.lvl_f[2 * slab] = acc.sd;
        a.lvl_f[2 * slab + 1] = acc.sq;
        a.lvl_i[3 * slab] = acc.pairs;
        a.lvl_i[3 * slab + 1] = acc.mn;
        a.lvl_i[3 * slab + 2] = acc.mx;
        if (acc.pairs && gs_flag(&a.flags[a.level]) == 0) a.flags[a.level] = 1;
    }
    if (threadIdx.x < 64) {
        a.src_f[(2 * slab) * 64 + threadIdx.x] = s_sum[0][threadIdx.x];
        a.src_f[(2 * slab + 1) * 64 + threadIdx.x] = s_sum[1][threadIdx.x];
        a.src_c[slab * 64 + threadIdx.x] = s_cnt[threadIdx.x];
    }
}

struct QualHopReduce {
    const int32_t *flags;
    const double *lvl_f; const qual_u64 *lvl_i; const double *src_f; const uint32_t *src_c;   // the slabs of G rows of X workgroups
    double *hop_f; qual_u64 *hop_i;           // per hop L, over all batches: (sum d, sum q) at 2 L, (pairs, min bits, max bits) at 3 L
    qual_u64 *reach; int32_t *ecc;            // per source of the batch
    double *over_h, *over_h2;
    int64_t X, G;
    int32_t level;
};

// Adds the slabs of one level in a fixed order.  Workgroup g < G: the 64 sources of group g, the X slabs taken by four
// stripes of threads and the stripes joined in order, then sum d / L and sum q / L^2 go onto the source's totals.
// Workgroup G: the level's five values over all G X slabs, strided over the threads and joined in thread order.
__global__ __launch_bounds__(QUAL_BLOCK) void qual_hop_reduce_kernel(QualHopReduce a) {
    __shared__ double s_f[2][QUAL_BLOCK];
    __shared__ qual_u64 s_c[QUAL_BLOCK];
    __shared__ qual_hop s_h[QUAL_BLOCK];
    if (gs_flag(&a.flags[a.level]) == 0) return;   // nothing was reached at this level, or its launch returned at once
    const int t = threadIdx.x;
    if ((int64_t)blockIdx.x < a.G) {
        const int64_t g = blockIdx.x;
        const int b = t & 63;
        double fa = 0.0, fb = 0.0;
        qual_u64 c = 0;
        for (int64_t x = t >> 6; x < a.X; x += QUAL_BLOCK / 64) {
            const int64_t slab = g * a.X + x;
            fa += a.src_f[(2 * slab) * 64 + b];
            fb += a.src_f[(2 * slab + 1) * 64 + b];
            c += a.src_c[slab * 64 + b];
        }
        s_f[0][t] = fa;
        s_f[1][t] = fb;
        s_c[t] = c;
        __syncthreads();
        if (t >= 64) return;
        for (int q = 1; q < QUAL_BLOCK / 64; ++q) {
            fa += s_f[0][64 * q + t];
            fb += s_f[1][64 * q + t];
            c += s_c[64 * q + t];
        }
        if (c == 0) return;
        const int64_t j = g * 64 + t;
        const double L = (double)a.level;
        a.reach[j] += c;
        a.ecc[j] = a.level;   // levels ascend
        a.over_h[j] += fa / L;
        a.over_h2[j] += fb / (L * L);
        return;
    }
    qual_hop v = qual_hop_empty();
    for (int64_t slab = t; slab < a.G * a.X; slab += QUAL_BLOCK) {
        const qual_hop one = {a.lvl_i[3 * slab], a.lvl_f[2 * slab], a.lvl_f[2 * slab + 1], (uint32_t)a.lvl_i[3 * slab + 1],
                              (uint32_t)a.lvl_i[3 * slab + 2]};
        qual_hop_join(v, one);
    }
    s_h[t] = v;
    __syncthreads();
    if (t != 0) return;
    for (int k = 1; k < QUAL_BLOCK; ++k) qual_hop_join(v, s_h[k]);
    // an earlier batch may have been here: its entry joins; an entry nobody reached yet is all zeros
    const int64_t L = a.level;
    const qual_hop old = {a.hop_i[3 * L], a.hop_f[2 * L], a.hop_f[2 * L + 1], (uint32_t)a.hop_i[3 * L + 1], (uint32_t)a.hop_i[3 * L + 2]};
    if (old.pairs) qual_hop_join(v, old);
    a.hop_f[2 * L] = v.sd;
    a.hop_f[2 * L + 1] = v.sq;
    a.hop_i[3 * L] = v.pairs;
    a.hop_i[3 * L + 1] = v.mn;
    a.hop_i[3 * L + 2] = v.mx;
}

}  // namespace

static thread_local std::string g_qual_error;

void qual_set_create_error(const std::string &msg) { g_qual_error = msg; }

namespace {

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
    gh_csr_from_keys(h->n, keys, GH_CSR_SYMMETRIC, &h->g_ptr, &h->g_idx);
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

// What both paths of the hop profile fill: hops[h - 1] for h = 1 .. H, and one entry per source.
struct qual_hop_result {
    std::vector<qual_hop> hops;
    std::vector<int64_t> reach;
    std::vector<int32_t> ecc;
    std::vector<double> over_h, over_h2;
};

// One breadth-first search per source; a thread keeps the sums of its sources per hop, and the threads join in order.
void qual_hops_host(const gh_qual *h, int64_t S, const int32_t *src, qual_hop_result *out) {
    const int64_t n = h->n;
    const int D = h->D;
    const float *pos = h->h_pos.data();
    const int64_t *ptr = h->g_ptr.data();
    const int32_t *idx = h->g_idx.data();
    std::mutex mu;
    std::map<int64_t, std::vector<qual_hop>> parts;   // by the thread's first source: thread order
    qual_host_parallel(S, 1, [&, n, D, pos, ptr, idx, src, out](int64_t first, int64_t last) {
        std::vector<qual_hop> mine;
        std::vector<int32_t> dist((size_t)n), queue;
        for (int64_t j = first; j < last; ++j) {
            const int32_t s = src[j];
            const float *xs = pos + (int64_t)s * D;
            std::fill(dist.begin(), dist.end(), -1);
            dist[s] = 0;
            queue.assign(1, s);
            double over_h = 0.0, over_h2 = 0.0;
            int64_t reach = 0;
            int32_t level = 0;
            for (size_t head = 0; head < queue.size();) {
                const size_t tail = queue.size();   // queue[head .. tail) is the frontier at `level`
                ++level;
                qual_hop acc = qual_hop_empty();
                for (; head < tail; ++head) {
                    const int32_t u = queue[head];
                    for (int64_t k = ptr[u]; k < ptr[u + 1]; ++k) {
                        const int32_t v = idx[k];
                        if (dist[v] >= 0) continue;
                        dist[v] = level;
                        queue.push_back(v);
                        double d;
                        qual_hop_pair(acc, qual_d2(xs, pos + (int64_t)v * D, 1, D), &d);
                    }
                }
                if (acc.pairs == 0) { --level; break; }
                if (mine.size() < (size_t)level) mine.resize((size_t)level, qual_hop_empty());
                qual_hop_join(mine[(size_t)level - 1], acc);
                const double L = (double)level;
                over_h += acc.sd / L;
                over_h2 += acc.sq / (L * L);
                reach += (int64_t)acc.pairs;
            }
            out->reach[j] = reach;
            out->ecc[j] = level;
            out->over_h[j] = over_h;
            out->over_h2[j] = over_h2;
        }
        std::lock_guard<std::mutex> lock(mu);
        parts[first] = std::move(mine);
    });
    for (auto &part : parts) {
        if (out->hops.size() < part.second.size()) out->hops.resize(part.second.size(), qual_hop_empty());
        for (size_t l = 0; l < part.second.size(); ++l) qual_hop_join(out->hops[l], part.second[l]);
    }
}

gh_status qual_hops_device(gh_qual *h, int64_t S, const int32_t *src, qual_hop_result *out) {
    const int64_t n = h->n, groups = (S + 63) / 64;
    GH_HIP(hipSetDevice(h->device));
    if (!h->d_gptr.p) {   // once per handle
        if (!h->d_gptr.alloc(8 * (size_t)(n + 1)) || !h->d_gidx.alloc(4 * h->g_idx.size())) {
            h->d_gptr.reset();
            h->err = "hipMalloc failed for " + std::to_string(8 * (n + 1) + 4 * (int64_t)h->g_idx.size()) + " bytes of graph";
            return GH_ERR_NOMEM;
        }
        GH_HIP(hipMemcpyAsync(h->d_gptr.p, h->g_ptr.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, h->stream));
        if (!h->g_idx.empty()) GH_HIP(hipMemcpyAsync(h->d_gidx.p, h->g_idx.data(), 4 * h->g_idx.size(), hipMemcpyHostToDevice, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    // G groups in flight, X workgroups to a group
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>({QUAL_HOP_STATE_BYTES / (24 * n), groups, (int64_t)65535}));   // 65535: grid.y
    const int64_t X = std::max<int64_t>(1, std::min<int64_t>((n + QUAL_BLOCK - 1) / QUAL_BLOCK, QUAL_HOP_MAX_BLOCKS / G));
    std::vector<int32_t> padded(64 * (size_t)groups, 0);   // the unused slots of the last group name vertex 0: a row that exists
    std::copy(src, src + S, padded.begin());
    gs_frontier f;
    gh_dev<int32_t> d_src, d_ecc;
    gh_dev<double> d_lvl_f, d_src_f, d_hop_f, d_over;
    gh_dev<qual_u64> d_lvl_i, d_hop_i, d_reach;
    gh_dev<uint32_t> d_src_c;
    const size_t slabs = (size_t)(G * X), per_src = 64 * (size_t)groups;
    if (!f.alloc(G, n) || !d_src.alloc(4 * per_src) ||
        !d_lvl_f.alloc(16 * slabs) || !d_lvl_i.alloc(24 * slabs) || !d_src_f.alloc(1024 * slabs) || !d_src_c.alloc(256 * slabs) ||
        !d_hop_f.alloc(16 * (size_t)n) || !d_hop_i.alloc(24 * (size_t)n) || !d_reach.alloc(8 * per_src) || !d_ecc.alloc(4 * per_src) ||
        !d_over.alloc(16 * per_src)) {
        h->err = "hipMalloc failed for " + std::to_string(G) + " source groups of search state";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_src.p, padded.data(), 4 * per_src, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemsetAsync(d_hop_f.p, 0, 16 * (size_t)n, h->stream));
    GH_HIP(hipMemsetAsync(d_hop_i.p, 0, 24 * (size_t)n, h->stream));
    GH_HIP(hipMemsetAsync(d_reach.p, 0, 8 * per_src, h->stream));
    GH_HIP(hipMemsetAsync(d_ecc.p, 0, 4 * per_src, h->stream));
    GH_HIP(hipMemsetAsync(d_over.p, 0, 16 * per_src, h->stream));
    const bool staged = 64 * (int64_t)h->D <= QUAL_HOP_SRC_LDS;
    QualHopLevel lv{};
    lv.ptr = h->d_gptr.p; lv.idx = h->d_gidx.p; lv.pos = h->d_pos.p;
    lv.vis = f.vis.p; lv.flags = f.flags.p;
    lv.lvl_f = d_lvl_f.p; lv.lvl_i = d_lvl_i.p; lv.src_f = d_src_f.p; lv.src_c = d_src_c.p;
    lv.n = n; lv.D = h->D;
    QualHopReduce rd{};
    rd.flags = f.flags.p;
    rd.lvl_f = d_lvl_f.p; rd.lvl_i = d_lvl_i.p; rd.src_f = d_src_f.p; rd.src_c = d_src_c.p;
    rd.hop_f = d_hop_f.p; rd.hop_i = d_hop_i.p;
    rd.X = X;
    int32_t H = 0;
    for (int64_t g0 = 0; g0 < groups; g0 += G) {
        const int64_t gb = std::min(G, groups - g0), ns = std::min<int64_t>(64 * gb, S - 64 * g0);
        GH_TRY_ST(f.begin(h, gb, ns, d_src.p + 64 * g0, QUAL_HOP_MAX_BLOCKS));
        lv.src = d_src.p + 64 * g0;
        rd.G = gb;
        rd.reach = d_reach.p + 64 * g0; rd.ecc = d_ecc.p + 64 * g0;
        rd.over_h = d_over.p + 64 * g0; rd.over_h2 = d_over.p + per_src + 64 * g0;
        const dim3 grid((unsigned)X, (unsigned)gb);
        int32_t last = 0;
        GH_TRY_ST(gh_level_loop(h, n, f.flags.p, QUAL_HOP_CHECK_EVERY, &last, [&](int32_t L) -> gh_status {
            lv.level = rd.level = L;
            lv.cur = f.cur(L);
            lv.nxt = f.nxt(L);
            if (staged) qual_hop_level_kernel<true><<<grid, dim3(QUAL_BLOCK), 0, h->stream>>>(lv);
            else qual_hop_level_kernel<false><<<grid, dim3(QUAL_BLOCK), 0, h->stream>>>(lv);
            GH_LAUNCH_CHECK();
            qual_hop_reduce_kernel<<<dim3((unsigned)gb + 1), dim3(QUAL_BLOCK), 0, h->stream>>>(rd);
            GH_LAUNCH_CHECK();
            return GH_OK;
        }));
        H = std::max(H, last);
    }
    std::vector<double> hop_f(2 * (size_t)H + 2), over(2 * per_src);
    std::vector<qual_u64> hop_i(3 * (size_t)H + 3), reach(per_src);
    if (H > 0) {   // entry L of the device arrays is hop L; entry 0 is unused
        GH_HIP(hipMemcpyAsync(hop_f.data(), d_hop_f.p, 16 * ((size_t)H + 1), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipMemcpyAsync(hop_i.data(), d_hop_i.p, 24 * ((size_t)H + 1), hipMemcpyDeviceToHost, h->stream));
    }
    GH_HIP(hipMemcpyAsync(reach.data(), d_reach.p, 8 * per_src, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(out->ecc.data(), d_ecc.p, 4 * (size_t)S, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(over.data(), d_over.p, 16 * per_src, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    out->hops.resize((size_t)H);
    for (int64_t L = 1; L <= H; ++L)
        out->hops[(size_t)L - 1] = {hop_i[3 * L], hop_f[2 * L], hop_f[2 * L + 1], (uint32_t)hop_i[3 * L + 1], (uint32_t)hop_i[3 * L + 2]};
    for (int64_t j = 0; j < S; ++j) {
        out->reach[j] = (int64_t)reach[j];
        out->over_h[j] = over[j];
        out->over_h2[j] = over[per_src + j];
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
    h->epoch += 1;   // what clusters.hip keeps about the old snapshot is void
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

extern "C" gh_status gh_qual_hop_profile(gh_qual_handle h, int64_t n_sources, const int32_t *sources, int64_t hop_cap, int64_t *n_hops,
                                         int64_t *pairs, double *sum_d, double *sum_d2, float *min_d2, float *max_d2, int64_t *reach,
                                         int32_t *eccentricity, double *sum_d_over_h, double *sum_d2_over_h2) {
    if (!h) { g_qual_error = "handle is NULL"; return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (!sources) n_sources = h->n;
    if (n_sources < 0) return qual_invalid(h, "n_sources must be >= 0, got " + std::to_string(n_sources));
    if (hop_cap < 0) return qual_invalid(h, "hop_cap must be >= 0, got " + std::to_string(hop_cap));
    for (int64_t j = 0; sources && j < n_sources; ++j)
        if (sources[j] < 0 || sources[j] >= h->n) return qual_invalid(h, "source " + std::to_string(j) + " has a vertex id outside [0, n)");
    GH_TRY_ST(qual_build_graph(h));
    const int64_t S = n_sources;
    std::vector<int32_t> all;
    if (!sources) {
        all.resize((size_t)S);
        for (int64_t j = 0; j < S; ++j) all[j] = (int32_t)j;
        sources = all.data();
    }
    qual_hop_result r;
    r.reach.assign((size_t)S, 0);
    r.ecc.assign((size_t)S, 0);
    r.over_h.assign((size_t)S, 0.0);
    r.over_h2.assign((size_t)S, 0.0);
    if (S > 0) {
        if (h->device < 0) qual_hops_host(h, S, sources, &r);
        else GH_TRY_ST(qual_hops_device(h, S, sources, &r));
    }
    const int64_t H = (int64_t)r.hops.size();
    if (n_hops) *n_hops = H;
    if ((pairs || sum_d || sum_d2 || min_d2 || max_d2) && hop_cap < H)
        return qual_invalid(h, "hop_cap = " + std::to_string(hop_cap) + " is below the greatest hop " + std::to_string(H));
    for (int64_t l = 0; l < H; ++l) {
        union { uint32_t u; float f; } mn = {r.hops[l].mn}, mx = {r.hops[l].mx};
        if (pairs) pairs[l] = (int64_t)r.hops[l].pairs;
        if (sum_d) sum_d[l] = r.hops[l].sd;
        if (sum_d2) sum_d2[l] = r.hops[l].sq;
        if (min_d2) min_d2[l] = mn.f;
        if (max_d2) max_d2[l] = mx.f;
    }
    if (reach) std::copy(r.reach.begin(), r.reach.end(), reach);
    if (eccentricity) std::copy(r.ecc.begin(), r.ecc.end(), eccentricity);
    if (sum_d_over_h) std::copy(r.over_h.begin(), r.over_h.end(), sum_d_over_h);
    if (sum_d2_over_h2) std::copy(r.over_h2.begin(), r.over_h2.end(), sum_d2_over_h2);
    return GH_OK;
}
