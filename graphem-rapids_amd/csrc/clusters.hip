// Clusters of an embedding (include/graphem_hip.h "embedding clusters"): exact k-means on the position snapshot of a gh_qual
// handle, the running minimum k-means++ draws from, and the per-cluster distance sums under the silhouette.
//
// The rule is the header's: the distance is qual_d2 (qual_handle.h), the assignment takes the least centre id among the
// nearest, and a centre is the quotient of an INTEGER sum of quantised coordinates by the member count.  Integer adds
// commute, so the labels and the centre bits depend on nothing but (positions, start centres, max_iter): the kernels and
// the host path (device_id < 0) run the same functions and give the same bits.
//
//   cl_scan_kernel      once per snapshot: the greatest |x| (its float32 bits, by an integer max) and the first row that
//                       holds a NaN or an infinity (by an integer min)
//   cl_lloyd_kernel     one Lloyd iteration in one launch: a thread keeps one vertex's row in registers (D = 2 .. 16; other
//                       D read the row from memory), the workgroup stages the centres through LDS in tiles and every lane
//                       reads the same centre word (a broadcast); the same thread adds its quantised row to int64 bins and
//                       counts itself, and counts a label that differs from the previous one.  While k (D + 1) <=
//                       CL_BIN_SLOTS the bins are in LDS and leave the workgroup as one 64-bit global atomic per non-zero
//                       bin; above that every thread adds to the global bins.  Either way the sums are the same integers.
//                       At most CL_LLOYD_BLOCKS workgroups stride over the vertices and each flushes once, after its last
//                       vertex, so that few of them add to the same global words.
//   cl_finish_kernel    sums and counts -> centres; clears the sums
//   cl_seed_kernel      min_d2[w] = min(min_d2[w], d2(x_w, x_vertex))
//   cl_gather_kernel    the columns in cluster order: after a counting sort by label a cluster is one contiguous segment
//   cl_sums_kernel      all pairs (row, column): a wave owns one row, the workgroup walks the column tiles through LDS as
//                       qual_rank_kernel does, and per PIECE -- the part of one cluster's segment inside one tile -- the wave
//                       adds sqrt((double)d2) in double, lanes striding the columns, then a shuffle tree: one double per
//                       (row, piece), no atomics
//   cl_join_kernel      adds the pieces of a cluster that tile boundaries cut, in piece order
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "dispatch.h"
#include "host_util.h"
#include "qual_handle.h"

#define CL_MAX_K 4096
#define CL_MAX_N (1ll << 24)                // |q| <= 2^39: an int64 sum over more members could overflow
#define CL_CENTRE_LDS 4096                  // floats of a staged centre tile: 16 KiB
#define CL_LLOYD_BLOCKS 1024                // workgroups of a Lloyd launch at most, four to a compute unit: they stride over the vertices
#define CL_BIN_SLOTS 2048                   // int64 bins of a workgroup, k (D + 1) of them (D sums and a count a cluster): 16 KiB
#define CL_SUMS_WAVES (QUAL_BLOCK / 64)     // rows per workgroup of cl_sums_kernel: they share the staged column tile
#define CL_SUMS_LDS 8192                    // floats of the column tile, D rows of tile_cols columns: 32 KiB
#define CL_SUMS_TILE 1024                   // columns of a tile at most; fewer when D * 1024 floats do not fit
#define CL_SUMS_MIN_BLOCKS 2048             // fewer row blocks than this: the column tiles are split over gridDim.y
#define CL_SUMS_PART_BYTES (1ll << 28)      // (row, piece) partial sums of one batch of rows
#define CL_SUMS_LAUNCH_PAIRS (1ll << 38)    // (row, column) pairs per launch

typedef unsigned long long cl_u64;

namespace {

// q(x) = llrint(ldexp((double)x, s)), ties to even: ldexp is exact here (|x| 2^s < 2^39, and a float's least bit times 2^s
// is far above the double's underflow), rint is the IEEE round to nearest even, and the conversion meets an integer.
__host__ __device__ __forceinline__ int64_t cl_quantise(float x, int s) { return (int64_t)rint(ldexp((double)x, s)); }

// centre = (float) ldexp((double)S / (double)count, -s): one int64 -> double conversion, one double division, an exact
// scaling, one double -> float conversion, each correctly rounded on both sides.
__host__ __device__ __forceinline__ float cl_centre(int64_t S, int64_t count, int s) {
    return (float)ldexp((double)S / (double)count, -s);
}

// Walks the centres [c0, c0 + m) upwards: a centre is taken when it is strictly nearer, so +inf and NaN never are.
template <int DT> __host__ __device__ __forceinline__ void cl_walk(const float *x, const float *cen, int D, int c0, int m, float &best,
                                                                   int32_t &label) {
    for (int c = 0; c < m; ++c) {
        const float d = DT > 0 ? qual_d2_fixed<(DT > 0 ? DT : 1)>(x, cen + (int64_t)c * DT) : qual_d2(x, cen + (int64_t)c * D, 1, D);
        if (d < best) {
            best = d;
            label = c0 + c;
        }
    }
}

__global__ __launch_bounds__(QUAL_BLOCK) void cl_scan_kernel(int64_t n, int D, const float *__restrict__ pos, uint32_t *max_bits,
                                                             cl_u64 *bad_row) {
    uint32_t mx = 0;
    cl_u64 bad = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x; i < n * D; i += (int64_t)gridDim.x * QUAL_BLOCK) {
        const uint32_t b = (uint32_t)__float_as_int(pos[i]) & 0x7FFFFFFFu;   // |x|: the bits order as the values do, NaN above inf
        if (b >= 0x7F800000u) bad = min(bad, (cl_u64)(i / D));
        else mx = max(mx, b);
    }
    if (mx) atomicMax(max_bits, mx);
    if (bad != ~0ull) atomicMin(bad_row, bad);
}

struct ClLloyd {
    const float *pos, *centres;
    const int32_t *prev;            // NULL: no previous labels
    int32_t *labels;
    float *d2;
    cl_u64 *sums, *counts;          // (k, D) and k int64 bins, two's complement
    int32_t *changed;
    int64_t n;
    int32_t D, k, tile_c, shift;
    int32_t accumulate, lds_bins, staged;
};

// A workgroup strides over the vertices, 256 at a time, thread = vertex: label and d2 of the vertex under a.centres; with
// a.accumulate also q(x_v) onto the bins of its label.  The bins and the count of changed labels leave the workgroup once,
// after its last vertex: at most CL_LLOYD_BLOCKS workgroups add to the same few global words.  All k centres in one tile:
// staged once.  DT = 0: the row is read from memory, and with a.staged = 0 (D > CL_CENTRE_LDS) the centres are too.
template <int DT>
__global__ __launch_bounds__(QUAL_BLOCK) void cl_lloyd_kernel(ClLloyd a) {
    __shared__ float s_c[CL_CENTRE_LDS];
    __shared__ cl_u64 s_bins[CL_BIN_SLOTS];
    __shared__ int32_t s_changed;
    const int D = DT > 0 ? DT : a.D, k = a.k;
    const bool staged = DT > 0 || a.staged, one_tile = a.tile_c >= k;
    const bool binned = a.accumulate && a.lds_bins;   // then k (D + 1) <= CL_BIN_SLOTS
    if (binned)
        for (int i = threadIdx.x; i < k * (D + 1); i += QUAL_BLOCK) s_bins[i] = 0;
    if (threadIdx.x == 0) s_changed = 0;
    if (staged && one_tile)
        for (int i = threadIdx.x; i < k * D; i += QUAL_BLOCK) s_c[i] = a.centres[i];   // k D <= CL_CENTRE_LDS
    __syncthreads();
    int32_t changed = 0;
    // the bounds are the workgroup's: every thread makes the same trips and meets the same barriers
    for (int64_t base = (int64_t)blockIdx.x * QUAL_BLOCK; base < a.n; base += (int64_t)gridDim.x * QUAL_BLOCK) {
        const int64_t v = base + threadIdx.x;
        const bool live = v < a.n;
        const float *row = a.pos + (live ? v : 0) * D;   // an idle thread walks row 0 and stores nothing
        float x[DT > 0 ? DT : 1];
        if (DT > 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d) x[d] = row[d];
        }
        float best = INFINITY;
        int32_t label = 0;
        for (int c0 = 0; c0 < k; c0 += a.tile_c) {
            const int m = min(a.tile_c, k - c0);   // m D <= CL_CENTRE_LDS when staged
            if (!staged) {
                cl_walk<0>(row, a.centres + (int64_t)c0 * D, D, c0, m, best, label);
                continue;
            }
            if (!one_tile) {
                __syncthreads();
                for (int i = threadIdx.x; i < m * D; i += QUAL_BLOCK) s_c[i] = a.centres[(int64_t)c0 * D + i];
                __syncthreads();
            }
            cl_walk<DT>(DT > 0 ? x : row, s_c, D, c0, m, best, label);
        }
        if (!live) continue;
        a.labels[v] = label;
        a.d2[v] = best;
        if (a.prev && a.prev[v] != label) ++changed;
        if (!a.accumulate) continue;
        for (int d = 0; d < D; ++d) {
            const cl_u64 q = (cl_u64)cl_quantise(DT > 0 ? x[DT > 0 ? d : 0] : row[d], a.shift);
            if (binned) atomicAdd(&s_bins[label * (D + 1) + d], q);
            else atomicAdd(&a.sums[(int64_t)label * D + d], q);
        }
        if (binned) atomicAdd(&s_bins[label * (D + 1) + D], 1ull);
        else atomicAdd(&a.counts[label], 1ull);
    }
    if (changed) atomicAdd(&s_changed, changed);
    __syncthreads();
    if (threadIdx.x == 0 && s_changed) atomicAdd(a.changed, s_changed);
    if (!binned) return;
    for (int i = threadIdx.x; i < k * (D + 1); i += QUAL_BLOCK) {
        const cl_u64 val = s_bins[i];
        if (val == 0) continue;
        const int c = i / (D + 1), d = i % (D + 1);
        if (d < D) atomicAdd(&a.sums[(int64_t)c * D + d], val);
        else atomicAdd(&a.counts[c], val);
    }
}

__global__ __launch_bounds__(QUAL_BLOCK) void cl_finish_kernel(int k, int D, int shift, int64_t *sums, const int64_t *__restrict__ counts,
                                                               float *centres) {
    const int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (i >= (int64_t)k * D) return;
    const int64_t cnt = counts[i / D];
    if (cnt > 0) centres[i] = cl_centre(sums[i], cnt, shift);   // a cluster without members keeps its centre
    sums[i] = 0;
}

__global__ __launch_bounds__(QUAL_BLOCK) void cl_seed_kernel(int64_t n, int D, const float *__restrict__ pos, int64_t vertex, int first,
                                                             float *min_d2) {
    const int64_t w = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (w >= n) return;
    const float d = qual_d2(pos + w * D, pos + vertex * D, 1, D);
    min_d2[w] = first || d < min_d2[w] ? d : min_d2[w];
}

// dst column j = row order[j] of the snapshot
__global__ __launch_bounds__(QUAL_BLOCK) void cl_gather_kernel(int64_t total, int D, const float *__restrict__ pos, const int32_t *__restrict__ order,
                                                               float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (i < total) dst[i] = pos[(int64_t)order[i / D] * D + i % D];
}

// A piece: the sorted columns [begin, end) -- inside one tile, of one cluster.
struct cl_piece {
    int64_t begin, end;
};

struct ClSums {
    const float *pos, *sorted;      // the snapshot and its columns in cluster order
    const int32_t *order;           // sorted column j is vertex order[j]
    const int32_t *rows;            // NULL: row r is vertex r
    const cl_piece *pieces;
    const int64_t *tile_piece;      // the pieces of tile t: [tile_piece[t], tile_piece[t + 1])
    double *part;                   // (batch rows, n_pieces)
    int64_t n, row0, nr, n_pieces, tiles_per_chunk;
    int32_t D, tile_cols;
};

// Wave w of workgroup blockIdx.x owns row row0 + 4 * blockIdx.x + w and meets the tiles [blockIdx.y * tiles_per_chunk, ...).
// part[(row - row0) * n_pieces + p] = the sum over the columns of piece p, the row's own vertex left out.  STAGED as in
// qual_rank_kernel: the tile goes through LDS as D rows of tile_cols columns; otherwise columns are read from memory.
template <bool STAGED>
__global__ __launch_bounds__(QUAL_BLOCK) void cl_sums_kernel(ClSums a) {
    __shared__ float s_tile[STAGED ? CL_SUMS_LDS : 1];
    const int lane = threadIdx.x & 63, D = a.D, tile_cols = a.tile_cols;
    const int64_t local = (int64_t)blockIdx.x * CL_SUMS_WAVES + (threadIdx.x >> 6);
    const bool live = local < a.nr;   // the same in every lane; an idle wave stages its share of the tile and adds nothing
    const int64_t u = live ? (a.rows ? (int64_t)a.rows[a.row0 + local] : a.row0 + local) : 0;
    const float *xu = a.pos + u * D;
    const int64_t n_tiles = (a.n + tile_cols - 1) / tile_cols;
    const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_chunk, t1 = min(n_tiles, t0 + a.tiles_per_chunk);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * tile_cols;
        const int m = (int)min((int64_t)tile_cols, a.n - base);   // the last tile is partial
        if (STAGED) {
            __syncthreads();
            for (int d = 0; d < D; ++d)
                for (int c = threadIdx.x; c < m; c += QUAL_BLOCK) s_tile[d * tile_cols + c] = a.sorted[(base + c) * D + d];
            __syncthreads();
        }
        if (!live) continue;
        for (int64_t p = a.tile_piece[t]; p < a.tile_piece[t + 1]; ++p) {
            const cl_piece pc = a.pieces[p];   // base <= begin < end <= base + m
            double acc = 0.0;
            for (int64_t j = pc.begin + lane; j < pc.end; j += 64) {
                if (a.order[j] == u) continue;
                const float d2 = STAGED ? qual_d2(xu, s_tile + (j - base), tile_cols, D) : qual_d2(xu, a.sorted + j * D, 1, D);
                acc += sqrt((double)d2);
            }
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
            if (lane == 0) a.part[local * a.n_pieces + p] = acc;
        }
    }
}

// sums[r][c] = the pieces of cluster c, [cluster_piece[c], cluster_piece[c + 1]), added in order
__global__ __launch_bounds__(QUAL_BLOCK) void cl_join_kernel(int64_t nr, int k, int64_t n_pieces, const int64_t *__restrict__ cluster_piece,
                                                             const double *__restrict__ part, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * QUAL_BLOCK + threadIdx.x;
    if (i >= nr * k) return;
    const int64_t r = i / k, c = i % k;
    double s = 0.0;
    for (int64_t p = cluster_piece[c]; p < cluster_piece[c + 1]; ++p) s += part[r * n_pieces + p];
    sums[i] = s;
}

// ---- the checks the calls share ------------------------------------------------------------------------------------------
gh_status cl_check_k(gh_qual *h, int64_t k) {
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    const int64_t top = std::min<int64_t>(h->n, CL_MAX_K);
    if (k < 1 || k > top)
        return qual_invalid(h, "k must be in [1, min(n, " + std::to_string(CL_MAX_K) + ")] = [1, " + std::to_string(top) + "], got " + std::to_string(k));
    return GH_OK;
}

}  // namespace

// The scan of the snapshot, once per epoch; a row with a NaN or an infinity is refused.  Declared in qual_handle.h:
// classify.hip refuses the same rows with the same message.
gh_status cl_scan(gh_qual *h) {
    if (h->scan_epoch != h->epoch) {
        const int64_t n = h->n, total = n * h->D;
        uint32_t mx = 0;
        int64_t bad = -1;
        if (h->device < 0) {
            for (int64_t i = 0; i < total; ++i) {
                union { float f; uint32_t u; } b = {h->h_pos[i]};
                const uint32_t a = b.u & 0x7FFFFFFFu;
                if (a >= 0x7F800000u) { if (bad < 0) bad = i / h->D; }
                else mx = std::max(mx, a);
            }
        } else {
            GH_HIP(hipSetDevice(h->device));
            gh_dev<cl_u64> d_out;   // [0] the first bad row, [1] (low word) the greatest bits
            if (!d_out.alloc(16)) { h->err = "hipMalloc failed for the snapshot scan"; return GH_ERR_NOMEM; }
            const cl_u64 init[2] = {~0ull, 0};
            cl_u64 out[2];
            GH_HIP(hipMemcpyAsync(d_out.p, init, 16, hipMemcpyHostToDevice, h->stream));
            const unsigned blocks = (unsigned)std::min<int64_t>(2048, qual_grid(total));
            cl_scan_kernel<<<dim3(blocks), dim3(QUAL_BLOCK), 0, h->stream>>>(n, h->D, h->d_pos.p, (uint32_t *)(d_out.p + 1), d_out.p);
            GH_LAUNCH_CHECK();
            GH_HIP(hipMemcpyAsync(out, d_out.p, 16, hipMemcpyDeviceToHost, h->stream));
            GH_HIP(hipStreamSynchronize(h->stream));
            mx = (uint32_t)out[1];
            bad = out[0] == ~0ull ? -1 : (int64_t)out[0];
        }
        h->max_abs_bits = mx;
        h->bad_row = bad;
        h->scan_epoch = h->epoch;
    }
    if (h->bad_row >= 0) return qual_invalid(h, "position row " + std::to_string(h->bad_row) + " is not finite");
    return GH_OK;
}

namespace {

gh_status cl_check_centres(gh_qual *h, int64_t k, const float *centres) {
    if (!centres) return qual_invalid(h, "centres is NULL");
    for (int64_t i = 0; i < k * h->D; ++i)
        if (!std::isfinite(centres[i])) return qual_invalid(h, "centre " + std::to_string(i / h->D) + " is not finite");
    return GH_OK;
}

// s = 38 - ilogb(M), 0 for M = 0
int cl_shift(const gh_qual *h) {
    union { uint32_t u; float f; } m = {h->max_abs_bits};
    return h->max_abs_bits ? 38 - std::ilogb(m.f) : 0;
}

// ---- the host path -----------------------------------------------------------------------------------------------------
// One assignment; bins != NULL: also the sums and counts, k (D + 1) int64 as (k, D) then k.
void cl_assign_host(const gh_qual *h, int k, const float *centres, int32_t *labels, float *d2, int shift, std::vector<int64_t> *bins) {
    const int D = h->D;
    const float *pos = h->h_pos.data();
    const int64_t slots = (int64_t)k * (D + 1);
    std::vector<std::vector<int64_t>> local;
    std::vector<int64_t> firsts;
    std::mutex mu;
    qual_host_parallel(h->n, 256, [&, D, k, pos, centres, labels, d2, shift, slots](int64_t first, int64_t last) {
        std::vector<int64_t> mine(bins ? (size_t)slots : 0, 0);
        for (int64_t v = first; v < last; ++v) {
            float best = INFINITY;
            int32_t label = 0;
            cl_walk<0>(pos + v * D, centres, D, 0, k, best, label);
            labels[v] = label;
            d2[v] = best;
            if (!bins) continue;
            for (int d = 0; d < D; ++d) mine[(size_t)label * D + d] += cl_quantise(pos[v * D + d], shift);
            mine[(size_t)k * D + label] += 1;
        }
        if (!bins) return;
        std::lock_guard<std::mutex> lock(mu);
        local.push_back(std::move(mine));
    });
    if (!bins) return;
    bins->assign((size_t)slots, 0);
    for (const auto &mine : local)
        for (int64_t i = 0; i < slots; ++i) (*bins)[i] += mine[i];
}

gh_status cl_kmeans_host(gh_qual *h, int k, float *centres, int max_iter, bool accumulate, int32_t *labels, float *d2, int64_t *counts,
                         int32_t *n_iter, int32_t *converged) {
    const int D = h->D, shift = cl_shift(h);
    const int64_t n = h->n;
    std::vector<int32_t> prev;
    std::vector<int64_t> bins;
    int it = 0;
    bool done = false;
    for (;;) {
        cl_assign_host(h, k, centres, labels, d2, shift, accumulate ? &bins : nullptr);
        if (it > 0 && std::equal(labels, labels + n, prev.begin())) { done = true; break; }
        if (it == max_iter) break;
        for (int64_t i = 0; i < (int64_t)k * D; ++i) {
            const int64_t cnt = bins[(size_t)k * D + i / D];
            if (cnt > 0) centres[i] = cl_centre(bins[i], cnt, shift);
        }
        prev.assign(labels, labels + n);
        ++it;
    }
    if (counts) std::copy(bins.begin() + (int64_t)k * D, bins.end(), counts);
    if (n_iter) *n_iter = it;
    if (converged) *converged = done ? 1 : 0;
    return GH_OK;
}

// ---- the device path ---------------------------------------------------------------------------------------------------
gh_status cl_launch_lloyd(gh_qual *h, const ClLloyd &a) {
    const dim3 grid(std::min<unsigned>(CL_LLOYD_BLOCKS, qual_grid(a.n))), block(QUAL_BLOCK);
    if (!gh_dispatch_dim(a.D, [&](auto d, auto) { cl_lloyd_kernel<d()><<<grid, block, 0, h->stream>>>(a); }))
        cl_lloyd_kernel<0><<<grid, block, 0, h->stream>>>(a);
    GH_LAUNCH_CHECK();
    return GH_OK;
}

gh_status cl_kmeans_device(gh_qual *h, int k, float *centres, int max_iter, bool accumulate, int32_t *labels, float *d2, int64_t *counts,
                           int32_t *n_iter, int32_t *converged) {
    const int D = h->D;
    const int64_t n = h->n, kd = (int64_t)k * D;
    GH_HIP(hipSetDevice(h->device));
    gh_dev<float> d_centres, d_d2;
    gh_dev<int32_t> d_lab[2], d_changed;
    gh_dev<int64_t> d_sums, d_counts;
    if (!d_centres.alloc(4 * (size_t)kd) || !d_d2.alloc(4 * (size_t)n) || !d_lab[0].alloc(4 * (size_t)n) || !d_lab[1].alloc(4 * (size_t)n) ||
        !d_changed.alloc(4) || !d_sums.alloc(8 * (size_t)kd) || !d_counts.alloc(8 * (size_t)k)) {
        h->err = "hipMalloc failed for " + std::to_string(12 * n + 12 * kd + 8 * k) + " bytes of labels, centres and bins";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_centres.p, centres, 4 * (size_t)kd, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemsetAsync(d_sums.p, 0, 8 * (size_t)kd, h->stream));
    ClLloyd a{};
    a.pos = h->d_pos.p; a.centres = d_centres.p; a.d2 = d_d2.p;
    a.sums = (cl_u64 *)d_sums.p; a.counts = (cl_u64 *)d_counts.p; a.changed = d_changed.p;
    a.n = n; a.D = D; a.k = k; a.shift = cl_shift(h);
    a.staged = D <= CL_CENTRE_LDS;
    a.tile_c = a.staged ? std::max(1, std::min(k, CL_CENTRE_LDS / D)) : k;
    a.accumulate = accumulate;
    a.lds_bins = (int64_t)k * (D + 1) <= CL_BIN_SLOTS;
    int it = 0, cur = 0;
    bool done = false;
    for (;;) {
        GH_HIP(hipMemsetAsync(d_counts.p, 0, 8 * (size_t)k, h->stream));
        GH_HIP(hipMemsetAsync(d_changed.p, 0, 4, h->stream));
        a.labels = d_lab[cur].p;
        a.prev = it > 0 ? d_lab[cur ^ 1].p : nullptr;
        GH_TRY_ST(cl_launch_lloyd(h, a));
        if (it > 0) {
            int32_t changed = 0;
            GH_HIP(hipMemcpyAsync(&changed, d_changed.p, 4, hipMemcpyDeviceToHost, h->stream));
            GH_HIP(hipStreamSynchronize(h->stream));
            if (changed == 0) { done = true; break; }
        }
        if (it == max_iter) break;
        cl_finish_kernel<<<dim3(qual_grid(kd)), dim3(QUAL_BLOCK), 0, h->stream>>>(k, D, a.shift, d_sums.p, d_counts.p, d_centres.p);
        GH_LAUNCH_CHECK();
        cur ^= 1;
        ++it;
    }
    GH_HIP(hipMemcpyAsync(labels, d_lab[cur].p, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipMemcpyAsync(d2, d_d2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (accumulate) GH_HIP(hipMemcpyAsync(centres, d_centres.p, 4 * (size_t)kd, hipMemcpyDeviceToHost, h->stream));
    if (counts) GH_HIP(hipMemcpyAsync(counts, d_counts.p, 8 * (size_t)k, hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    if (n_iter) *n_iter = it;
    if (converged) *converged = done ? 1 : 0;
    return GH_OK;
}

void cl_sums_host(const gh_qual *h, int k, const int32_t *labels, int64_t n_rows, const int32_t *rows, double *sums) {
    const int64_t n = h->n;
    const int D = h->D;
    const float *pos = h->h_pos.data();
    qual_host_parallel(n_rows, 1, [=](int64_t first, int64_t last) {
        for (int64_t r = first; r < last; ++r) {
            const int64_t u = rows ? rows[r] : r;
            double *out = sums + r * k;
            std::fill(out, out + k, 0.0);
            for (int64_t w = 0; w < n; ++w)
                if (w != u) out[labels[w]] += sqrt((double)qual_d2(pos + u * D, pos + w * D, 1, D));
        }
    });
}

gh_status cl_sums_device(gh_qual *h, int k, const int32_t *labels, int64_t n_rows, const int32_t *rows, double *sums) {
    const int64_t n = h->n;
    const int D = h->D;
    // the counting sort by label: cluster c owns the sorted columns [start[c], start[c + 1]), vertex ids ascending
    std::vector<int64_t> start((size_t)k + 1, 0);
    for (int64_t w = 0; w < n; ++w) start[(size_t)labels[w] + 1] += 1;
    for (int c = 0; c < k; ++c) start[c + 1] += start[c];
    std::vector<int32_t> order((size_t)n);
    {
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (int64_t w = 0; w < n; ++w) order[(size_t)fill[labels[w]]++] = (int32_t)w;
    }
    // the tile: D rows of tile_cols columns in CL_SUMS_LDS floats, tile_cols a multiple of 64; none fits: no staging
    const int fit = (int)std::min<int64_t>(CL_SUMS_TILE, CL_SUMS_LDS / D / 64 * 64);
    const bool staged = fit >= 64;
    const int tile_cols = staged ? fit : CL_SUMS_TILE;
    const int64_t n_tiles = (n + tile_cols - 1) / tile_cols;
    // the pieces, in column order: a cluster's segment cut at the tile boundaries
    std::vector<cl_piece> pieces;
    std::vector<int64_t> tile_piece((size_t)n_tiles + 1, 0), cluster_piece((size_t)k + 1, 0);
    for (int c = 0; c < k; ++c) {
        for (int64_t b = start[c]; b < start[c + 1];) {
            const int64_t e = std::min(start[c + 1], (b / tile_cols + 1) * tile_cols);
            pieces.push_back({b, e});
            tile_piece[(size_t)(b / tile_cols) + 1] += 1;
            b = e;
        }
        cluster_piece[c + 1] = (int64_t)pieces.size();
    }
    for (int64_t t = 0; t < n_tiles; ++t) tile_piece[t + 1] += tile_piece[t];
    const int64_t n_pieces = (int64_t)pieces.size();   // >= 1: n >= 1
    // rows per batch: the partial sums and the pair tests of one launch stay bounded
    int64_t batch = std::min<int64_t>(CL_SUMS_PART_BYTES / (8 * std::max<int64_t>(n_pieces, k)), CL_SUMS_LAUNCH_PAIRS / n);
    batch = std::max<int64_t>(CL_SUMS_WAVES, std::min<int64_t>(batch / CL_SUMS_WAVES * CL_SUMS_WAVES, (n_rows + CL_SUMS_WAVES - 1) / CL_SUMS_WAVES * CL_SUMS_WAVES));
    GH_HIP(hipSetDevice(h->device));
    gh_dev<float> d_sorted;
    gh_dev<int32_t> d_order, d_rows;
    gh_dev<cl_piece> d_pieces;
    gh_dev<int64_t> d_tile_piece, d_cluster_piece;
    gh_dev<double> d_part, d_sums;
    if (!d_sorted.alloc(4 * (size_t)(n * D)) || !d_order.alloc(4 * (size_t)n) || (rows && !d_rows.alloc(4 * (size_t)n_rows)) ||
        !d_pieces.alloc(sizeof(cl_piece) * (size_t)n_pieces) || !d_tile_piece.alloc(8 * (size_t)(n_tiles + 1)) ||
        !d_cluster_piece.alloc(8 * (size_t)(k + 1)) || !d_part.alloc(8 * (size_t)(batch * n_pieces)) || !d_sums.alloc(8 * (size_t)(batch * k))) {
        h->err = "hipMalloc failed for " + std::to_string(4 * n * D + 8 * batch * (n_pieces + k)) + " bytes of sorted columns and partial sums";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_order.p, order.data(), 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (rows) GH_HIP(hipMemcpyAsync(d_rows.p, rows, 4 * (size_t)n_rows, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_pieces.p, pieces.data(), sizeof(cl_piece) * (size_t)n_pieces, hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_tile_piece.p, tile_piece.data(), 8 * (size_t)(n_tiles + 1), hipMemcpyHostToDevice, h->stream));
    GH_HIP(hipMemcpyAsync(d_cluster_piece.p, cluster_piece.data(), 8 * (size_t)(k + 1), hipMemcpyHostToDevice, h->stream));
    cl_gather_kernel<<<dim3(qual_grid(n * D)), dim3(QUAL_BLOCK), 0, h->stream>>>(n * D, D, h->d_pos.p, d_order.p, d_sorted.p);
    GH_LAUNCH_CHECK();
    ClSums a{};
    a.pos = h->d_pos.p; a.sorted = d_sorted.p; a.order = d_order.p; a.rows = rows ? d_rows.p : nullptr;
    a.pieces = d_pieces.p; a.tile_piece = d_tile_piece.p; a.part = d_part.p;
    a.n = n; a.n_pieces = n_pieces; a.D = D; a.tile_cols = tile_cols;
    for (int64_t row0 = 0; row0 < n_rows; row0 += batch) {
        const int64_t nr = std::min(batch, n_rows - row0);
        const int64_t blocks = (nr + CL_SUMS_WAVES - 1) / CL_SUMS_WAVES;
        // a few rows only (a sample, a small layout): their columns are split so that every compute unit has work
        const int64_t chunks = std::max<int64_t>(1, std::min(n_tiles, CL_SUMS_MIN_BLOCKS / blocks));
        a.tiles_per_chunk = (n_tiles + chunks - 1) / chunks;
        const int64_t used = (n_tiles + a.tiles_per_chunk - 1) / a.tiles_per_chunk;   // <= 2048 < 65536: grid.y
        a.row0 = row0; a.nr = nr;
        if (staged) cl_sums_kernel<true><<<dim3((unsigned)blocks, (unsigned)used), dim3(QUAL_BLOCK), 0, h->stream>>>(a);
        else cl_sums_kernel<false><<<dim3((unsigned)blocks, (unsigned)used), dim3(QUAL_BLOCK), 0, h->stream>>>(a);
        GH_LAUNCH_CHECK();
        cl_join_kernel<<<dim3(qual_grid(nr * k)), dim3(QUAL_BLOCK), 0, h->stream>>>(nr, k, n_pieces, d_cluster_piece.p, d_part.p, d_sums.p);
        GH_LAUNCH_CHECK();
        GH_HIP(hipMemcpyAsync(sums + row0 * k, d_sums.p, 8 * (size_t)(nr * k), hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));   // d_sums is written again by the next batch
    }
    return GH_OK;
}

gh_status cl_kmeans_call(gh_qual *h, int64_t k, float *centres, int64_t max_iter, bool accumulate, int32_t *labels, float *d2, int64_t *counts,
                         int32_t *n_iter, int32_t *converged) {
    GH_TRY_ST(cl_check_k(h, k));
    if (max_iter < 0) return qual_invalid(h, "max_iter must be >= 0, got " + std::to_string(max_iter));
    if (accumulate && h->n > CL_MAX_N) return qual_invalid(h, "exact centre sums hold up to 2^24 vertices, got " + std::to_string(h->n));
    if (!labels || !d2) return qual_invalid(h, "labels or d2 is NULL");
    GH_TRY_ST(cl_check_centres(h, k, centres));
    GH_TRY_ST(cl_scan(h));
    if (h->device < 0) return cl_kmeans_host(h, (int)k, centres, (int)max_iter, accumulate, labels, d2, counts, n_iter, converged);
    return cl_kmeans_device(h, (int)k, centres, (int)max_iter, accumulate, labels, d2, counts, n_iter, converged);
}

}  // namespace

extern "C" gh_status gh_qual_kmeans_assign(gh_qual_handle h, int32_t k, const float *centres, int32_t *labels, float *d2) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    // without bins nothing is written to the centres
    return cl_kmeans_call(h, k, const_cast<float *>(centres), 0, false, labels, d2, nullptr, nullptr, nullptr);
}

extern "C" gh_status gh_qual_kmeans(gh_qual_handle h, int32_t k, float *centres, int32_t max_iter, int32_t *labels, float *d2, int64_t *counts,
                                    int32_t *n_iter, int32_t *converged) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    return cl_kmeans_call(h, k, centres, max_iter, true, labels, d2, counts, n_iter, converged);
}

extern "C" gh_status gh_qual_position_rows(gh_qual_handle h, int64_t n_rows, const int32_t *rows, float *out) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (n_rows < 0) return qual_invalid(h, "n_rows must be >= 0, got " + std::to_string(n_rows));
    if (n_rows == 0) return GH_OK;
    if (!rows || !out) return qual_invalid(h, "rows or out is NULL");
    for (int64_t r = 0; r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= h->n) return qual_invalid(h, "row " + std::to_string(r) + " has a vertex id outside [0, n)");
    const int D = h->D;
    if (h->device < 0) {
        for (int64_t r = 0; r < n_rows; ++r) std::copy(h->h_pos.begin() + (int64_t)rows[r] * D, h->h_pos.begin() + ((int64_t)rows[r] + 1) * D, out + r * D);
        return GH_OK;
    }
    GH_HIP(hipSetDevice(h->device));
    gh_dev<int32_t> d_rows;
    gh_dev<float> d_out;
    if (!d_rows.alloc(4 * (size_t)n_rows) || !d_out.alloc(4 * (size_t)(n_rows * D))) {
        h->err = "hipMalloc failed for " + std::to_string(4 * n_rows * (D + 1)) + " bytes of rows";
        return GH_ERR_NOMEM;
    }
    GH_HIP(hipMemcpyAsync(d_rows.p, rows, 4 * (size_t)n_rows, hipMemcpyHostToDevice, h->stream));
    cl_gather_kernel<<<dim3(qual_grid(n_rows * D)), dim3(QUAL_BLOCK), 0, h->stream>>>(n_rows * D, D, h->d_pos.p, d_rows.p, d_out.p);
    GH_LAUNCH_CHECK();
    GH_HIP(hipMemcpyAsync(out, d_out.p, 4 * (size_t)(n_rows * D), hipMemcpyDeviceToHost, h->stream));
    GH_HIP(hipStreamSynchronize(h->stream));
    return GH_OK;
}

extern "C" gh_status gh_qual_kmeans_seed_step(gh_qual_handle h, int64_t vertex, int32_t first, float *min_d2) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    if (h->D < 1) return qual_invalid(h, "no positions were set");
    if (vertex < 0 || vertex >= h->n) return qual_invalid(h, "vertex " + std::to_string(vertex) + " is outside [0, n)");
    if (!min_d2) return qual_invalid(h, "min_d2 is NULL");
    if (!first && h->seed_epoch != h->epoch) return qual_invalid(h, "no seed step with first set came before on these positions");
    GH_TRY_ST(cl_scan(h));
    const int64_t n = h->n;
    const int D = h->D;
    if (h->device < 0) {
        if (first) h->h_min_d2.assign((size_t)n, 0.0f);
        const float *pos = h->h_pos.data();
        float *m = h->h_min_d2.data();
        qual_host_parallel(n, 4096, [=](int64_t a, int64_t b) {
            for (int64_t w = a; w < b; ++w) {
                const float d = qual_d2(pos + w * D, pos + vertex * D, 1, D);
                m[w] = first || d < m[w] ? d : m[w];
            }
        });
        std::copy(m, m + n, min_d2);
    } else {
        GH_HIP(hipSetDevice(h->device));
        if (h->d_min_d2.bytes < 4 * (size_t)n || !h->d_min_d2.p) {
            if (!first) return qual_invalid(h, "no seed step with first set came before on these positions");
            if (!h->d_min_d2.alloc(4 * (size_t)n)) { h->err = "hipMalloc failed for " + std::to_string(4 * n) + " bytes of minima"; return GH_ERR_NOMEM; }
        }
        cl_seed_kernel<<<dim3(qual_grid(n)), dim3(QUAL_BLOCK), 0, h->stream>>>(n, D, h->d_pos.p, vertex, first, h->d_min_d2.p);
        GH_LAUNCH_CHECK();
        GH_HIP(hipMemcpyAsync(min_d2, h->d_min_d2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        GH_HIP(hipStreamSynchronize(h->stream));
    }
    h->seed_epoch = h->epoch;
    return GH_OK;
}

extern "C" gh_status gh_qual_cluster_distance_sums(gh_qual_handle h, int32_t k, const int32_t *labels, int64_t n_rows, const int32_t *rows,
                                                   double *sums) {
    if (!h) { qual_set_create_error("handle is NULL"); return GH_ERR_INVALID; }
    GH_TRY_ST(cl_check_k(h, k));
    if (!labels) return qual_invalid(h, "labels is NULL");
    if (!rows) n_rows = h->n;
    if (n_rows < 0) return qual_invalid(h, "n_rows must be >= 0, got " + std::to_string(n_rows));
    for (int64_t w = 0; w < h->n; ++w)
        if (labels[w] < 0 || labels[w] >= k) return qual_invalid(h, "label " + std::to_string(w) + " is outside [0, k)");
    for (int64_t r = 0; rows && r < n_rows; ++r)
        if (rows[r] < 0 || rows[r] >= h->n) return qual_invalid(h, "row " + std::to_string(r) + " has a vertex id outside [0, n)");
    GH_TRY_ST(cl_scan(h));
    if (n_rows == 0) return GH_OK;
    if (!sums) return qual_invalid(h, "sums is NULL");
    if (h->device < 0) cl_sums_host(h, k, labels, n_rows, rows, sums);
    else GH_TRY_ST(cl_sums_device(h, k, labels, n_rows, rows, sums));
    return GH_OK;
}
